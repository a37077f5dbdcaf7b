"""Stochastic rounding in the optimizer step on a group of SEPARATE table tensors (sparse_row_update_grouped /
sparse_row_adam_grouped(stochastic_rounding=True, seeds=[...], step=...), the two updaters, the two torch ops).

The contract: ONE SEED PER TABLE, and the bits of entry k are those of (seeds[t], step, row inside table t, column).  So
a grouped stochastic step equals, bit for bit in tables and states, num_tables single-table stochastic steps with
seed = seeds[t] at the same step, run at the group's lane width -- the oracle of most tests here, fed the entries of
GroupedGrad.per_table() -- and, independently of the library's single-table kernel, the numpy model of
tests/stochastic_rounding_reference.py.  A table's trajectory depends neither on the group it is in nor on its place
there.

The case builders are those of tests/test_gpu_grouped_sparse_update.py (row counts (1, 5, 70) and (3, 1, 1, 64, 2): with
every row named each table boundary falls inside one wavefront's entries).  Every test here needs `seeds`, which the
grouped step did not take before."""
import numpy as np
import pytest
import torch

import stochastic_rounding_reference as S
from test_gpu_grouped_sparse_update import (BETAS, DEV, EPS, FIVE, GROUPS, LR, Side, entries_of, hashed, hashed_ints, ibits,
                                            check_untouched, lookups, placed, rule_id, same_bits, updater_tensors)

pytestmark = pytest.mark.gpu

SIXTEEN = (torch.float16, torch.bfloat16)
# distinct seeds: one at or above 2^63, one with a non-zero high word, small ones, zero
SEEDS = (0xF00DFACE12345678, 0x0000000500000007, 3, 0, 0x8000000000000000, 41, 2 ** 64 - 1)
STEP = 2 ** 32 + 5          # (the step's high word goes into the key: a step at or above 2^32 reaches it)


@pytest.fixture(scope="module")
def ce():
    import cuembed_amd
    return cuembed_amd


def seeds_for(rows):
    return list(SEEDS[:len(rows)])


def short(v):
    return str(v).replace("torch.", "")


def grouped_step(ce, group, side, rule, opts, ids, rows, seeds, step, **count):
    if rule in ("adam", "rowwise_adam"):
        ce.sparse_row_adam_grouped(group, ids, rows, exp_avg=side.states[0], exp_avg_sq=side.states[1], lr=LR, betas=BETAS,
                                   eps=EPS, rowwise=rule == "rowwise_adam", stochastic_rounding=True, seeds=seeds,
                                   step=step, **opts, **count)
    else:
        ce.sparse_row_update_grouped(group, ids, rows, rule=rule, lr=LR, eps=EPS,
                                     states=side.states[0] if side.states else None, stochastic_rounding=True, seeds=seeds,
                                     step=step, **count)


def per_table_steps(ce, group, side, rule, opts, ids, rows, valid, seeds, step):
    """The oracle: the entries of GroupedGrad.per_table(), one single-table STOCHASTIC call per table with that table's
    seed."""
    last = torch.tensor([valid - 1], dtype=ids.dtype, device=DEV)
    per_table = ce.GroupedGrad(ids, rows, last, group.row_base, group.row_base_device).per_table()
    assert sum(i.numel() for i, _ in per_table) == valid
    for t, (local_ids, local_rows) in enumerate(per_table):
        kw = dict(stochastic_rounding=True, seed=seeds[t], step=step)
        if rule in ("adam", "rowwise_adam"):
            ce.sparse_row_adam(side.tables[t], local_ids, local_rows, exp_avg=side.states[0][t], exp_avg_sq=side.states[1][t],
                               lr=LR, betas=BETAS, eps=EPS, rowwise=rule == "rowwise_adam", **opts, **kw)
        else:
            ce.sparse_row_update(side.tables[t], local_ids, local_rows, rule=rule, lr=LR, eps=EPS,
                                 state=side.states[0][t] if side.states else None, **kw)


def compare(ce, rows, width, dtype, rule, opts, coverage="all", index=torch.int32, count_kind="all", misaligned=(),
            steps=2, seeds=None):
    """`steps` consecutive grouped stochastic steps (step numbers STEP, STEP + 1, ...) against the per-table chain on
    clones of the alignment that makes the single-table calls run at the group's lane width; returns the grouped side."""
    total = sum(rows)
    seeds = seeds_for(rows) if seeds is None else seeds
    named = entries_of(rows, coverage)
    mine = Side(rows, width, dtype, rule, misaligned)
    theirs = Side(rows, width, dtype, rule, range(len(rows)) if misaligned else ())
    group, their_group = ce.TableGroup(mine.tables), ce.TableGroup(theirs.tables)
    assert same_bits(mine.tensors(), theirs.tensors())
    for n in range(steps):
        valid = len(named)
        tail = 0 if count_kind == "all" else 3
        ids = torch.tensor(named + [total + 5 if count_kind == "word" else -1] * tail, dtype=index, device=DEV)
        grads = placed(0.25 * hashed((valid + tail) * width, 1000 + n), (valid + tail, width), dtype)
        count = {"all": {}, "host": dict(count=valid),
                 "word": dict(count=torch.tensor([valid], dtype=torch.int64, device=DEV)),
                 "last_id": dict(last_id=torch.tensor([valid - 1], dtype=index, device=DEV))}[count_kind]
        before = mine.clones()
        grouped_step(ce, group, mine, rule, opts, ids, grads, seeds, STEP + n, **count)
        per_table_steps(ce, their_group, theirs, rule, opts, ids, grads, valid, seeds, STEP + n)
        torch.cuda.synchronize()
        assert same_bits(mine.tensors(), theirs.tensors()), "step %d differs from the per-table stochastic calls" % n
        check_untouched(rows, width, mine, before, named)
        assert not same_bits(mine.tables, before[:len(rows)]), "the step changed nothing"
    return mine


# ---- 1. the per-table chain -----------------------------------------------------------------------------------------------
# what varies with the width: the ids' type, the count source and the coverage (all of each appear for every rule)
VARIANT = {8: dict(index=torch.int64, count_kind="all", coverage="all"),
           36: dict(index=torch.int32, count_kind="last_id", coverage="skip_middle"),
           128: dict(index=torch.int64, count_kind="word", coverage="all")}


@pytest.mark.parametrize("rule", FIVE, ids=rule_id)
@pytest.mark.parametrize("width", [8, 36, 128])
@pytest.mark.parametrize("dtype", SIXTEEN, ids=short)
@pytest.mark.parametrize("rows", GROUPS, ids=lambda r: "x".join(map(str, r)))
def test_a_grouped_stochastic_step_is_the_per_table_stochastic_chain(ce, rows, dtype, width, rule):
    """All five rules, both 16-bit types, lanes of 16 bytes (widths 8, 128) and 8 (36), two consecutive steps; int32 and
    int64 ids, every row or a middle table without an entry, and the count as nothing / last_id / a device word with a
    tail of out-of-range ids behind it."""
    compare(ce, rows, width, dtype, rule[0], rule[1], **VARIANT[width])


@pytest.mark.parametrize("rule", FIVE, ids=rule_id)
@pytest.mark.parametrize("width, slices", [(1000, 4), (2056, 0)])
@pytest.mark.parametrize("dtype", SIXTEEN, ids=short)
def test_rows_wider_than_a_lane_group(ce, dtype, width, slices, rule):
    """The walk's other two bodies: four slices per lane (125 lanes of 16 bytes) and the run-time loop (257 lanes), with a
    host-known count below the array's size."""
    assert ce.sparse_row_update_launch_shape(dtype, width, 71)["slices_per_lane"] == slices
    compare(ce, GROUPS[1], width, dtype, rule[0], rule[1], count_kind="host", steps=1)


# ---- 2. the naming, against the numpy model ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype, kind", [(torch.float16, "fp16"), (torch.bfloat16, "bf16")], ids=["float16", "bfloat16"])
def test_sgd_equals_the_numpy_model_with_the_tables_own_seed_and_local_rows(ce, dtype, kind):
    """SGD on a small group against stochastic_rounding_reference: fields(seeds[t], step, LOCAL rows, width) per table.
    Nothing of the library's single-table kernel takes part."""
    rows, width = GROUPS[0], 24
    seeds = seeds_for(rows)
    side = Side(rows, width, dtype, "sgd")
    before = [ibits(t).cpu().numpy().view(np.uint16).copy() for t in side.tables]
    named = entries_of(rows, "skip_middle")
    ids = torch.tensor(named, dtype=torch.int32, device=DEV)
    grads = placed(0.25 * hashed(len(named) * width, 31), (len(named), width), dtype)
    ce.sparse_row_update_grouped(ce.TableGroup(side.tables), ids, grads, rule="sgd", lr=LR, stochastic_rounding=True,
                                 seeds=seeds, step=STEP)
    torch.cuda.synchronize()
    g_bits = ibits(grads).cpu().numpy().view(np.uint16)
    base = 0
    for t, n in enumerate(rows):
        at = [k for k, r in enumerate(named) if base <= r < base + n]
        local = [named[k] - base for k in at]
        want = S.sgd(before[t], local, g_bits[at], LR, kind, seed=seeds[t], step=STEP) if at else before[t]
        got = ibits(side.tables[t]).cpu().numpy().view(np.uint16)
        assert np.array_equal(got, want), "table %d" % t
        if at:      # and the rounding is not the nearest one everywhere
            assert not np.array_equal(got, S.sgd(before[t], local, g_bits[at], LR, kind))
        base += n


# ---- 3. the seeds are what is read -------------------------------------------------------------------------------------------
def twin_step(ce, dtype, seeds, rule="sgd"):
    """Two tables with the same contents and the same gradient rows, stepped with `seeds`; returns the two tables."""
    n, width = 40, 16
    values = hashed(n * width, 5)
    tables = [placed(values, (n, width), dtype) for _ in range(2)]
    one = 0.25 * hashed(n * width, 6)
    grads = placed(torch.cat([one, one]), (2 * n, width), dtype)
    ids = torch.arange(2 * n, dtype=torch.int32, device=DEV)
    ce.sparse_row_update_grouped(ce.TableGroup(tables), ids, grads, rule=rule, lr=LR, stochastic_rounding=True, seeds=seeds,
                                 step=STEP)
    torch.cuda.synchronize()
    return tables


@pytest.mark.parametrize("dtype", SIXTEEN, ids=short)
def test_the_seeds_are_what_is_read(ce, dtype):
    a, b = SEEDS[0], SEEDS[1]
    same = twin_step(ce, dtype, [a, a])
    assert same_bits([same[0]], [same[1]])                 # same contents, same gradient, same seed: same bits
    ab = twin_step(ce, dtype, [a, b])
    assert not same_bits([ab[0]], [ab[1]])                 # different seeds: different bits
    assert same_bits([ab[0]], [same[0]])                   # (table 0 does not see table 1's seed)
    ba = twin_step(ce, dtype, [b, a])
    assert same_bits([ba[0]], [ab[1]]) and same_bits([ba[1]], [ab[0]])     # swapping the seeds swaps the outcome


# ---- 4. the group's composition does not matter ----------------------------------------------------------------------------
@pytest.mark.parametrize("rule", (FIVE[0], FIVE[4]), ids=rule_id)
def test_a_tables_bits_do_not_depend_on_its_group_or_its_place_in_it(ce, rule):
    """One table as member 0 of a group of 2 and as member 3 of a group of 5 (all tables aligned): same seed, same
    gradient rows for its entries -> the same bits in the table and in its state."""
    rule, opts = rule
    n, width, dtype, seed = 64, 8, torch.float16, SEEDS[0]
    own = 0.25 * hashed(n * width, 70)
    results = []
    for rows, member in (((n, 7), 0), ((3, 1, 2, n, 9), 3)):
        side = Side(rows, width, dtype, rule, salt=10 * len(rows))
        watched = Side((n,), width, dtype, rule, salt=999)        # the watched table and its state: the same in both groups
        side.tables[member] = watched.tables[0]
        for k in range(len(side.states)):
            side.states[k][member] = watched.states[k][0]
        seeds = [11 + t for t in range(len(rows))]
        seeds[member] = seed
        chunks = [own if t == member else 0.25 * hashed(m * width, 80 + t) for t, m in enumerate(rows)]
        grads = placed(torch.cat(chunks), (sum(rows), width), dtype)
        ids = torch.arange(sum(rows), dtype=torch.int64, device=DEV)
        grouped_step(ce, ce.TableGroup(side.tables), side, rule, opts, ids, grads, seeds, STEP)
        torch.cuda.synchronize()
        results.append([side.tables[member]] + [plane[member] for plane in side.states])
    assert same_bits(results[0], results[1])


# ---- 5. alignment ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", FIVE, ids=rule_id)
@pytest.mark.parametrize("dtype, width", [(torch.float16, 8), (torch.bfloat16, 36)], ids=short)
def test_one_table_4_bytes_off_narrows_the_lanes_and_keeps_the_bits(ce, dtype, width, rule):
    """One table of the group is a view 4 bytes off a 16-byte boundary: the whole group runs with 4-byte lanes, and
    equals the chain on clones that are all 4 bytes off.  For SGD and Adagrad, whose arithmetic has no order, the result
    also equals the aligned group's: the stochastic bits do not depend on the lane width."""
    rows = GROUPS[0]
    assert ce.TableGroup(Side(rows, width, dtype, "sgd", (1,)).tables).lane_bytes() == 4
    narrow = compare(ce, rows, width, dtype, rule[0], rule[1], misaligned=(1,))
    if rule[0] in ("sgd", "adagrad"):
        wide = compare(ce, rows, width, dtype, rule[0], rule[1])
        assert same_bits(narrow.tensors(), wide.tensors())


# ---- 6. the step's sources ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", (FIVE[1], FIVE[3]), ids=rule_id)
def test_an_immediate_step_and_a_device_word_give_the_same_bits(ce, rule):
    rule, opts = rule
    rows, width, dtype = GROUPS[1], 8, torch.bfloat16
    ids = torch.arange(sum(rows), dtype=torch.int32, device=DEV)
    grads = placed(0.25 * hashed(ids.numel() * width, 12), (ids.numel(), width), dtype)
    sides = []
    for step in (STEP, torch.tensor([STEP], dtype=torch.int64, device=DEV), STEP + 1):
        side = Side(rows, width, dtype, rule)
        grouped_step(ce, ce.TableGroup(side.tables), side, rule, opts, ids, grads, seeds_for(rows), step)
        sides.append(side)
    torch.cuda.synchronize()
    assert same_bits(sides[0].tensors(), sides[1].tensors())
    assert not same_bits(sides[0].tables, sides[2].tables)       # (and the step is read: another step, other bits)


def stochastic_updater(optim, group, rule, opts, seeds):
    if rule in ("adam", "rowwise_adam"):
        return optim.GroupSparseAdamUpdater(group, LR, betas=BETAS, eps=EPS, weight_decay=opts["weight_decay"],
                                            rowwise=rule == "rowwise_adam", stochastic_rounding=True, seeds=seeds)
    return optim.GroupSparseUpdater(group, rule, LR, eps=EPS, initial_accumulator_value=0.125, stochastic_rounding=True,
                                    seeds=seeds)


@pytest.mark.parametrize("rule", (FIVE[0], FIVE[3]), ids=rule_id)
def test_the_updaters_advance_the_rounding_step_once_per_apply(ce, rule):
    """.rounding_step: an int64 device word, 0 at first, + 1 per apply -- also for a gradient without entries."""
    from cuembed_amd import optim
    rows, width, dtype = GROUPS[0], 8, torch.float16
    group = ce.TableGroup(Side(rows, width, dtype, "sgd").tables)
    u = stochastic_updater(optim, group, rule[0], rule[1], seeds_for(rows))
    assert u.rounding_step.dtype == torch.int64 and u.rounding_step.is_cuda and u.rounding_step.item() == 0
    ids = torch.arange(sum(rows), dtype=torch.int32, device=DEV)
    grads = placed(0.25 * hashed(ids.numel() * width, 13), (ids.numel(), width), dtype)
    last = torch.tensor([ids.numel() - 1], dtype=torch.int32, device=DEV)
    u.apply(ce.GroupedGrad(ids, grads, last, group.row_base, group.row_base_device))
    assert u.rounding_step.item() == 1
    before = [t.clone() for t in updater_tensors(u)]
    u.apply(ce.GroupedGrad(ids[:0], grads[:0], torch.tensor([-1], dtype=torch.int32, device=DEV), group.row_base,
                           group.row_base_device))
    assert u.rounding_step.item() == 2
    assert same_bits(updater_tensors(u), before)
    # without the feature's keywords the updater rounds to nearest and owns no step, as before
    assert optim.GroupSparseUpdater(group, "sgd", LR).rounding_step is None


# ---- 7. the updaters ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", FIVE, ids=rule_id)
@pytest.mark.parametrize("csr, mode", [(True, "sum"), (False, "mean"), (True, "mean"), (False, "sum")],
                         ids=["csr_sum", "fixed_mean", "csr_mean", "fixed_sum"])
def test_three_updater_steps_equal_one_single_table_updater_per_table(ce, csr, mode, rule):
    """Three backward_and_apply steps of GroupSparseUpdater / GroupSparseAdamUpdater with seeds against num_tables
    SparseUpdater / SparseAdamUpdater(seed=seeds[t]) fed GroupedGrad.per_table(): the step word of the group and those of
    the per-table updaters count alike, and so do the Adam clocks."""
    from cuembed_amd import optim
    rule, opts = rule
    rows, width, dtype, batch = GROUPS[1], 8, torch.float16, 5
    seeds = seeds_for(rows)
    mine, theirs = Side(rows, width, dtype, "sgd"), Side(rows, width, dtype, "sgd")
    u = stochastic_updater(optim, ce.TableGroup(mine.tables), rule, opts, seeds)
    if rule in ("adam", "rowwise_adam"):
        singles = [optim.SparseAdamUpdater(t, LR, betas=BETAS, eps=EPS, weight_decay=opts["weight_decay"],
                                           rowwise=rule == "rowwise_adam", stochastic_rounding=True, seed=seeds[k])
                   for k, t in enumerate(theirs.tables)]
    else:
        singles = [optim.SparseUpdater(t, rule, LR, eps=EPS, initial_accumulator_value=0.125, stochastic_rounding=True,
                                       seed=seeds[k]) for k, t in enumerate(theirs.tables)]
    start = [t.clone() for t in mine.tables]
    for n in range(3):
        idx, offsets = lookups(rows, batch, csr, salt=20 * n)
        grad_y = placed(hashed(batch * len(rows) * width, 77 + n), (batch, len(rows), width), dtype)
        grad = u.backward_and_apply(grad_y, idx, offsets, mode=mode)
        for single, (local_ids, local_rows) in zip(singles, grad.per_table()):
            single.apply(local_ids, local_rows)
    torch.cuda.synchronize()
    assert u.rounding_step.item() == 3 and all(s.rounding_step.item() == 3 for s in singles)
    want = list(theirs.tables)
    if rule in ("adam", "rowwise_adam"):
        want += [s.exp_avg for s in singles] + [s.exp_avg_sq for s in singles]
    elif rule != "sgd":
        want += [s.state for s in singles]
    assert same_bits(updater_tensors(u), want)
    assert not same_bits(mine.tables, start)


# ---- 8. capture ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", FIVE, ids=rule_id)
def test_a_captured_stochastic_step_replays_like_eager_steps(ce, rule):
    """forward + backward_and_apply with seeds captured in a HIP graph: nothing is read back and nothing is allocated for
    the seeds or the step word, or the capture would fail.  One eager warm-up step and three replays equal four eager
    steps bit for bit, which needs fresh bits -- the step word advanced on the device -- at every replay.  (grad_y holds
    multiples of 1/8, so the backward's sums are exact whatever their association.)"""
    from cuembed_amd import optim
    rule, opts = rule
    rows, width, dtype, batch = GROUPS[1], 8, torch.float16, 6
    idx, offsets = lookups(rows, batch, True, salt=3)
    grad_y = placed(((hashed_ints(batch * len(rows) * width, 5) % 33) - 16).double() / 8.0, (batch, len(rows), width), dtype)

    def fresh():
        return stochastic_updater(optim, ce.TableGroup(Side(rows, width, dtype, "sgd").tables), rule, opts, seeds_for(rows))

    out = {}

    def step(u):
        out["y"] = ce.embedding_forward_grouped(u.group, idx, offsets)
        u.backward_and_apply(grad_y, idx, offsets)

    captured, eager = fresh(), fresh()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step(captured)                                   # warm-up outside capture (library / module loading)
        torch.cuda.current_stream().synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            step(captured)
    torch.cuda.synchronize()
    after_warm_up = [t.clone() for t in updater_tensors(captured)]
    assert captured.rounding_step.item() == 1            # (capturing runs nothing)
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    for _ in range(4):
        step(eager)
    torch.cuda.synchronize()
    assert captured.rounding_step.item() == 4 and eager.rounding_step.item() == 4
    assert not same_bits(updater_tensors(captured)[:len(rows)], after_warm_up[:len(rows)])
    assert same_bits(updater_tensors(captured), updater_tensors(eager))


# ---- 9. the torch ops -----------------------------------------------------------------------------------------------------------
def test_torch_op_update_with_seeds(ce):
    from cuembed_amd import cuembed_pyt
    rows, width, dtype = GROUPS[0], 36, torch.bfloat16
    seeds = seeds_for(rows)
    a, b = Side(rows, width, dtype, "adagrad"), Side(rows, width, dtype, "adagrad")
    ids = torch.tensor(entries_of(rows, "skip_middle") + [-1, -1], dtype=torch.int64, device=DEV)
    grads = placed(0.25 * hashed(ids.numel() * width, 9), (ids.numel(), width), dtype)
    last = torch.tensor([ids.numel() - 3], dtype=torch.int64, device=DEV)
    kw = dict(rule="adagrad", lr=LR, eps=EPS, last_id=last, stochastic_rounding=True, seeds=seeds, step=STEP)
    group_a = ce.TableGroup(a.tables)
    cuembed_pyt.cuembed_sparse_row_update_grouped(group_a, ids, grads, states=a.states[0], **kw)
    ce.sparse_row_update_grouped(ce.TableGroup(b.tables), ids, grads, states=b.states[0], **kw)
    torch.cuda.synchronize()
    assert same_bits(a.tensors(), b.tensors())
    assert not same_bits(a.tables, Side(rows, width, dtype, "adagrad").tables)
    with pytest.raises(RuntimeError, match="seeds"):           # seeds without the rounding: the op says so
        cuembed_pyt.cuembed_sparse_row_update_grouped(group_a, ids, grads, rule="sgd", lr=LR, seeds=seeds)
    # the schema, the fake kernel and the real kernel agree on the new argument forms
    from cuembed_amd import grouped_backward as gb
    seeds_device = gb._seeds_tensor(group_a, tuple(seeds))
    assert seeds_device.dtype == torch.int64 and seeds_device[0].item() == seeds[0] - 2 ** 64
    step_word = torch.tensor([STEP], dtype=torch.int64, device=DEV)
    op = torch.ops.cuembed_pyt.cuembed_sparse_row_update_grouped
    front = (list(a.tables), group_a.table_ptrs, list(a.states[0]), gb._state_ptrs(group_a, a.states[0])[1],
             group_a.row_base_device, ids, grads, "adagrad", LR, EPS, None, -1, None, last, True, seeds_device)
    for tail in ((STEP, None), (0, step_word)):
        torch.library.opcheck(op, front + tail, test_utils=["test_schema", "test_faketensor"])


def test_torch_op_adam_with_seeds(ce):
    from cuembed_amd import cuembed_pyt
    from cuembed_amd import grouped_backward as gb
    rows, width, dtype = GROUPS[1], 8, torch.float16
    seeds = seeds_for(rows)
    a, b = Side(rows, width, dtype, "rowwise_adam"), Side(rows, width, dtype, "rowwise_adam")
    ids = torch.tensor(entries_of(rows, "all"), dtype=torch.int32, device=DEV)
    grads = placed(0.25 * hashed(ids.numel() * width, 11), (ids.numel(), width), dtype)
    bias = torch.tensor([0.7316], dtype=torch.float32, device=DEV)
    step_word = torch.tensor([STEP], dtype=torch.int64, device=DEV)
    kw = dict(lr=LR, bias_factor=bias, betas=BETAS, eps=EPS, weight_decay=0.0125, rowwise=True, count=ids.numel() - 2,
              stochastic_rounding=True, seeds=seeds, step=step_word)
    group_a = ce.TableGroup(a.tables)
    cuembed_pyt.cuembed_sparse_row_adam_grouped(group_a, ids, grads, exp_avg=a.states[0], exp_avg_sq=a.states[1], **kw)
    ce.sparse_row_adam_grouped(ce.TableGroup(b.tables), ids, grads, exp_avg=b.states[0], exp_avg_sq=b.states[1], **kw)
    torch.cuda.synchronize()
    assert same_bits(a.tensors(), b.tensors())
    assert not same_bits(a.tables, Side(rows, width, dtype, "rowwise_adam").tables)
    with pytest.raises(RuntimeError, match="stochastic rounding"):
        cuembed_pyt.cuembed_sparse_row_adam_grouped(group_a, ids, grads, exp_avg=a.states[0], exp_avg_sq=a.states[1],
                                                    lr=LR, stochastic_rounding=True)
    op = torch.ops.cuembed_pyt.cuembed_sparse_row_adam_grouped
    args = (list(a.tables), group_a.table_ptrs, list(a.states[0]), gb._state_ptrs(group_a, a.states[0])[1],
            list(a.states[1]), gb._state_ptrs(group_a, a.states[1])[1], group_a.row_base_device, ids, grads, True, LR, 1.0,
            BETAS[0], BETAS[1], EPS, 0.0125, None, bias, ids.numel() - 2, None, None, True,
            gb._seeds_tensor(group_a, tuple(seeds)), 0, step_word)
    torch.library.opcheck(op, args, test_utils=["test_schema", "test_faketensor"])
