"""The optimizer step on a group of SEPARATE table tensors in one launch (sparse_row_update_grouped,
sparse_row_adam_grouped, GroupSparseUpdater, GroupSparseAdamUpdater, the two torch ops) against the project's own
single-table step: num_tables calls of sparse_row_update / sparse_row_adam on clones, fed the entries of
GroupedGrad.per_table().  Tables and every state tensor are compared BIT FOR BIT, on hashed (arbitrary) data.

Why bit for bit holds for every rule: a row's arithmetic depends on nothing but that row, and the one thing that has an
order -- the row-wise rules' sum of g^2 -- is summed in an order fixed by the width and the LANE width alone
(tests/optimizer_bits_reference.py: row_sums; sparse_update.hpp: PlanUpdate takes the entry count for the grid only).
The grouped step picks ONE lane width for the group, from its least aligned table, so the oracle's clones are given
the alignment that makes the single-table call pick the same one: all 16-byte aligned, or all 4 bytes off.

The shapes are the smallest at which resolving an entry's table can go wrong: row counts (1, 5, 70) and (3, 1, 1, 64, 2),
so that with every row named each table boundary falls inside one wavefront's entries."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
GROUPS = ((1, 5, 70), (3, 1, 1, 64, 2))
SHAPES = ((torch.float32, 4), (torch.float16, 8), (torch.bfloat16, 36), (torch.float16, 128), (torch.float32, 128))
PLAIN = dict(weight_decay=0.0, bias_factor=1.0)
TUNED = dict(weight_decay=0.0125, bias_factor=0.7316)
RULES = (("sgd", {}), ("adagrad", {}), ("rowwise_adagrad", {}), ("adam", PLAIN), ("adam", TUNED), ("rowwise_adam", PLAIN),
         ("rowwise_adam", TUNED))
FIVE = (("sgd", {}), ("adagrad", {}), ("rowwise_adagrad", {}), ("adam", TUNED), ("rowwise_adam", TUNED))
LR, EPS, BETAS = 0.0371, 1e-3, (0.9, 0.98)


def rule_id(r):
    return r[0] + ("_wd_bias" if r[1].get("weight_decay") else "")


@pytest.fixture(scope="module")
def ce():
    import cuembed_amd
    return cuembed_amd


def hashed_ints(n, salt):
    """n arbitrary 24-bit values (CPU int64), a pure function of (position, salt)."""
    i = torch.arange(n, dtype=torch.int64)
    h = ((i + 1) * 2654435761 ^ (salt + 1) * 0x9E3779B9) & 0xFFFFFFFF
    h = h ^ (h >> 15)
    h = (h * 0x85EBCA6B) & 0xFFFFFFFF
    h = h ^ (h >> 13)
    h = (h * 0xC2B2AE35) & 0xFFFFFFFF
    h = h ^ (h >> 16)
    return h >> 8


def hashed(n, salt, positive=False):
    """Arbitrary values in [-0.5, 0.5) (or [0, 1)): not exactly representable in the 16-bit types, nor are their products."""
    return hashed_ints(n, salt).double() / 16777216.0 - (0.0 if positive else 0.5)


def placed(values, shape, dtype, misaligned=False):
    """The values as a contiguous device tensor that starts on a 16-byte boundary, or (misaligned) 4 bytes past one."""
    n = values.numel()
    if misaligned:
        pad = 4 // torch.empty((), dtype=dtype).element_size()
        t = torch.empty(n + pad + 8, dtype=dtype, device=DEV)[pad:pad + n].view(shape)
    else:
        t = torch.empty(shape, dtype=dtype, device=DEV)
    t.copy_(values.to(dtype).view(shape))
    assert t.is_contiguous() and t.data_ptr() % 16 == (4 if misaligned else 0)
    return t


def ibits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def same_bits(a, b):
    return all(torch.equal(ibits(x), ibits(y)) for x, y in zip(a, b))


def state_shapes(rule, rows, width):
    """The shapes of the rule's state tensors, per table: a list (one entry per state tensor) of lists."""
    full, word = [(n, width) for n in rows], [(n,) for n in rows]
    return {"sgd": [], "adagrad": [full], "rowwise_adagrad": [word], "adam": [full, full],
            "rowwise_adam": [full, word]}[rule]


class Side:
    """The tables and state tensors of one side of a comparison.  misaligned: the set of table numbers that sit 4 bytes
    off a 16-byte boundary (their per-element state stays aligned: torch owns that alignment)."""

    def __init__(self, rows, width, dtype, rule, misaligned=(), salt=0):
        self.tables = [placed(hashed(n * width, salt + t), (n, width), dtype, t in misaligned) for t, n in enumerate(rows)]
        self.states = [[placed(hashed(torch.Size(s).numel(), salt + 100 * (k + 1) + t, positive=True), s, torch.float32)
                        for t, s in enumerate(shapes)] for k, shapes in enumerate(state_shapes(rule, rows, width))]

    def tensors(self):
        return self.tables + [s for plane in self.states for s in plane]

    def clones(self):
        return [t.clone() for t in self.tensors()]


def grouped_step(ce, group, side, rule, opts, ids, rows, **count):
    if rule in ("adam", "rowwise_adam"):
        ce.sparse_row_adam_grouped(group, ids, rows, exp_avg=side.states[0], exp_avg_sq=side.states[1], lr=LR, betas=BETAS,
                                   eps=EPS, rowwise=rule == "rowwise_adam", **opts, **count)
    else:
        ce.sparse_row_update_grouped(group, ids, rows, rule=rule, lr=LR, eps=EPS, states=side.states[0] if side.states else None,
                                     **count)


def per_table_steps(ce, group, side, rule, opts, ids, rows, valid, bias_factor=None):
    """The oracle: the entries of GroupedGrad.per_table() (one read-back of the cuts), one single-table call per table."""
    last = torch.tensor([valid - 1], dtype=ids.dtype, device=DEV)
    grad = ce.GroupedGrad(ids, rows, last, group.row_base, group.row_base_device)
    per_table = grad.per_table()
    assert sum(i.numel() for i, _ in per_table) == valid
    for t, (local_ids, local_rows) in enumerate(per_table):
        if rule in ("adam", "rowwise_adam"):
            kw = dict(opts)
            if bias_factor is not None:
                kw["bias_factor"] = bias_factor
            ce.sparse_row_adam(side.tables[t], local_ids, local_rows, exp_avg=side.states[0][t], exp_avg_sq=side.states[1][t],
                               lr=LR, betas=BETAS, eps=EPS, rowwise=rule == "rowwise_adam", **kw)
        else:
            ce.sparse_row_update(side.tables[t], local_ids, local_rows, rule=rule, lr=LR, eps=EPS,
                                 state=side.states[0][t] if side.states else None)


def entries_of(rows, coverage):
    """Ascending global rows of the tables laid end to end."""
    base = [0]
    for n in rows:
        base.append(base[-1] + n)
    T = len(rows)
    if coverage == "all":
        return list(range(base[-1]))
    if coverage == "first":
        return list(range(base[0], base[1]))
    if coverage == "last":
        return list(range(base[T - 1], base[T]))
    if coverage == "skip_middle":
        mid = T // 2
        return [r for r in range(base[-1]) if not base[mid] <= r < base[mid + 1]]
    if coverage == "one":
        return [base[1]]
    if coverage == "last_rows":      # the last row of every table: the row just below each boundary
        return [base[t + 1] - 1 for t in range(T)]
    raise ValueError(coverage)


def check_untouched(rows, width, side, before, named):
    """Rows that no valid entry names keep their bits, in the table and in every state tensor: all of them."""
    base, per_table = 0, []
    for n in rows:
        keep = torch.ones(n, dtype=torch.bool)
        for r in named:
            if base <= r < base + n:
                keep[r - base] = False
        per_table.append(keep.to(DEV))
        base += n
    T = len(rows)
    for k, (now, was) in enumerate(zip(side.tensors(), before)):
        keep = per_table[k % T]
        assert torch.equal(ibits(now)[keep], ibits(was)[keep]), "tensor %d: a row that no entry names changed" % k


def compare(ce, rows, width, dtype, rule, opts, coverage="all", index=torch.int32, count_kind="all", misaligned=(),
            oracle_misaligned=None, steps=2, flat=False):
    """`steps` consecutive grouped steps against the per-table oracle; returns the grouped side."""
    total = sum(rows)
    named = entries_of(rows, coverage)
    if flat:
        mine = Side(rows, width, dtype, rule)
        storage = torch.cat(mine.tables)
        group = ce.TableGroup.from_flat(storage, rows)
        mine.tables = list(group.tables)
    else:
        mine = Side(rows, width, dtype, rule, misaligned)
        group = ce.TableGroup(mine.tables)
    if oracle_misaligned is None:      # the oracle runs at the group's lane width: all tables off, or none
        oracle_misaligned = range(len(rows)) if misaligned else ()
    theirs = Side(rows, width, dtype, rule, oracle_misaligned)
    assert same_bits(mine.tensors(), theirs.tensors())
    their_group = ce.TableGroup(theirs.tables)
    for step in range(steps):
        valid = len(named)
        tail = {"all": 0, "zero": 0, "short_minus_one": 5, "short_past_total": 5}.get(count_kind, 3)
        fill = total + 5 if count_kind == "short_past_total" else -1
        ids = torch.tensor(named + [fill] * tail, dtype=index, device=DEV)
        grads = placed(0.25 * hashed((valid + tail) * width, 1000 + step), (valid + tail, width), dtype)
        if count_kind == "zero":
            valid, named_now = 0, []
        else:
            named_now = named
        count = {"all": {}, "host": dict(count=valid), "zero": dict(count=0),
                 "word32": dict(count=torch.tensor([valid], dtype=torch.int32, device=DEV)),
                 "word64": dict(count=torch.tensor([valid], dtype=torch.int64, device=DEV)),
                 "last_id": dict(last_id=torch.tensor([valid - 1], dtype=index, device=DEV)),
                 "short_minus_one": dict(last_id=torch.tensor([valid - 1], dtype=index, device=DEV)),
                 "short_past_total": dict(count=torch.tensor([valid], dtype=torch.int32, device=DEV))}[count_kind]
        before = mine.clones()
        grouped_step(ce, group, mine, rule, opts, ids, grads, **count)
        per_table_steps(ce, their_group, theirs, rule, opts, ids, grads, valid)
        torch.cuda.synchronize()
        assert same_bits(mine.tensors(), theirs.tensors()), "step %d differs from the per-table calls" % step
        check_untouched(rows, width, mine, before, named_now)
        if named_now:
            assert not same_bits(mine.tables, before[:len(rows)]), "the step changed nothing"
    return mine


@pytest.mark.parametrize("rule", RULES, ids=rule_id)
@pytest.mark.parametrize("dtype, width", SHAPES, ids=lambda v: str(v).replace("torch.", ""))
@pytest.mark.parametrize("rows", GROUPS, ids=lambda r: "x".join(map(str, r)))
def test_every_rule_on_every_row_of_every_table(ce, rows, dtype, width, rule):
    """Every row named, two consecutive steps (the second reads the state the first wrote); int64 ids for the widths
    of one full lane per row."""
    compare(ce, rows, width, dtype, rule[0], rule[1], index=torch.int64 if width in (8, 128) else torch.int32)


@pytest.mark.parametrize("rule", FIVE, ids=rule_id)
@pytest.mark.parametrize("coverage", ["first", "last", "skip_middle", "one", "last_rows"])
@pytest.mark.parametrize("rows", GROUPS, ids=lambda r: "x".join(map(str, r)))
def test_entry_coverage(ce, rows, coverage, rule):
    """Only the first table, only the last, a middle table without an entry, one entry in all, the row below each
    boundary."""
    compare(ce, rows, 8, torch.float16, rule[0], rule[1], coverage=coverage,
            index=torch.int64 if coverage in ("last", "one") else torch.int32)


@pytest.mark.parametrize("rule", (FIVE[0], FIVE[2], FIVE[3]), ids=rule_id)
@pytest.mark.parametrize("index", [torch.int32, torch.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("count_kind", ["host", "word32", "word64", "last_id", "zero", "short_minus_one", "short_past_total"])
def test_count_sources(ce, count_kind, index, rule):
    """A host int, a device word of either dtype, last_id, count=0, and a count below the array's size whose tail holds
    -1 or total_rows + 5: entries past the count are never looked at."""
    compare(ce, GROUPS[0], 4, torch.float32, rule[0], rule[1], coverage="skip_middle", index=index, count_kind=count_kind)


def test_a_count_outside_the_array_applies_nothing(ce):
    rows, width = GROUPS[0], 4
    for rule, opts in (FIVE[1], FIVE[4]):
        side = Side(rows, width, torch.float32, rule)
        group = ce.TableGroup(side.tables)
        ids = torch.arange(sum(rows), dtype=torch.int32, device=DEV)
        grads = placed(hashed(ids.numel() * width, 7), (ids.numel(), width), torch.float32)
        before = side.clones()
        for word in (-1, -5, ids.numel() + 1):
            grouped_step(ce, group, side, rule, opts, ids, grads, count=torch.tensor([word], dtype=torch.int64, device=DEV))
            grouped_step(ce, group, side, rule, opts, ids, grads, last_id=torch.tensor([word - 1], dtype=torch.int32, device=DEV))
        torch.cuda.synchronize()
        assert same_bits(side.tensors(), before)


@pytest.mark.parametrize("rule", FIVE, ids=rule_id)
@pytest.mark.parametrize("dtype, width", SHAPES[:4], ids=lambda v: str(v).replace("torch.", ""))
@pytest.mark.parametrize("misaligned", [(1,), ()], ids=["one_table_4_bytes_off", "aligned"])
def test_alignment(ce, misaligned, dtype, width, rule):
    """One table of the group is a view 4 bytes off a 16-byte boundary: the whole group narrows to 4-byte lanes (the
    oracle's clones are all put 4 bytes off, so that every single-table call runs at that width); and the same group
    with all tables aligned."""
    group = ce.TableGroup(Side(GROUPS[0], width, dtype, "sgd", misaligned).tables)
    assert group.lane_bytes() == (4 if misaligned else (8 if width == 36 else 16))
    compare(ce, GROUPS[0], width, dtype, rule[0], rule[1], misaligned=misaligned)


@pytest.mark.parametrize("rule", FIVE, ids=rule_id)
@pytest.mark.parametrize("width, misaligned, slices", [(260, (), 4), (1028, (), 0), (128, (3,), 4)])
def test_rows_wider_than_a_lane_group(ce, width, misaligned, slices, rule):
    """The walk's other two bodies: four slices per lane (65 lanes of 16 bytes; 128 lanes of 4 bytes) and the run-time
    loop over the slices (257 lanes)."""
    lane = 4 if misaligned else 16
    shape = ce.sparse_row_update_launch_shape(torch.float32, width, 71)
    assert shape["slices_per_lane"] == slices or misaligned
    assert (width * 4 // lane > 64) and ((width * 4 // lane > 256) == (slices == 0))
    compare(ce, GROUPS[1], width, torch.float32, rule[0], rule[1], misaligned=misaligned, steps=1)


@pytest.mark.parametrize("rule", FIVE, ids=rule_id)
@pytest.mark.parametrize("dtype, width", [SHAPES[0], SHAPES[2]], ids=lambda v: str(v).replace("torch.", ""))
def test_one_storage_and_separate_tensors_give_the_same_bits(ce, dtype, width, rule):
    """The same data as row slices of ONE tensor (TableGroup.from_flat) and as separate tensors."""
    flat = compare(ce, GROUPS[1], width, dtype, rule[0], rule[1], flat=True, oracle_misaligned=())
    separate = compare(ce, GROUPS[1], width, dtype, rule[0], rule[1])
    assert same_bits(flat.tensors(), separate.tensors())


# ---- the updaters ---------------------------------------------------------------------------------------------------
def lookups(rows, batch, csr, salt=0):
    """(idx, offsets) of a group's bags: CSR with bags of 0 to 3 lookups, or fixed hotness 2."""
    T = len(rows)
    if not csr:
        idx = torch.stack([(hashed_ints(batch * 2, salt + t) % n).view(batch, 2) for t, n in enumerate(rows)])
        return idx.to(torch.int32).to(DEV), None
    lengths = (hashed_ints(T * batch, salt + 50) % 4).tolist()
    ids, offsets = [], [0]
    for g, n in enumerate(lengths):
        ids += (hashed_ints(n, salt + 60 + g) % rows[g // batch]).tolist()
        offsets.append(offsets[-1] + n)
    return torch.tensor(ids, dtype=torch.int32, device=DEV), torch.tensor(offsets, dtype=torch.int32, device=DEV)


def updater_for(optim, group, rule, opts):
    if rule in ("adam", "rowwise_adam"):
        return optim.GroupSparseAdamUpdater(group, LR, betas=BETAS, eps=EPS, weight_decay=opts["weight_decay"],
                                            rowwise=rule == "rowwise_adam", bias_correction=opts["bias_factor"] != 1.0)
    return optim.GroupSparseUpdater(group, rule, LR, eps=EPS, initial_accumulator_value=0.125)


def updater_tensors(u):
    if hasattr(u, "exp_avg"):
        return list(u.group.tables) + list(u.exp_avg) + list(u.exp_avg_sq)
    return list(u.group.tables) + list(u.states or ())


@pytest.mark.parametrize("rule", FIVE + (("adam", PLAIN),), ids=rule_id)
@pytest.mark.parametrize("mode", ["sum", "mean"])
@pytest.mark.parametrize("csr", [True, False], ids=["csr", "fixed"])
def test_backward_and_apply_is_the_per_table_chain(ce, csr, mode, rule):
    """GroupSparseUpdater / GroupSparseAdamUpdater.backward_and_apply: the grouped backward in its compressed form and
    ONE step, against the same gradient cut per table (one read-back) and applied by num_tables single-table calls."""
    from cuembed_amd import optim
    rows, width, dtype, batch = GROUPS[1], 8, torch.float16, 5
    rule, opts = rule
    mine = Side(rows, width, dtype, "sgd")
    theirs = Side(rows, width, dtype, "sgd")
    group = ce.TableGroup(mine.tables)
    u = updater_for(optim, group, rule, opts)
    before = [t.clone() for t in updater_tensors(u)]
    idx, offsets = lookups(rows, batch, csr)
    grad_y = placed(hashed(batch * len(rows) * width, 77), (batch, len(rows), width), dtype)
    grad = u.backward_and_apply(grad_y, idx, offsets, mode=mode)
    torch.cuda.synchronize()
    # the oracle starts from the updater's initial state and applies the SAME compressed gradient table by table
    T = len(rows)
    theirs.states = [before[T * (k + 1):T * (k + 2)] for k in range((len(before) - T) // T)]
    bias = u.bias_factor.clone() if hasattr(u, "bias_factor") and opts["bias_factor"] != 1.0 else None
    kw = dict(opts, bias_factor=1.0) if opts else {}
    valid = int(grad.last_id.item()) + 1
    assert 0 < valid <= grad.capacity
    per_table_steps(ce, ce.TableGroup(theirs.tables), theirs, rule, kw, grad.ids, grad.rows, valid, bias_factor=bias)
    torch.cuda.synchronize()
    assert same_bits(updater_tensors(u), theirs.tensors())
    assert not same_bits(u.group.tables, before[:T])
    if hasattr(u, "powers"):
        assert u.powers[0].item() == 1.0     # (the clock counts with bias_correction=False too; its factor is not used)
        assert u.bias_factor.item() == pytest.approx(ce.adam_bias_factor(1, BETAS), rel=1e-6)


@pytest.mark.parametrize("rule", FIVE, ids=rule_id)
def test_a_captured_step_on_separate_tensors_replays_like_eager_steps(ce, rule):
    """forward + backward_and_apply on a group of SEPARATE tensors captured in a HIP graph: no read-back anywhere, or the
    capture would fail.  One eager warm-up step and three replays equal four eager steps, bit for bit -- for Adam that
    needs the bias-factor clock to advance on the device at every replay.  (grad_y holds multiples of 1/8, so the
    backward's sums are exact whatever their association; tables, learning rate and state are arbitrary.)"""
    from cuembed_amd import optim
    rows, width, dtype, batch = GROUPS[1], 8, torch.float32, 6
    rule, opts = rule
    idx, offsets = lookups(rows, batch, True, salt=3)
    grad_y = placed(((hashed_ints(batch * len(rows) * width, 5) % 33) - 16).double() / 8.0, (batch, len(rows), width), dtype)

    def fresh():
        return updater_for(optim, ce.TableGroup(Side(rows, width, dtype, "sgd").tables), rule, opts)

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
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    for _ in range(4):
        step(eager)
    torch.cuda.synchronize()
    assert not same_bits(updater_tensors(captured)[:len(rows)], after_warm_up[:len(rows)])
    assert same_bits(updater_tensors(captured), updater_tensors(eager))
    if hasattr(eager, "powers"):
        assert captured.powers[0].item() == 4.0 and torch.equal(captured.powers, eager.powers)
        assert torch.equal(ibits(captured.bias_factor), ibits(eager.bias_factor))


# ---- the torch ops --------------------------------------------------------------------------------------------------
def test_torch_op_update(ce):
    from cuembed_amd import cuembed_pyt
    rows, width, dtype = GROUPS[0], 36, torch.bfloat16
    a, b = Side(rows, width, dtype, "adagrad"), Side(rows, width, dtype, "adagrad")
    ids = torch.tensor(entries_of(rows, "skip_middle") + [-1, -1], dtype=torch.int64, device=DEV)
    grads = placed(hashed(ids.numel() * width, 9), (ids.numel(), width), dtype)
    last = torch.tensor([ids.numel() - 3], dtype=torch.int64, device=DEV)
    cuembed_pyt.cuembed_sparse_row_update_grouped(ce.TableGroup(a.tables), ids, grads, rule="adagrad", lr=LR,
                                                  states=a.states[0], eps=EPS, last_id=last)
    ce.sparse_row_update_grouped(ce.TableGroup(b.tables), ids, grads, rule="adagrad", lr=LR, states=b.states[0], eps=EPS,
                                 last_id=last)
    torch.cuda.synchronize()
    assert same_bits(a.tensors(), b.tensors())
    assert not same_bits(a.tables, Side(rows, width, dtype, "adagrad").tables)
    with pytest.raises(RuntimeError, match="stochastic rounding"):
        cuembed_pyt.cuembed_sparse_row_update_grouped(ce.TableGroup(a.tables), ids, grads, rule="sgd", lr=LR,
                                                      stochastic_rounding=True)


def test_torch_op_adam(ce):
    from cuembed_amd import cuembed_pyt
    rows, width, dtype = GROUPS[1], 8, torch.float16
    a, b = Side(rows, width, dtype, "rowwise_adam"), Side(rows, width, dtype, "rowwise_adam")
    ids = torch.tensor(entries_of(rows, "all"), dtype=torch.int32, device=DEV)
    grads = placed(hashed(ids.numel() * width, 11), (ids.numel(), width), dtype)
    bias = torch.tensor([0.7316], dtype=torch.float32, device=DEV)
    kw = dict(lr=LR, bias_factor=bias, betas=BETAS, eps=EPS, weight_decay=0.0125, rowwise=True, count=ids.numel() - 2)
    cuembed_pyt.cuembed_sparse_row_adam_grouped(ce.TableGroup(a.tables), ids, grads, exp_avg=a.states[0],
                                                exp_avg_sq=a.states[1], **kw)
    ce.sparse_row_adam_grouped(ce.TableGroup(b.tables), ids, grads, exp_avg=b.states[0], exp_avg_sq=b.states[1], **kw)
    torch.cuda.synchronize()
    assert same_bits(a.tensors(), b.tensors())
    assert not same_bits(a.tables, Side(rows, width, dtype, "rowwise_adam").tables)
