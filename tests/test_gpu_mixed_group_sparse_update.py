"""The optimizer step on a group of tables of DIFFERENT widths in one launch (sparse_row_update_mixed_group,
sparse_row_adam_mixed_group, MixedGroupSparseUpdater, MixedGroupSparseAdamUpdater) against the project's independent fp32
step model, tests/optimizer_bits_reference.py: `step` once per table, at that table's width and the group's lane width.
Tables and every state tensor are compared BIT FOR BIT, on hashed (non-representable) data.

The groups are the smallest at which the walk can go wrong: row counts (1, 5, 70) with widths (8, 128, 16), so that with
every row named each cut falls inside one 64-entry tile; row counts (3, 1, 1, 64, 2) with a row wider than 64 lanes, one-lane
rows and partial passes in one tile; a float32 counterpart with a 260-wide table; a bfloat16 one whose narrowest row is 4
bytes, which forces 4-byte lanes.  Every rows[k, W_t:] is NaN before the call, and the entries past the count are
poisoned (id -1, NaN rows): any read of either shows in the bits."""
import numpy as np
import pytest
import torch

import optimizer_bits_reference as R
from test_gpu_grouped_sparse_update import hashed, hashed_ints, ibits, lookups, placed, same_bits

pytestmark = pytest.mark.gpu

DEV = "cuda"
KIND = {torch.float32: "f32", torch.float16: "f16", torch.bfloat16: "bf16"}
GROUPS = {"f16_cuts": (torch.float16, (1, 5, 70), (8, 128, 16)),
          "f16_wide": (torch.float16, (3, 1, 1, 64, 2), (16, 8, 520, 8, 32)),
          "f32_wide": (torch.float32, (3, 1, 1, 64, 2), (8, 4, 260, 4, 16)),
          "bf16_4_byte_lanes": (torch.bfloat16, (1, 5, 70), (2, 130, 38))}
LANE = {"f16_cuts": 16, "f16_wide": 16, "f32_wide": 16, "bf16_4_byte_lanes": 4}
PLAIN = dict(weight_decay=0.0, bias_factor=1.0)
TUNED = dict(weight_decay=0.0125, bias_factor=0.7316)
RULES = (("sgd", {}), ("adagrad", {}), ("rowwise_adagrad", {}), ("adam", PLAIN), ("adam", TUNED), ("rowwise_adam", PLAIN),
         ("rowwise_adam", TUNED))
FIVE = (RULES[0], RULES[1], RULES[2], RULES[4], RULES[6])
LR, EPS, BETAS = 0.0371, 1e-3, (0.9, 0.98)
TAIL = 3          # poisoned entries behind the valid ones


def rule_id(r):
    return r[0] + ("_wd_bias" if r[1].get("weight_decay") else "")


@pytest.fixture(scope="module")
def ce():
    import cuembed_amd
    return cuembed_amd


def patterns(t):
    """A tensor's bit patterns as the model takes them (uint16 / uint32 numpy)."""
    raw = ibits(t.detach().cpu().contiguous()).numpy()
    return raw.view(np.uint16 if raw.dtype == np.int16 else np.uint32)


def state_shapes(rule, rows, widths):
    full, word = [(n, w) for n, w in zip(rows, widths)], [(n,) for n in rows]
    return {"sgd": [], "adagrad": [full], "rowwise_adagrad": [word], "adam": [full, full], "rowwise_adam": [full, word]}[rule]


class Side:
    """The tables and state tensors of a mixed-width group (misaligned: every table 4 bytes off a 16-byte boundary)."""

    def __init__(self, dtype, rows, widths, rule, misaligned=False):
        self.tables = [placed(hashed(n * w, t), (n, w), dtype, misaligned) for t, (n, w) in enumerate(zip(rows, widths))]
        self.states = [[placed(hashed(torch.Size(s).numel(), 100 * (k + 1) + t, positive=True), s, torch.float32)
                        for t, s in enumerate(shapes)] for k, shapes in enumerate(state_shapes(rule, rows, widths))]

    def tensors(self):
        return self.tables + [s for plane in self.states for s in plane]


def named_rows(rows, subset):
    """Ascending global rows of the tables laid end to end."""
    base = np.concatenate([[0], np.cumsum(rows)])
    every = list(range(int(base[-1])))
    if subset == "all":
        return every
    if subset == "every_other":
        return every[::2]
    if subset == "one_table_empty":
        mid = len(rows) // 2
        return [r for r in every if not base[mid] <= r < base[mid + 1]]
    assert subset == "empty"
    return []


def gradient(dtype, rows, widths, named, index, salt):
    """(ids, rows) as embedding_backward_mixed_group leaves them, made hostile: NaN in every padded column, and TAIL
    entries behind the valid ones with id -1 and NaN rows."""
    w_max, n = max(widths), len(named) + TAIL
    grads = (0.25 * hashed(n * w_max, 1000 + salt)).view(n, w_max).clone()
    base = np.concatenate([[0], np.cumsum(rows)])
    for k, r in enumerate(named):
        grads[k, widths[int(np.searchsorted(base, r, side="right")) - 1]:] = float("nan")
    grads[len(named):] = float("nan")
    ids = torch.tensor(list(named) + [-1] * TAIL, dtype=index, device=DEV)
    return ids, placed(grads, (n, w_max), dtype)


def step(ce, group, side, rule, opts, ids, grads, **count):
    if rule in ("adam", "rowwise_adam"):
        ce.sparse_row_adam_mixed_group(group, ids, grads, exp_avg=side.states[0], exp_avg_sq=side.states[1], lr=LR,
                                       betas=BETAS, eps=EPS, rowwise=rule == "rowwise_adam", **opts, **count)
    else:
        ce.sparse_row_update_mixed_group(group, ids, grads, rule=rule, lr=LR, eps=EPS,
                                         states=side.states[0] if side.states else None, **count)


def model(dtype, rows, widths, rule, opts, before, ids, grads, valid, lane):
    """The oracle: optimizer_bits_reference.step once per table on the bit patterns `before` (Side.tensors() order), at the
    table's width and the group's lane width.  Returns the expected patterns in the same order."""
    kind, T = KIND[dtype], len(rows)
    base = np.concatenate([[0], np.cumsum(rows)])
    all_ids = ids.cpu().numpy().astype(np.int64)[:valid]
    g = patterns(grads)
    tables, planes = [], [[] for _ in range((len(before) - T) // T)]
    for t in range(T):
        mine = np.nonzero((all_ids >= base[t]) & (all_ids < base[t + 1]))[0]
        state = [before[T * (k + 1) + t] for k in range(len(planes))]
        table, state, _ = R.step(rule, kind, before[t], state, all_ids - base[t], g[:valid, :widths[t]], mine, lr=LR, eps=EPS,
                                 betas=BETAS, lane=lane, **opts)
        tables.append(table)
        for k, s in enumerate(state):
            planes[k].append(s)
    return tables + [s for plane in planes for s in plane]


def check(ce, name, rule, opts, subset="all", index=torch.int32, count_kind="last_id", steps=1):
    dtype, rows, widths = GROUPS[name]
    assert min(R.lane_bytes(KIND[dtype], w) for w in widths) == LANE[name]
    side = Side(dtype, rows, widths, rule)
    group = ce.MixedTableGroup(side.tables)
    named = named_rows(rows, subset)
    for s in range(steps):
        ids, grads = gradient(dtype, rows, widths, named, index, s)
        valid = len(named)
        count = {"host": dict(count=valid), "word32": dict(count=torch.tensor([valid], dtype=torch.int32, device=DEV)),
                 "word64": dict(count=torch.tensor([valid], dtype=torch.int64, device=DEV)),
                 "last_id": dict(last_id=torch.tensor([valid - 1], dtype=index, device=DEV))}[count_kind]
        before = [patterns(t) for t in side.tensors()]
        want = model(dtype, rows, widths, rule, opts, before, ids, grads, valid, LANE[name])
        step(ce, group, side, rule, opts, ids, grads, **count)
        torch.cuda.synchronize()
        for k, (now, expected) in enumerate(zip(side.tensors(), want)):
            assert np.array_equal(patterns(now), expected), "step %d, tensor %d differs from the model" % (s, k)
        if named:
            assert not np.array_equal(patterns(side.tables[0]), before[0]), "the step changed nothing"


@pytest.mark.parametrize("rule", RULES, ids=rule_id)
@pytest.mark.parametrize("name", list(GROUPS))
def test_every_rule_on_every_row_of_every_table(ce, name, rule):
    """Every row named, two consecutive steps (the second reads the state the first wrote); int64 ids on two groups."""
    check(ce, name, rule[0], rule[1], index=torch.int64 if name in ("f16_wide", "bf16_4_byte_lanes") else torch.int32, steps=2)


@pytest.mark.parametrize("rule", FIVE, ids=rule_id)
@pytest.mark.parametrize("subset", ["every_other", "one_table_empty", "empty"])
def test_named_subsets(ce, subset, rule):
    """Every other row, one table without an entry, an empty gradient (only poisoned entries)."""
    check(ce, "f16_wide", rule[0], rule[1], subset=subset, count_kind="host" if subset == "empty" else "last_id")


@pytest.mark.parametrize("rule", (FIVE[0], FIVE[2], FIVE[3]), ids=rule_id)
@pytest.mark.parametrize("index", [torch.int32, torch.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("count_kind", ["host", "word32", "word64", "last_id"])
def test_count_sources(ce, count_kind, index, rule):
    check(ce, "f16_cuts", rule[0], rule[1], subset="every_other", index=index, count_kind=count_kind)


@pytest.mark.parametrize("rule", (FIVE[1], FIVE[4]), ids=rule_id)
def test_a_count_outside_the_array_applies_nothing(ce, rule):
    dtype, rows, widths = GROUPS["f16_cuts"]
    side = Side(dtype, rows, widths, rule[0])
    group = ce.MixedTableGroup(side.tables)
    ids, grads = gradient(dtype, rows, widths, named_rows(rows, "all"), torch.int32, 7)
    before = [t.clone() for t in side.tensors()]
    for word in (-1, ids.numel() + 1):
        step(ce, group, side, rule[0], rule[1], ids, grads, count=torch.tensor([word], dtype=torch.int64, device=DEV))
        step(ce, group, side, rule[0], rule[1], ids, grads, last_id=torch.tensor([word - 1], dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    assert same_bits(side.tensors(), before)


@pytest.mark.parametrize("rule", FIVE, ids=rule_id)
@pytest.mark.parametrize("misaligned", [False, True], ids=["aligned", "all_4_bytes_off"])
def test_the_bits_of_single_table_calls(ce, misaligned, rule):
    """Widths that are all multiples of 16 bytes: bit for bit the num_tables real sparse_row_update / sparse_row_adam calls
    fed per_table(), on aligned tensors (16-byte lanes everywhere) and with every table 4 bytes off (4-byte lanes)."""
    dtype, rows, widths = GROUPS["f16_cuts"]
    rule, opts = rule
    mine, theirs = Side(dtype, rows, widths, rule, misaligned), Side(dtype, rows, widths, rule, misaligned)
    group = ce.MixedTableGroup(mine.tables)
    named = named_rows(rows, "all")
    ids, grads = gradient(dtype, rows, widths, named, torch.int32, 3)
    last = torch.tensor([len(named) - 1], dtype=torch.int32, device=DEV)
    step(ce, group, mine, rule, opts, ids, grads, last_id=last)
    grad = ce.MixedGroupedGrad(ids, grads, last, group.row_base, group.row_base_device, group.widths)
    for t, (local_ids, local_rows) in enumerate(grad.per_table()):
        local_rows = local_rows.contiguous()
        if rule in ("adam", "rowwise_adam"):
            ce.sparse_row_adam(theirs.tables[t], local_ids, local_rows, exp_avg=theirs.states[0][t],
                               exp_avg_sq=theirs.states[1][t], lr=LR, betas=BETAS, eps=EPS, rowwise=rule == "rowwise_adam", **opts)
        else:
            ce.sparse_row_update(theirs.tables[t], local_ids, local_rows, rule=rule, lr=LR, eps=EPS,
                                 state=theirs.states[0][t] if theirs.states else None)
    torch.cuda.synchronize()
    assert same_bits(mine.tensors(), theirs.tensors())
    assert not same_bits(mine.tables, Side(dtype, rows, widths, rule).tables)


@pytest.mark.parametrize("rule", ["rowwise_adagrad", "rowwise_adam"])
def test_a_captured_step_replays_like_eager_steps(ce, rule):
    """forward + backward_and_apply on tables of different widths captured on one stream: no read-back anywhere, or the
    capture would fail.  One eager warm-up step and two replays equal three eager steps, bit for bit (grad_y holds
    multiples of 1/8, so the backward's sums are exact whatever their association)."""
    from cuembed_amd import optim
    dtype, rows, widths = GROUPS["f32_wide"]
    batch = 6
    idx, offsets = lookups(rows, batch, True, salt=3)
    grad_y = placed(((hashed_ints(batch * sum(widths), 5) % 33) - 16).double() / 8.0, (batch, sum(widths)), dtype)

    def fresh():
        group = ce.MixedTableGroup(Side(dtype, rows, widths, "sgd").tables)
        if rule == "rowwise_adam":
            return optim.MixedGroupSparseAdamUpdater(group, LR, betas=BETAS, eps=EPS, weight_decay=0.0125, rowwise=True)
        return optim.MixedGroupSparseUpdater(group, rule, LR, eps=EPS, initial_accumulator_value=0.125)

    def tensors(u):
        return list(u.group.tables) + (list(u.exp_avg) + list(u.exp_avg_sq) if hasattr(u, "exp_avg") else list(u.states))

    def one_step(u):
        ce.embedding_forward_mixed_group(u.group, idx, offsets)
        u.backward_and_apply(grad_y, idx, offsets)

    captured, eager = fresh(), fresh()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        one_step(captured)                               # warm-up outside capture (library loading, the group's device arrays)
        torch.cuda.current_stream().synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            one_step(captured)
    torch.cuda.synchronize()
    after_warm_up = [t.clone() for t in tensors(captured)]
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    for _ in range(3):
        one_step(eager)
    torch.cuda.synchronize()
    assert not same_bits(tensors(captured)[:len(rows)], after_warm_up[:len(rows)])
    assert same_bits(tensors(captured), tensors(eager))
    if hasattr(eager, "powers"):
        assert captured.powers[0].item() == 3.0 and torch.equal(captured.powers, eager.powers)


@pytest.mark.parametrize("rule", (FIVE[2], FIVE[3]), ids=rule_id)
def test_the_torch_ops_give_the_python_functions_bits(ce, rule):
    """cuembed_pyt::cuembed_sparse_row_update_mixed_group / cuembed_sparse_row_adam_mixed_group (one case each: row-wise
    Adagrad, lazy Adam with weight decay and a bias factor) against sparse_row_update_mixed_group /
    sparse_row_adam_mixed_group on clones, bit for bit."""
    from cuembed_amd import cuembed_pyt
    dtype, rows, widths = GROUPS["f16_wide"]
    rule, opts = rule
    mine, theirs = Side(dtype, rows, widths, rule), Side(dtype, rows, widths, rule)
    named = named_rows(rows, "all")
    ids, grads = gradient(dtype, rows, widths, named, torch.int64, 11)
    count = dict(count=torch.tensor([len(named)], dtype=torch.int32, device=DEV))
    if rule == "adam":
        cuembed_pyt.cuembed_sparse_row_adam_mixed_group(ce.MixedTableGroup(mine.tables), ids, grads, exp_avg=mine.states[0],
                                                        exp_avg_sq=mine.states[1], lr=LR, betas=BETAS, eps=EPS, **opts, **count)
    else:
        cuembed_pyt.cuembed_sparse_row_update_mixed_group(ce.MixedTableGroup(mine.tables), ids, grads, rule=rule, lr=LR,
                                                          eps=EPS, states=mine.states[0], **count)
    step(ce, ce.MixedTableGroup(theirs.tables), theirs, rule, opts, ids, grads, **count)
    torch.cuda.synchronize()
    assert same_bits(mine.tensors(), theirs.tensors())
    assert not same_bits(mine.tables, Side(dtype, rows, widths, rule).tables)
