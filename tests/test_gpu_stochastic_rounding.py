"""Stochastic rounding of the sparse optimizer step on the GPU: the table after cuembed_amd.ops.sparse_row_update(...,
stochastic_rounding=True), cuembed_amd.optim and the torch op, bit for bit against the host reference
(tests/stochastic_rounding_reference.py) -- the random field of (seed, step, table row, column) applied to the fp32 value
the kernel stores -- on the smallest shapes that reach every lane width, body and count source."""
import copy

import numpy as np
import pytest
import torch

import stochastic_rounding_reference as S

pytestmark = pytest.mark.gpu

TORCH = {"fp16": torch.float16, "bf16": torch.bfloat16}
INDEX = {"i32": torch.int32, "i64": torch.int64}
NCAT, ENTRIES = 300, 37          # an odd count: one group's second in-flight entry is dead
LR, EPS, SEED = 0.0371, 1e-8, 0xC0FFEE1234567
# 8: one 16-byte lane; 50: 4-byte lanes; 100: 8-byte lanes; 256: one slice per lane, two entries in flight; 1000: four
# slices per lane; 2056: the run-time loop (257 lanes of 16 bytes)
WIDTHS = [8, 50, 100, 256, 1000, 2056]


@pytest.fixture(scope="module")
def ce():
    import cuembed_amd
    assert torch.cuda.is_available()
    return cuembed_amd


def dev(bits_, kind):
    """uint16 patterns -> a GPU tensor of the table's dtype."""
    return torch.from_numpy(np.ascontiguousarray(bits_).view(np.int16)).view(TORCH[kind]).cuda()


def pat(t):
    """A 16-bit GPU tensor's patterns on the host."""
    return t.detach().contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def f32bits(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy()


def problem(kind, width, seed=0, ncat=NCAT, entries=ENTRIES, grads=None):
    """Arbitrary (non-representable update) data: table / gradient patterns and random distinct row ids."""
    rng = np.random.default_rng(1000 * width + seed)
    table = S.nearest(rng.standard_normal((ncat, width)).astype(np.float32), kind)
    if grads is None:
        grad = S.nearest(rng.standard_normal((entries, width)).astype(np.float32), kind)
    else:
        grad = S.nearest((rng.choice(grads, size=(entries, width)) * rng.choice([-1.0, 1.0], size=(entries, width)))
                         .astype(np.float32), kind)
    ids = rng.permutation(ncat)[:entries].astype(np.int64)
    return table, ids, grad


# ---- SGD, bit for bit -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("index", ["i32", "i64"])
@pytest.mark.parametrize("kind", ["fp16", "bf16"])
def test_sgd_equals_the_host_reference(ce, kind, index, width):
    table, ids, grad = problem(kind, width)
    t = dev(table, kind)
    d_ids = torch.from_numpy(ids).to(INDEX[index]).cuda()
    want = table
    for step in (0, 1, 2):
        g = S.nearest(np.roll(S.to_f32(grad, kind), step, axis=0), kind)
        ce.sparse_row_update(t, d_ids, dev(g, kind), rule="sgd", lr=LR, stochastic_rounding=True, seed=SEED, step=step)
        want = S.sgd(want, ids, g, LR, kind, seed=SEED, step=step)
        assert np.array_equal(pat(t), want), "step %d" % step          # (the whole table: unnamed rows are untouched)
    assert not np.array_equal(want, S.sgd(S.sgd(S.sgd(table, ids, grad, LR, kind), ids, grad, LR, kind), ids, grad, LR, kind))


def offset_view(bits_, kind, elements):
    """The same values in a buffer whose base pointer is `elements` elements past an aligned address."""
    flat = torch.zeros((bits_.size + elements,), dtype=TORCH[kind], device="cuda")
    view = flat[elements:].view(bits_.shape)
    view.copy_(dev(bits_, kind))
    assert view.data_ptr() % 16 == 2 * elements and view.is_contiguous()
    return view


@pytest.mark.parametrize("kind", ["fp16", "bf16"])
def test_the_bits_do_not_depend_on_the_lane_width(ce, kind):
    """width 256 takes 16-byte lanes; a table 4 bytes off takes 4-byte lanes, gradient rows 8 bytes off 8-byte lanes
    (a lane then computes the Philox call of its column group and picks its fields): the same table."""
    table, ids, grad = problem(kind, 256)
    d_ids = torch.from_numpy(ids).cuda()
    want = S.sgd(table, ids, grad, LR, kind, seed=SEED, step=5)
    for table_off, rows_off in ((0, 0), (2, 0), (0, 4), (4, 2)):
        t = offset_view(table, kind, table_off)
        ce.sparse_row_update(t, d_ids, offset_view(grad, kind, rows_off), rule="sgd", lr=LR, stochastic_rounding=True,
                             seed=SEED, step=5)
        assert np.array_equal(pat(t), want), (table_off, rows_off)


@pytest.mark.parametrize("kind", ["fp16", "bf16"])
@pytest.mark.parametrize("width", [64, 1000])
def test_the_bits_do_not_depend_on_the_count_source(ce, kind, width):
    """29 valid entries of 37 by a host count, last_id, a device count word and counts[2] over two pieces: the same
    table, which is the reference's; the entries past the count repeat valid rows with large gradients and do nothing."""
    table, ids, grad = problem(kind, width)
    valid = 29
    ids = ids.copy()
    ids[valid:] = ids[:ENTRIES - valid]                          # valid ids again ...
    grad = grad.copy()
    grad[valid:] = S.nearest(np.float32(64.0), kind)             # ... with rows that would show
    want = S.sgd(table, ids[:valid], grad[:valid], LR, kind, seed=SEED, step=3)
    assert np.array_equal(want[np.setdiff1d(np.arange(NCAT), ids[:valid])], table[np.setdiff1d(np.arange(NCAT), ids[:valid])])
    d_ids, d_grad = torch.from_numpy(ids).cuda(), dev(grad, kind)
    # two pieces of 19 entries holding 15 + 14 valid ones
    piece = 19
    ids2 = np.concatenate([ids[:15], ids[:piece - 15], ids[15:valid], ids[:piece - 14]])
    grad2 = np.concatenate([grad[:15], grad[valid:valid + piece - 15], grad[15:valid], grad[valid:valid + piece - 14]])
    sources = [
        (d_ids, d_grad, dict(count=valid)),
        (d_ids, d_grad, dict(last_id=torch.tensor([valid - 1], dtype=torch.int64, device="cuda"))),
        (d_ids, d_grad, dict(count=torch.tensor([valid], dtype=torch.int32, device="cuda"))),
        (d_ids, d_grad, dict(count=torch.tensor([valid], dtype=torch.int64, device="cuda"))),
        (torch.from_numpy(ids2).cuda(), dev(grad2, kind),
         dict(counts=torch.tensor([15, 14], dtype=torch.int32, device="cuda"), piece_rows=piece)),
    ]
    for i, g, kw in sources:
        t = dev(table, kind)
        ce.sparse_row_update(t, i, g, rule="sgd", lr=LR, stochastic_rounding=True, seed=SEED, step=3, **kw)
        assert np.array_equal(pat(t), want), sorted(kw)
    # the step from a device word
    t = dev(table, kind)
    ce.sparse_row_update(t, d_ids, d_grad, rule="sgd", lr=LR, stochastic_rounding=True, seed=SEED, count=valid,
                         step=torch.tensor([3], dtype=torch.int64, device="cuda"))
    assert np.array_equal(pat(t), want)


# ---- the Adagrad rules: the fp32 value from today's kernel on an fp32 twin ----------------------------------------------
def twin_check(ce, rule, kind, width, grads=None):
    table, ids, grad = problem(kind, width, seed=1, grads=grads)
    d_ids = torch.from_numpy(ids).cuda()
    shape = (NCAT, width) if rule == "adagrad" else (NCAT,)
    rng = np.random.default_rng(width)
    state0 = torch.from_numpy((rng.random(shape) * 0.5 + 0.125).astype(np.float32)).cuda()
    t, g = dev(table, kind), dev(grad, kind)
    # round to nearest on the 16-bit table: the state every variant must reach
    near_t, near_s = t.clone(), state0.clone()
    ce.sparse_row_update(near_t, d_ids, g, rule=rule, lr=LR, state=near_s, eps=EPS)
    # the fp32 twin: the rules are element-wise, so it stores the fp32 value x the 16-bit kernel rounds
    twin_t, twin_s = t.float(), state0.clone()
    ce.sparse_row_update(twin_t, d_ids, g.float(), rule=rule, lr=LR, state=twin_s, eps=EPS)
    x = twin_t.cpu().numpy()
    assert np.array_equal(pat(near_t), S.nearest(x, kind))                     # (the twin is a twin)
    sr_t, sr_s = t.clone(), state0.clone()
    ce.sparse_row_update(sr_t, d_ids, g, rule=rule, lr=LR, state=sr_s, eps=EPS, stochastic_rounding=True, seed=SEED, step=9)
    want = table.copy()
    want[ids] = S.stochastic(x[ids], S.fields(SEED, 9, ids, width), kind)
    got = pat(sr_t)
    assert np.array_equal(got, want)
    assert np.array_equal(f32bits(sr_s), f32bits(near_s)) and np.array_equal(f32bits(sr_s), f32bits(twin_s))
    assert not np.array_equal(f32bits(sr_s), f32bits(state0))
    # every stored value is one of the two neighbours of x in the table's type
    down, up = S.stochastic(x[ids], 0, kind), S.stochastic(x[ids], 0xFFFF, kind)
    assert ((got[ids] == down) | (got[ids] == up)).all()
    assert (got[ids] != S.nearest(x[ids], kind)).any()


@pytest.mark.parametrize("width", [8, 50, 256, 1000, 2056])
@pytest.mark.parametrize("kind", ["fp16", "bf16"])
def test_adagrad_equals_the_rounded_fp32_twin(ce, kind, width):
    twin_check(ce, "adagrad", kind, width)


@pytest.mark.parametrize("width", [8, 50, 256, 1000, 2056])
@pytest.mark.parametrize("kind", ["fp16", "bf16"])
def test_rowwise_adagrad_equals_the_rounded_fp32_twin(ce, kind, width):
    # gradients of +-{2^-3, 2^-4, 2^-5}: the row's sum of squares is exact in any summation order
    twin_check(ce, "rowwise_adagrad", kind, width, grads=[2.0 ** -3, 2.0 ** -4, 2.0 ** -5])


# ---- properties -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["fp16", "bf16"])
def test_properties(ce, kind):
    table, ids, grad = problem(kind, 136)
    d_ids, g = torch.from_numpy(ids).cuda(), dev(grad, kind)

    def run(lr=LR, **kw):
        t = dev(table, kind)
        ce.sparse_row_update(t, d_ids, g, rule="sgd", lr=lr, stochastic_rounding=True, **kw)
        return pat(t)

    assert np.array_equal(run(lr=0.0, seed=SEED, step=1), table)              # nothing to round: unchanged, bit for bit
    a = run(seed=SEED, step=1)
    assert np.array_equal(a, run(seed=SEED, step=1))                          # the same (seed, step): the same table
    assert not np.array_equal(a, run(seed=SEED, step=2))
    assert not np.array_equal(a, run(seed=SEED + 1, step=1))
    assert not np.array_equal(a, run(seed=SEED, step=1 + 2 ** 32))            # the step's high word counts too
    assert not np.array_equal(a, run(seed=SEED + 2 ** 32, step=1))
    x = S.sgd_value(table[ids], grad, LR, kind)
    assert ((a[ids] == S.stochastic(x, 0, kind)) | (a[ids] == S.stochastic(x, 0xFFFF, kind))).all()
    with pytest.raises(TypeError, match="float32 table"):
        ce.sparse_row_update(dev(table, kind).float(), d_ids, g.float(), rule="sgd", lr=LR, stochastic_rounding=True)
    with pytest.raises(ValueError, match="device"):
        ce.sparse_row_update(dev(table, kind), d_ids, g, rule="sgd", lr=LR, stochastic_rounding=True,
                             step=torch.zeros(1, dtype=torch.int64))


# ---- the symptom and the cure, on the device ----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["fp16", "bf16"])
def test_the_512_step_walk(ce, kind):
    from cuembed_amd import optim
    want, _, plain = S.walk(kind)
    ones = torch.ones((S.WALK_ROWS, S.WALK_WIDTH), dtype=TORCH[kind], device="cuda")
    ids = torch.arange(S.WALK_ROWS, device="cuda")
    sr = optim.SparseUpdater(ones.clone(), "sgd", S.WALK_LR[kind], stochastic_rounding=True, seed=S.WALK_SEED)
    near = optim.SparseUpdater(ones.clone(), "sgd", S.WALK_LR[kind])
    for _ in range(S.WALK_STEPS):
        sr.apply(ids, ones)
        near.apply(ids, ones)
    assert int(sr.rounding_step) == S.WALK_STEPS
    assert np.array_equal(pat(sr.table), want)
    assert np.array_equal(pat(near.table), plain) and bool((near.table == 1).all())      # the symptom
    # an fp32 table moves to 1 - 512 lr (1 - 2^-8 for fp16's lr); the 16-bit one follows within the 5 sigma of the
    # host test: 0.11 moves of one spacing below 1.0
    spacing = 2.0 ** -11 if kind == "fp16" else 2.0 ** -8
    mean = float(sr.table.double().mean())
    print("%s: table mean %.6f, fp32 %.6f" % (kind, mean, 1.0 - S.WALK_STEPS * S.WALK_LR[kind]))
    assert abs(mean - (1.0 - S.WALK_STEPS * S.WALK_LR[kind])) <= 0.11 * spacing


# ---- HIP graph ------------------------------------------------------------------------------------------------------------
def test_step_under_hip_graph_capture_draws_fresh_bits(ce):
    """forward + backward_and_apply with stochastic rounding captured once and replayed three times: the three eager
    steps of a second updater with the same seed, bit for bit -- the step word advances on the device -- and not what
    replaying with a frozen step gives."""
    from cuembed_amd import optim
    ncat, W, B, H = 200, 64, 64, 4
    rng = np.random.default_rng(3)
    table0 = torch.from_numpy(rng.standard_normal((ncat, W)).astype(np.float32)).half().cuda()
    batches = [torch.from_numpy(rng.integers(0, ncat, size=(B, H)).astype(np.int32)).cuda() for _ in range(3)]
    gy = torch.from_numpy(rng.standard_normal((B, W)).astype(np.float32)).half().cuda()

    def new_updater():
        return optim.SparseUpdater(table0.clone(), "sgd", 0.01, stochastic_rounding=True, seed=SEED)

    eager = new_updater()
    eager_out = torch.empty((B, W), dtype=torch.float16, device="cuda")
    for b in batches:
        ce.embedding_forward(eager.table, b.view(-1), num_hots=H, out=eager_out)
        eager.backward_and_apply(gy, b)
    torch.cuda.synchronize()

    def replayed(frozen):
        up = new_updater()
        idx = batches[0].clone()
        out = torch.empty((B, W), dtype=torch.float16, device="cuda")

        def step():
            ce.embedding_forward(up.table, idx.view(-1), num_hots=H, out=out)
            up.backward_and_apply(gy, idx)

        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            step()                               # warm-up outside capture (allocates the buffers); undone below
            up.table.copy_(table0)
            up.rounding_step.zero_()
            torch.cuda.current_stream().synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                step()
        torch.cuda.synchronize()
        for b in batches:
            idx.copy_(b)
            if frozen:
                up.rounding_step.zero_()
            g.replay()
        torch.cuda.synchronize()
        return up, out

    graph, graph_out = replayed(False)
    assert int(graph.rounding_step) == 3 and int(eager.rounding_step) == 3
    assert np.array_equal(pat(graph.table), pat(eager.table))
    assert np.array_equal(pat(graph_out), pat(eager_out))
    assert not np.array_equal(pat(eager.table), pat(table0))
    frozen, _ = replayed(True)
    assert not np.array_equal(pat(frozen.table), pat(eager.table))


# ---- front ends -------------------------------------------------------------------------------------------------------------
def _sparse_grad(ids_sorted, grad, kind):
    """Strictly ascending ids: what cuemb_embedding's coalesced gradient kinds deliver (the optimizers check that)."""
    return torch.sparse_coo_tensor(torch.from_numpy(ids_sorted).cuda()[None], dev(grad, kind), size=(NCAT, grad.shape[1]))


@pytest.mark.parametrize("name,rule", [("SparseSGD", "sgd"), ("SparseAdagrad", "adagrad"), ("RowwiseAdagrad", "rowwise_adagrad")])
def test_optimizers_equal_the_ops_call_and_resume_the_bit_stream(ce, name, rule):
    from cuembed_amd import optim
    kind, width, seed = "bf16", 72, 2 ** 64 - 12345
    table, ids, grad = problem(kind, width)
    ids = np.sort(ids)
    grads = [S.nearest(np.roll(S.to_f32(grad, kind), k, axis=1), kind) for k in range(4)]
    kw = {} if rule == "sgd" else dict(initial_accumulator_value=0.25)

    def optimizer(p):
        return getattr(optim, name)([p], 0.05, stochastic_rounding=True, seed=seed, **kw)

    # the uninterrupted run: four steps, against the ops call with the same seed and step
    p = torch.nn.Parameter(dev(table, kind))
    opt = optimizer(p)
    t = dev(table, kind)
    state = None if rule == "sgd" else torch.full((NCAT, width) if rule == "adagrad" else (NCAT,), 0.25, device="cuda")
    snapshots = []
    for step, g in enumerate(grads):
        p.grad = _sparse_grad(ids, g, kind)
        opt.step()
        ce.sparse_row_update(t, torch.from_numpy(ids).cuda(), dev(g, kind), rule=rule, lr=0.05, state=state, eps=1e-8,
                             stochastic_rounding=True, seed=seed, step=step)
        assert np.array_equal(pat(p.data), pat(t)), "step %d" % step
        snapshots.append(pat(p.data).copy())
        if step == 1:
            saved, saved_table = copy.deepcopy(opt.state_dict()), p.detach().clone()
    assert opt.state[p]["rounding_step"] == 4
    if rule == "sgd":
        assert np.array_equal(snapshots[0], S.sgd(table, ids, grads[0], 0.05, kind, seed=seed, step=0))
    # resumed after two steps: a new optimizer (with another seed until the state arrives) continues the same bits
    q = torch.nn.Parameter(saved_table)
    resumed = getattr(optim, name)([q], 0.05, stochastic_rounding=True, seed=1, **kw)
    resumed.load_state_dict(saved)
    for step in (2, 3):
        q.grad = _sparse_grad(ids, grads[step], kind)
        resumed.step()
        assert np.array_equal(pat(q.data), snapshots[step]), "resumed step %d" % step
    # without the feature's keywords the optimizer rounds to nearest, as before
    r = torch.nn.Parameter(dev(table, kind))
    plain = getattr(optim, name)([r], 0.05, **kw)
    r.grad = _sparse_grad(ids, grads[0], kind)
    plain.step()
    assert not np.array_equal(pat(r.data), snapshots[0])


@pytest.mark.parametrize("kind", ["fp16", "bf16"])
def test_torch_op(ce, kind):
    from cuembed_amd import cuembed_pyt as P
    width, seed = 40, 2 ** 63 + 99                                       # (a seed past the signed range)
    table, ids, grad = problem(kind, width)
    d_ids, g = torch.from_numpy(ids).cuda(), dev(grad, kind)
    want = dev(table, kind)
    ce.sparse_row_update(want, d_ids, g, rule="sgd", lr=LR, stochastic_rounding=True, seed=seed, step=6)
    assert np.array_equal(pat(want), S.sgd(table, ids, grad, LR, kind, seed=seed, step=6))
    t = dev(table, kind)
    P.cuembed_sparse_row_update_(t, d_ids, g, "sgd", LR, stochastic_rounding=True, seed=seed, step=6)
    assert np.array_equal(pat(t), pat(want))
    t = dev(table, kind)
    P.cuembed_sparse_row_update_(t, d_ids, g, "sgd", LR, stochastic_rounding=True, seed=seed,
                                 step=torch.tensor([6], dtype=torch.int64, device="cuda"))
    assert np.array_equal(pat(t), pat(want))
    # the raw op: 12 positional arguments as before (round to nearest), or the four new ones behind them
    t = dev(table, kind)
    torch.ops.cuembed_pyt.cuembed_sparse_row_update_(t, None, d_ids, g, "sgd", LR, 1e-8, None, -1, None, None, 0)
    assert np.array_equal(pat(t), S.sgd(table, ids, grad, LR, kind))
    t = dev(table, kind)
    torch.ops.cuembed_pyt.cuembed_sparse_row_update_(t, None, d_ids, g, "sgd", LR, 1e-8, None, -1, None, None, 0,
                                                     True, seed - 2 ** 64, 6, None)
    assert np.array_equal(pat(t), pat(want))
    with pytest.raises(Exception, match="float32"):
        P.cuembed_sparse_row_update_(t.float(), d_ids, g.float(), "sgd", LR, stochastic_rounding=True, seed=1, step=0)
