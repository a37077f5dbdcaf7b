"""The sparse optimizer step on the GPU: cuembed_amd.ops.sparse_row_update, cuembed_amd.optim and the torch op against
the fp64 rules of tests/optimizer_reference.py -- every element within the derived bounds, every row that is not named
(and its state) bit-identical to before."""
import numpy as np
import pytest
import torch

import optimizer_reference as R

pytestmark = pytest.mark.gpu

TORCH = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
INDEX = {"i32": torch.int32, "i64": torch.int64}
LR, EPS = 0.05, 1e-8


@pytest.fixture(scope="module")
def ce():
    import cuembed_amd
    assert torch.cuda.is_available()
    return cuembed_amd


def bits(t):
    """The tensor's bit patterns on the host (bf16 has no numpy dtype)."""
    t = t.detach().contiguous()
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32).cpu().numpy()


def f64(t):
    return t.detach().double().cpu().numpy()


def distinct_rows(oracle, ncat, batch, hot, index="i32"):
    """The distinct rows of a power-law batch from the oracle's generator, ascending (a coalesced gradient's ids)."""
    idx = oracle.generate_indices(ncat, batch, hot, alpha=1.15)
    return torch.from_numpy(np.unique(idx).astype(np.int64)).to(INDEX[index]).cuda()


def new_state(rule, ncat, width, fill=0.0):
    if rule == "sgd":
        return None
    shape = (ncat, width) if rule == "adagrad" else (ncat,)
    return torch.full(shape, fill, dtype=torch.float32, device="cuda")


def check_step(rule, kind, table0, state0, ids, rows, table1, state1, lr=LR, eps=EPS):
    """table1 / state1 (after) against the fp64 rule applied to table0 / state0 (before): named rows within the bounds,
    every other row and its state bit-identical.  Returns the worst ratios (weights, state)."""
    ncat, width = table0.shape
    named = ids.long().cpu().numpy()
    assert np.unique(named).size == named.size
    k = R.k_for(width)
    w0 = f64(table0)[named]
    s0 = None if state0 is None else f64(state0)[named]
    w_new, d, s_new = R.step(rule, w0, f64(rows), s0, lr, eps)
    worst_w = R.worst_ratio(f64(table1)[named], w_new, R.weight_bound(kind, w_new, w0, d, k))
    worst_s = 0.0 if state0 is None else R.worst_ratio(f64(state1)[named], s_new, R.state_bound(s_new, k))
    print("%s %s W=%d: worst weight error / bound = %.3f, state = %.3f" % (rule, kind, width, worst_w, worst_s))
    other = np.ones(ncat, dtype=bool)
    other[named] = False
    assert np.array_equal(bits(table1)[other], bits(table0)[other]), "a row that was not named changed"
    if state0 is not None:
        assert np.array_equal(bits(state1)[other], bits(state0)[other]), "the state of a row that was not named changed"
    assert worst_w <= 1.0 and worst_s <= 1.0
    return worst_w, worst_s


WIDTHS = [8, 50, 128, 256, 1000]


@pytest.mark.parametrize("index", ["i32", "i64"])
@pytest.mark.parametrize("kind", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("rule", R.RULES)
def test_rules_types_widths_and_two_steps(ce, oracle, rule, kind, index):
    """Every rule x type x index type x width (50: rows of 200 / 100 bytes, not a multiple of 16), gradients at scales
    1 and 2^-14, and a second step on the same rows (the state carries over)."""
    ncat = 3000
    for width in WIDTHS:
        ids = distinct_rows(oracle, ncat, 256, 8, index)
        for scale in (1.0, 2.0 ** -14):
            table = (torch.rand((ncat, width), device="cuda") * 2 - 1).to(TORCH[kind])
            state = new_state(rule, ncat, width)
            for _ in range(2):
                rows = ((torch.rand((ids.numel(), width), device="cuda") * 2 - 1) * scale).to(TORCH[kind])
                table0 = table.clone()
                state0 = None if state is None else state.clone()
                ce.sparse_row_update(table, ids, rows, rule=rule, lr=LR, state=state, eps=EPS)
                check_step(rule, kind, table0, state0, ids, rows, table, state)
            if state is not None:
                assert float(state.abs().max()) > 0


def padded_problem(oracle, kind, rule, width, ncat=2000):
    """A gradient whose buffers hold more entries than are valid: the tail holds VALID ids that repeat earlier ones,
    with non-zero rows."""
    ids = distinct_rows(oracle, ncat, 128, 8)
    n = ids.numel()
    cap = n + 37
    pad_ids = torch.cat([ids, ids[torch.arange(cap - n, device="cuda") % n]])
    rows = (torch.rand((cap, width), device="cuda") * 2 - 1).to(TORCH[kind])
    table = (torch.rand((ncat, width), device="cuda") * 2 - 1).to(TORCH[kind])
    return ids, n, pad_ids, rows, table


@pytest.mark.parametrize("rule", R.RULES)
def test_count_sources_ignore_the_tail(ce, oracle, rule):
    kind, width, ncat = "f16", 64, 2000
    ids, n, pad_ids, rows, table = padded_problem(oracle, kind, rule, width, ncat)
    want_t, want_s = table.clone(), new_state(rule, ncat, width, 0.5)
    ce.sparse_row_update(want_t, ids, rows[:n].contiguous(), rule=rule, lr=LR, state=want_s)   # the truncated input
    check_step(rule, kind, table, new_state(rule, ncat, width, 0.5), ids, rows[:n], want_t, want_s)
    sources = {
        "host count": dict(count=n),
        "count word int32": dict(count=torch.tensor([n], dtype=torch.int32, device="cuda")),
        "count word int64": dict(count=torch.tensor([n], dtype=torch.int64, device="cuda")),
        "last id": dict(last_id=torch.tensor([n - 1], dtype=torch.int32, device="cuda")),
        "one piece": dict(counts=torch.tensor([n], dtype=torch.int32, device="cuda"), piece_rows=pad_ids.numel()),
    }
    for name, kw in sources.items():
        t, s = table.clone(), new_state(rule, ncat, width, 0.5)
        ce.sparse_row_update(t, pad_ids, rows, rule=rule, lr=LR, state=s, **kw)
        assert np.array_equal(bits(t), bits(want_t)), name
        if s is not None:
            assert np.array_equal(bits(s), bits(want_s)), name
    # a count above the capacity (the backward wrote nothing then) and a negative one change nothing
    for word in (pad_ids.numel() + 1, -1):
        for dtype in (torch.int32, torch.int64):
            t, s = table.clone(), new_state(rule, ncat, width, 0.5)
            ce.sparse_row_update(t, pad_ids, rows, rule=rule, lr=LR, state=s,
                                 count=torch.tensor([word], dtype=dtype, device="cuda"))
            assert np.array_equal(bits(t), bits(table)), word
            if s is not None:
                assert float((s - 0.5).abs().max()) == 0.0
    t = table.clone()
    s = new_state(rule, ncat, width, 0.5)
    ce.sparse_row_update(t, pad_ids, rows, rule=rule, lr=LR, state=s,
                         last_id=torch.tensor([pad_ids.numel()], dtype=torch.int32, device="cuda"))
    assert np.array_equal(bits(t), bits(table))


@pytest.mark.parametrize("counts_dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("rule", R.RULES)
def test_three_pieces(ce, oracle, rule, counts_dtype):
    """Pieces with counts {0, 1, piece_rows}: the layout SparseGradResult.wait() returns.  The pieces own disjoint id
    ranges; the slots past a piece's count hold valid ids of that range with non-zero rows."""
    kind, width, ncat, piece = "f32", 32, 900, 40
    table = torch.rand((ncat, width), device="cuda") * 2 - 1
    ids = torch.cat([torch.randperm(300, device="cuda")[:piece] + 300 * p for p in range(3)]).to(torch.int64)
    rows = torch.rand((3 * piece, width), device="cuda") * 2 - 1
    counts = torch.tensor([0, 1, piece], dtype=counts_dtype, device="cuda")
    t, s = table.clone(), new_state(rule, ncat, width, 0.25)
    ce.sparse_row_update(t, ids, rows, rule=rule, lr=LR, state=s, counts=counts, piece_rows=piece)
    valid = torch.cat([torch.arange(piece, piece + 1), torch.arange(2 * piece, 3 * piece)]).cuda()
    check_step(rule, kind, table, new_state(rule, ncat, width, 0.25), ids[valid], rows[valid], t, s)
    want_t, want_s = table.clone(), new_state(rule, ncat, width, 0.25)
    ce.sparse_row_update(want_t, ids[valid].contiguous(), rows[valid].contiguous(), rule=rule, lr=LR, state=want_s)
    assert np.array_equal(bits(t), bits(want_t))
    if s is not None:
        assert np.array_equal(bits(s), bits(want_s))


@pytest.mark.parametrize("rule", R.RULES)
def test_lr_from_a_device_word(ce, oracle, rule):
    kind, width, ncat = "bf16", 128, 2000
    ids, n, _, rows, table = padded_problem(oracle, kind, rule, width, ncat)
    rows = rows[:n].contiguous()
    lr = float(np.float32(0.0371))
    a_t, a_s = table.clone(), new_state(rule, ncat, width)
    b_t, b_s = table.clone(), new_state(rule, ncat, width)
    ce.sparse_row_update(a_t, ids, rows, rule=rule, lr=lr, state=a_s)
    word = torch.tensor([lr], dtype=torch.float32, device="cuda")
    ce.sparse_row_update(b_t, ids, rows, rule=rule, lr=word, state=b_s)
    assert np.array_equal(bits(a_t), bits(b_t))
    assert not np.array_equal(bits(a_t), bits(table))
    if a_s is not None:
        assert np.array_equal(bits(a_s), bits(b_s))
    check_step(rule, kind, table, new_state(rule, ncat, width), ids, rows, b_t, b_s, lr=lr)


@pytest.mark.parametrize("kind", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("rule", R.RULES)
def test_rows_wider_than_the_register_path(ce, oracle, rule, kind):
    """2,050 elements: 1,025 lanes of 8 (fp32) or 4 (16-bit) bytes -- the run-time loop over a row's slices."""
    ncat, width = 300, 2050
    assert ce.sparse_row_update_launch_shape(TORCH[kind], width, 100)["slices_per_lane"] == 0
    ids = distinct_rows(oracle, ncat, 32, 4, "i64")
    table = (torch.rand((ncat, width), device="cuda") * 2 - 1).to(TORCH[kind])
    state = new_state(rule, ncat, width)
    for _ in range(2):
        rows = (torch.rand((ids.numel(), width), device="cuda") * 2 - 1).to(TORCH[kind])
        table0, state0 = table.clone(), None if state is None else state.clone()
        ce.sparse_row_update(table, ids, rows, rule=rule, lr=LR, state=state)
        check_step(rule, kind, table0, state0, ids, rows, table, state)


# ---- SparseUpdater: the whole backward + update without a read-back ---------------------------------------------------
def _reference_step(ce, rule, table, state, gy, idx, offsets, weights, lr):
    """embedding_backward (compressed, HOST-known count) followed by ops.sparse_row_update: what backward_and_apply must
    equal bit for bit.  Returns (ids, rows) of the compressed gradient."""
    ncat = table.shape[0]
    if offsets is None:
        t_idx, t_sid, t_w, remap = ce.transpose_fixed_hotness(idx, idx.shape[0], idx.shape[1], weights,
                                                              num_categories=ncat, remapped=True)
    else:
        sid = ce.extract_row_ids_from_csr(offsets, nnz=idx.numel(), dtype=idx.dtype)
        t_idx, t_sid, t_w, remap = ce.transpose(sid, idx, weights, num_categories=ncat, remapped=True)
    nu = int(remap[-1].item()) + 1
    rows, ids = ce.embedding_backward(gy, nu, t_idx, t_sid, remap, t_w)
    ce.sparse_row_update(table, ids, rows, rule=rule, lr=lr, state=state, count=nu)
    return ids, rows


@pytest.mark.parametrize("rule", R.RULES)
def test_backward_and_apply_on_config1(ce, oracle, rule):
    """C1 (fp32, 1 k x 32, B = 1,024, H = 8): forward + SparseUpdater.backward_and_apply."""
    from cuembed_amd import optim
    a = oracle.allocate_forward(1024, 32, 1024, 8, alpha=1.15)
    table = torch.from_numpy(a["table"]).cuda()
    idx = torch.from_numpy(a["indices"]).cuda().view(1024, 8)
    gy_np = oracle.allocate_grad_y(1024 * 32).reshape(1024, 32)
    gy = torch.from_numpy(gy_np).cuda()
    up = optim.SparseUpdater(table.clone(), rule, LR, initial_accumulator_value=0.1)
    out = ce.embedding_forward(up.table, idx.view(-1), num_hots=8)
    assert np.array_equal(out.cpu().numpy(), oracle.embedding_forward(a["table"], a["indices"], num_hots=8))
    up.backward_and_apply(gy, idx)
    want_t, want_s = table.clone(), new_state(rule, 1024, 32, 0.1)
    ids, rows = _reference_step(ce, rule, want_t, want_s, gy, idx, None, None, LR)
    assert np.array_equal(bits(up.table), bits(want_t))
    if want_s is not None:
        assert np.array_equal(bits(up.state), bits(want_s))
    # ... and within the bounds of the fp64 rule applied to the ORACLE's compressed gradient
    o_ti, o_ts, _ = oracle.transpose(oracle.extract_row_ids_from_fixed(1024, 8), a["indices"])
    o_remap = oracle.compute_compressed_grad_indices(o_ti)
    o_grad, o_inv = oracle.embedding_backward(gy_np, 32, int(o_remap[-1]) + 1, o_ti, o_ts, o_remap)
    check_step(rule, "f32", table, new_state(rule, 1024, 32, 0.1), torch.from_numpy(o_inv).cuda(),
               torch.from_numpy(o_grad).cuda(), up.table, up.state)


@pytest.mark.parametrize("kind", ["f32", "f16"])
@pytest.mark.parametrize("rule", R.RULES)
def test_backward_and_apply_on_a_weighted_csr_batch(ce, oracle, rule, kind):
    """(Integer-valued gradients and weights: a run that crosses workgroups arrives through atomics in any order, so
    two backward calls only agree bit for bit where every sum is exact.)"""
    ncat, width, batch = 5000, 64, 700
    lengths = torch.randint(0, 12, (batch,))
    offsets = torch.cat([torch.zeros(1, dtype=torch.int64), lengths.cumsum(0)]).to(torch.int32).cuda()
    nnz = int(lengths.sum())
    idx = torch.from_numpy(oracle.generate_indices(ncat, nnz, 1, alpha=1.15)[:nnz].astype(np.int32)).cuda()
    weights = torch.randint(1, 3, (nnz,), device="cuda").to(TORCH[kind])
    gy = torch.randint(-3, 4, (batch, width), device="cuda").to(TORCH[kind])
    table = (torch.rand((ncat, width), device="cuda") * 2 - 1).to(TORCH[kind])
    from cuembed_amd import optim
    ce.capacity_overflowed(reset=True)      # (the word is sticky and process-wide: other tests raise it on purpose)
    up = optim.SparseUpdater(table.clone(), rule, LR)
    for _ in range(2):                      # (the second call reuses the object's buffers)
        up.backward_and_apply(gy, idx, offsets, weights)
    want_t, want_s = table.clone(), new_state(rule, ncat, width)
    for _ in range(2):
        before_t, before_s = want_t.clone(), None if want_s is None else want_s.clone()
        ids, rows = _reference_step(ce, rule, want_t, want_s, gy, idx, offsets, weights, LR)
        check_step(rule, kind, before_t, before_s, ids, rows, want_t, want_s)
    assert np.array_equal(bits(up.table), bits(want_t))
    if want_s is not None:
        assert np.array_equal(bits(up.state), bits(want_s))
    assert not ce.capacity_overflowed()


@pytest.mark.parametrize("rule", R.RULES)
def test_step_under_hip_graph_capture(ce, oracle, rule):
    """forward + backward_and_apply captured on a side stream, replayed three times with new indices in the same buffers
    and a changed device-side lr: bit-identical to the eager sequence."""
    from cuembed_amd import optim
    ncat, W, B, H = 5000, 64, 512, 16
    table0 = torch.from_numpy(oracle.allocate_forward(ncat, W, B, H, alpha=1.15)["table"]).cuda()
    batches = [torch.from_numpy(oracle.generate_indices(ncat, B, H, alpha=al)).cuda().view(B, H)
               for al in (1.15, 0.0, 1.05, 1.3)]
    rates = [0.05, 0.02, 0.01, 0.04]
    gy = torch.from_numpy(oracle.allocate_grad_y(B * W).reshape(B, W)).cuda()

    def run(captured):
        idx = batches[0].clone()
        lr = torch.tensor([rates[0]], dtype=torch.float32, device="cuda")
        out = torch.empty((B, W), device="cuda")
        up = optim.SparseUpdater(table0.clone(), rule, lr, initial_accumulator_value=0.1)
        outs = []

        def step():
            ce.embedding_forward(up.table, idx.view(-1), num_hots=H, out=out)
            up.backward_and_apply(gy, idx)

        if not captured:
            for b, r in zip(batches, rates):
                idx.copy_(b)
                lr.fill_(r)
                step()
                outs.append(out.clone())
            torch.cuda.synchronize()
            return up, outs
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            step()                               # warm-up outside capture: this is step 0 of the sequence
            outs.append(out.clone())
            torch.cuda.current_stream().synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                step()
        torch.cuda.synchronize()
        # the capture itself ran nothing; replay steps 1..3
        for b, r in zip(batches[1:], rates[1:]):
            idx.copy_(b)
            lr.fill_(r)
            g.replay()
            outs.append(out.clone())
        torch.cuda.synchronize()
        return up, outs

    eager, eager_outs = run(False)
    graph, graph_outs = run(True)
    assert np.array_equal(bits(graph.table), bits(eager.table))
    assert not np.array_equal(bits(eager.table), bits(table0))
    if eager.state is not None:
        assert np.array_equal(bits(graph.state), bits(eager.state))
    for a, b in zip(eager_outs, graph_outs):
        assert np.array_equal(bits(a), bits(b))


# ---- torch.optim front ends ----------------------------------------------------------------------------------------
def _sparse_grad_problem(kind, ncat=4000, width=64, batch=300, hot=6):
    from cuembed_amd import cuembed_pyt as P
    w = torch.nn.Parameter((torch.rand((ncat, width), device="cuda") * 2 - 1).to(TORCH[kind]))
    idx = (torch.rand((batch * hot,), device="cuda") ** 3 * ncat).long().clamp_(max=ncat - 1)
    off = torch.arange(0, batch * hot + 1, hot, device="cuda")
    scale = (torch.rand((batch, width), device="cuda") * 2 - 1).to(TORCH[kind])

    def backward():
        w.grad = None
        (P.cuemb_embedding(w, idx, off, sparse_grad=True) * scale).sum().backward()
        assert w.grad.is_sparse       # (autograd's accumulation drops the is_coalesced flag the backward had set)
    return w, backward


@pytest.mark.parametrize("kind", ["f32", "f16"])
@pytest.mark.parametrize("rule", R.RULES)
def test_optimizers_after_a_sparse_backward(ce, rule, kind):
    """SparseSGD / SparseAdagrad against torch.optim.SGD / Adagrad on an fp32 copy of the table on the GPU, RowwiseAdagrad
    against the helper; two steps; then state_dict() -> a new optimizer -> the same next step."""
    from cuembed_amd import optim
    w, backward = _sparse_grad_problem(kind)
    cls = {"sgd": optim.SparseSGD, "adagrad": optim.SparseAdagrad, "rowwise_adagrad": optim.RowwiseAdagrad}[rule]
    opt = cls([w], lr=LR)
    for _ in range(2):
        backward()
        g = w.grad
        ids, rows = g._indices()[0].clone(), g._values().clone()
        before = w.detach().clone()
        state0 = None if rule == "sgd" else opt.state[w]["sum"].clone()
        if rule != "rowwise_adagrad":
            # torch's optimizer on an fp32 copy, from the same stored values and the same sparse gradient
            ref = torch.nn.Parameter(before.float().clone())       # (.float() of an fp32 tensor is the tensor itself)
            t_opt = torch.optim.SGD([ref], lr=LR) if rule == "sgd" else torch.optim.Adagrad([ref], lr=LR, eps=1e-8)
            if rule == "adagrad":
                t_opt.state[ref]["sum"].copy_(state0)
            ref.grad = torch.sparse_coo_tensor(g._indices(), rows.float(), size=g.shape, is_coalesced=True)
            t_opt.step()
        opt.step()
        state1 = None if rule == "sgd" else opt.state[w]["sum"]
        check_step(rule, kind, before, state0, ids, rows, w.detach(), state1)
        if rule != "rowwise_adagrad":
            # torch's fp32 result is itself within the fp32 part of the bound of the exact one
            named = ids.cpu().numpy()
            w_new, d, _ = R.step(rule, f64(before)[named], f64(rows), None if state0 is None else f64(state0)[named], LR)
            assert R.worst_ratio(f64(ref)[named], w_new, R.weight_bound("f32", w_new, f64(before)[named], d)) <= 1.0
            other = torch.ones(w.shape[0], dtype=torch.bool, device="cuda")
            other[ids] = False
            assert torch.equal(ref.detach()[other], before.float()[other])
    # state_dict() -> a new optimizer -> the same next step
    backward()
    twin_w = torch.nn.Parameter(w.detach().clone())
    twin_w.grad = torch.sparse_coo_tensor(w.grad._indices().clone(), w.grad._values().clone(), size=w.grad.shape,
                                          is_coalesced=True)
    twin = cls([twin_w], lr=0.5)
    twin.load_state_dict(opt.state_dict())
    opt.step()
    twin.step()
    assert np.array_equal(bits(twin_w), bits(w))
    if rule != "sgd":
        assert np.array_equal(bits(twin.state[twin_w]["sum"]), bits(opt.state[w]["sum"]))
        assert twin.state[twin_w]["sum"].dtype == torch.float32


@pytest.mark.parametrize("sparse_grad", ["uncoalesced", "padded"])
def test_optimizers_reject_the_uncoalesced_kinds_on_the_gpu(ce, sparse_grad):
    from cuembed_amd import cuembed_pyt as P
    from cuembed_amd import optim
    w = torch.nn.Parameter(torch.rand((3000, 32), device="cuda"))
    idx = torch.randint(0, 3000, (64 * 4,), device="cuda")
    off = torch.arange(0, 64 * 4 + 1, 4, device="cuda")
    P.cuemb_embedding(w, idx, off, sparse_grad=sparse_grad).sum().backward()
    before = w.detach().clone()
    ids = w.grad._indices()[0]
    if not bool((ids[1:] > ids[:-1]).all()):       # ("uncoalesced" is one block, hence coalesced, at small sizes)
        with pytest.raises(ValueError, match="COALESCED"):
            optim.SparseSGD([w], lr=0.1).step()
        assert torch.equal(w.detach(), before)
    else:
        assert sparse_grad != "padded"


# ---- the torch op ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", R.RULES)
def test_torch_op_eager_and_compiled(ce, oracle, rule):
    from cuembed_amd import cuembed_pyt as P
    kind, width, ncat = "f16", 64, 2000
    ids, n, pad_ids, rows, table = padded_problem(oracle, kind, rule, width, ncat)
    word = torch.tensor([n], dtype=torch.int32, device="cuda")
    want_t, want_s = table.clone(), new_state(rule, ncat, width)
    ce.sparse_row_update(want_t, pad_ids, rows, rule=rule, lr=LR, state=want_s, count=word)
    assert not np.array_equal(bits(want_t), bits(table))
    op_t, op_s = table.clone(), new_state(rule, ncat, width)
    P.cuembed_sparse_row_update_(op_t, pad_ids, rows, rule, LR, state=op_s, count=word)
    assert np.array_equal(bits(op_t), bits(want_t))

    def fn(t, s, i, r, c):
        torch.ops.cuembed_pyt.cuembed_sparse_row_update_(t, s, i, r, rule, LR, 1e-8, None, -1, c, None, 0)
        return t + 0

    c_t, c_s = table.clone(), new_state(rule, ncat, width)
    try:
        got = torch.compile(fn, fullgraph=True)(c_t, c_s, pad_ids, rows, word)
    except Exception as e:  # noqa: BLE001 - no working inductor toolchain on the box: trace with aot_eager instead
        print("inductor unavailable (%s): aot_eager" % type(e).__name__)
        torch._dynamo.reset()
        c_t, c_s = table.clone(), new_state(rule, ncat, width)
        got = torch.compile(fn, fullgraph=True, backend="aot_eager")(c_t, c_s, pad_ids, rows, word)
    assert np.array_equal(bits(c_t), bits(want_t)) and np.array_equal(bits(got), bits(want_t))
    if want_s is not None:
        assert np.array_equal(bits(op_s), bits(want_s)) and np.array_equal(bits(c_s), bits(want_s))


_PYTHON_BACKEND_CHILD = """
import sys, torch
sys.path.insert(0, %r)
import cuembed_amd as ce
from cuembed_amd import cuembed_pyt as P
assert P.BACKEND == "python"
torch.manual_seed(3)
table = torch.rand((500, 32), device="cuda").half()
ids = torch.randperm(500, device="cuda")[:64].int()
rows = (torch.rand((64, 32), device="cuda") - 0.5).half()
word = torch.tensor([40], dtype=torch.int64, device="cuda")
for rule in ("sgd", "adagrad", "rowwise_adagrad"):
    shape = None if rule == "sgd" else ((500, 32) if rule == "adagrad" else (500,))
    a_t, b_t = table.clone(), table.clone()
    a_s = None if shape is None else torch.zeros(shape, device="cuda")
    b_s = None if shape is None else torch.zeros(shape, device="cuda")
    ce.sparse_row_update(a_t, ids, rows, rule=rule, lr=0.05, state=a_s, count=word)
    P.cuembed_sparse_row_update_(b_t, ids, rows, rule, 0.05, state=b_s, count=word)
    assert torch.equal(a_t, b_t) and not torch.equal(a_t, table), rule
    assert a_s is None or torch.equal(a_s, b_s), rule
print("python backend OK")
"""


def test_torch_op_from_the_python_backend():
    """CUEMBED_PYT_BACKEND=python registers the same op from Python (a fresh process: the backend is chosen at import)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, CUEMBED_PYT_BACKEND="python")
    r = subprocess.run([sys.executable, "-c", _PYTHON_BACKEND_CHILD % root], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and "python backend OK" in r.stdout, r.stdout


# ---- the exchange's pieces ---------------------------------------------------------------------------------------------
def test_exchange_result_apply_to(ce):
    """SparseGradResult.apply_to feeds (ids, rows, counts, piece) to the pieces form: same table as the update with the
    exact rows."""
    from cuembed_amd import distributed as D
    from cuembed_amd import optim
    ncat, width, world, piece = 900, 16, 3, 50
    tail = torch.zeros((world, piece + 2), dtype=torch.int64, device="cuda")
    rows = torch.rand((world * piece, width), device="cuda") * 2 - 1
    counts = [0, 1, piece]
    for r in range(world):
        tail[r, :piece] = torch.randperm(300, device="cuda")[:piece] + 300 * r      # valid ids of the owner's range
        tail[r, piece] = counts[r]
    result = D.SparseGradResult([], tail.view(-1), rows, piece, world)
    table = torch.rand((ncat, width), device="cuda")
    up = optim.SparseUpdater(table.clone(), "rowwise_adagrad", LR)
    result.apply_to(up)
    valid = torch.cat([torch.arange(r * piece, r * piece + counts[r]) for r in range(world)]).cuda()
    ids = tail[:, :piece].reshape(-1)[valid]
    check_step("rowwise_adagrad", "f32", table, new_state("rowwise_adagrad", ncat, width), ids, rows[valid], up.table,
               up.state)


# ---- full size ---------------------------------------------------------------------------------------------------------
def test_config4_gradient_full_size(ce):
    """C4 (10 M x 256 fp16, B = 65,536, H = 64): the library's own 572,029-row gradient, SGD and row-wise Adagrad; the
    fp64 rule on a seeded sample of 4,096 named rows and 4,096 rows that were not named (unchanged)."""
    from cuembed_amd import harness
    from cuembed_amd import optim
    ncat, W, B, H = 10_000_000, 256, 65536, 64
    idx = torch.from_numpy(harness.generate_indices(ncat, B, H, alpha=1.15)).cuda().view(B, H)
    g = torch.Generator(device="cuda").manual_seed(11)
    table = torch.empty((ncat, W), dtype=torch.float16, device="cuda")
    for lo in range(0, ncat, 1_000_000):          # (in slices: no fp32 temporary of the whole table)
        table[lo:lo + 1_000_000] = (torch.rand((1_000_000, W), device="cuda", generator=g) * 2 - 1).half()
    gy = ((torch.rand((B, W), device="cuda", generator=g) * 2 - 1) * 2.0 ** -4).half()
    t_idx, t_sid, _, remap = ce.transpose_fixed_hotness(idx, B, H, num_categories=ncat, remapped=True)
    nu = int(remap[-1].item()) + 1
    assert nu == 572029
    rows, ids = ce.embedding_backward(gy, nu, t_idx, t_sid, remap)
    pick = torch.randperm(nu, device="cuda", generator=g)[:4096]
    named = ids[pick].long()
    is_named = torch.zeros(ncat, dtype=torch.bool, device="cuda")
    is_named[ids.long()] = True
    others = (~is_named).nonzero().squeeze(1)
    others = others[torch.randperm(others.numel(), device="cuda", generator=g)[:4096]]
    del is_named
    before_named, before_others = table[named].clone(), table[others].clone()
    for rule in ("sgd", "rowwise_adagrad"):
        up = optim.SparseUpdater(table, rule, LR, initial_accumulator_value=0.01)
        if rule == "sgd":
            up.apply(ids, rows, count=nu)
        else:
            up.apply(ids, rows, last_id=remap[-1:])         # the count read on the device
        s0 = None if rule == "sgd" else np.full(4096, float(np.float32(0.01)))
        w_new, d, s_new = R.step(rule, f64(before_named), f64(rows[pick]), s0, LR)
        got = f64(table[named])
        worst = R.worst_ratio(got, w_new, R.weight_bound("f16", w_new, f64(before_named), d))
        print("C4 %s: checksum of the sampled rows %.17g (fp64 rule: %.17g), worst error / bound %.3f"
              % (rule, got.sum(), w_new.sum(), worst))
        assert worst <= 1.0
        if rule != "sgd":
            assert R.worst_ratio(f64(up.state[named]), s_new, R.state_bound(s_new)) <= 1.0
            assert float((up.state[others] - 0.01).abs().max()) == 0.0
        assert np.array_equal(bits(table[others]), bits(before_others))
        before_named = table[named].clone()
        del up
