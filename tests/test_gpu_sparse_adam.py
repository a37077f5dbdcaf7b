"""The sparse Adam step on the GPU: cuembed_amd.ops.sparse_row_adam, the bias-factor clock, cuembed_amd.optim's
SparseAdamUpdater / SparseAdam / RowwiseAdam and the torch op against the fp64 rules of tests/adam_reference.py -- every
element of the named rows and of both moments within the derived bounds, every row that is not named bit-identical to
before in the table and in both moments -- on the smallest shapes that reach every lane width, body and count source."""
import numpy as np
import pytest
import torch

import adam_reference as R
import stochastic_rounding_reference as S

pytestmark = pytest.mark.gpu

TORCH = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
INDEX = {"i32": torch.int32, "i64": torch.int64}
LR, EPS, BETAS = 0.05, 1e-8, (0.9, 0.999)


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


def moments(rule, ncat, width, fill=0.0):
    """(exp_avg, exp_avg_sq) filled with (fill, fill^2)."""
    m = torch.full((ncat, width), fill, dtype=torch.float32, device="cuda")
    v = torch.full((ncat, width) if rule == "adam" else (ncat,), fill * fill, dtype=torch.float32, device="cuda")
    return m, v


def adam(ce, rule, table, ids, rows, m, v, **kw):
    kw.setdefault("lr", LR)
    kw.setdefault("betas", BETAS)
    kw.setdefault("eps", EPS)
    ce.sparse_row_adam(table, ids, rows, exp_avg=m, exp_avg_sq=v, rowwise=rule == "rowwise_adam", **kw)


def check_step(rule, kind, before, ids, rows, after, lr=LR, bias_factor=1.0, betas=BETAS, eps=EPS, weight_decay=0.0):
    """after = (table, exp_avg, exp_avg_sq) against the fp64 rule applied to before = (table, exp_avg, exp_avg_sq): the
    named rows within the bounds, every other row bit-identical in all three.  Returns the worst ratios (w, m, v)."""
    table0, m0, v0 = before
    table1, m1, v1 = after
    ncat, width = table0.shape
    named = ids.long().cpu().numpy()
    assert np.unique(named).size == named.size
    k = R.k_for(width)
    sc = R.scalars(lr, bias_factor, betas, eps, weight_decay)
    w0 = f64(table0)[named]
    r = R.step(rule, w0, f64(rows), f64(m0)[named], f64(v0)[named], sc)
    worst = (R.worst_ratio(f64(table1)[named], r["w"], R.weight_bound(kind, r, w0, k)),
             R.worst_ratio(f64(m1)[named], r["m"], R.exp_avg_bound(r, k)),
             R.worst_ratio(f64(v1)[named], r["v"], R.exp_avg_sq_bound(r, k)))
    print("%s %s W=%d: worst error / bound: weights %.3f, exp_avg %.3f, exp_avg_sq %.3f" % ((rule, kind, width) + worst))
    other = np.ones(ncat, dtype=bool)
    other[named] = False
    assert np.array_equal(bits(table1)[other], bits(table0)[other]), "a row that was not named changed"
    assert np.array_equal(bits(m1)[other], bits(m0)[other]), "exp_avg of a row that was not named changed"
    assert np.array_equal(bits(v1)[other], bits(v0)[other]), "exp_avg_sq of a row that was not named changed"
    assert max(worst) <= 1.0, worst
    return worst


def clones(*ts):
    return tuple(t.clone() for t in ts)


# 8: one 16-byte lane (fp32: two); 50: rows of 200 / 100 bytes, not a multiple of 16; 128, 256: one slice per lane, two
# entries in flight; 1000: four slices per lane with a partial last one; 2048: fp32 rows take the run-time loop
WIDTHS = [8, 50, 128, 256, 1000, 2048]


@pytest.mark.parametrize("index", ["i32", "i64"])
@pytest.mark.parametrize("kind", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("rule", R.RULES)
def test_rules_types_widths_and_three_steps(ce, oracle, rule, kind, index):
    """Every rule x type x index type x width; gradients at scale 1 (no weight decay, moments from zero) and 2^-14
    (weight_decay 0.01, moments that start away from zero); three consecutive steps with the bias factor of steps
    1 to 3, every one checked against the reference."""
    ncat = 3000
    assert ce.sparse_row_update_launch_shape(torch.float32, 2048, 100)["slices_per_lane"] == 0
    ids = distinct_rows(oracle, ncat, 256, 8, index)
    for width in WIDTHS:
        for scale, wd, start in ((1.0, 0.0, 0.0), (2.0 ** -14, 0.01, 2.0 ** -15)):
            table = (torch.rand((ncat, width), device="cuda") * 2 - 1).to(TORCH[kind])
            m, v = moments(rule, ncat, width, start)
            for t in (1, 2, 3):
                rows = ((torch.rand((ids.numel(), width), device="cuda") * 2 - 1) * scale).to(TORCH[kind])
                before = clones(table, m, v)
                c = ce.adam_bias_factor(t, BETAS)
                adam(ce, rule, table, ids, rows, m, v, bias_factor=c, weight_decay=wd)
                check_step(rule, kind, before, ids, rows, (table, m, v), bias_factor=c, weight_decay=wd)
            assert float(m.abs().max()) > 0 and float(v.max()) > 0


@pytest.mark.parametrize("rule", R.RULES)
def test_more_entries_than_one_pass_of_the_grid(ce, rule):
    """At 3,000 rows the grid covers every entry in one pass, so a group's second in-flight entry and the grid stride
    never carry work.  Here they do: f16, W = 64 (8 lanes per entry, one slice per lane), one sixteenth more entries
    than the device's resident groups hold, plus 37 for a ragged last pass."""
    kind, width = "f16", 64
    shape = ce.sparse_row_update_launch_shape(TORCH[kind], width, 1 << 30, compute_units=0)
    assert shape["slices_per_lane"] == 1
    per_pass = shape["grid"] * (256 // shape["lanes_per_entry"])         # entries one pass of the largest grid covers
    n = per_pass + per_pass // 16 + 37                                    # (69,669 on 256 compute units)
    ncat = n + n // 7
    assert ce.sparse_row_update_launch_shape(TORCH[kind], width, n, compute_units=0)["grid"] == shape["grid"]
    assert per_pass < n < 2 * per_pass and n % per_pass != 0
    ids = torch.randperm(ncat, device="cuda")[:n].to(torch.int32)
    table = (torch.rand((ncat, width), device="cuda") * 2 - 1).to(TORCH[kind])
    rows = (torch.rand((n, width), device="cuda") * 2 - 1).to(TORCH[kind])
    m, v = moments(rule, ncat, width, 0.25)
    before = clones(table, m, v)
    c = ce.adam_bias_factor(2, BETAS)
    adam(ce, rule, table, ids, rows, m, v, bias_factor=c, weight_decay=0.01)
    check_step(rule, kind, before, ids, rows, (table, m, v), bias_factor=c, weight_decay=0.01)


def padded_problem(oracle, kind, width, ncat=2000):
    """A gradient whose buffers hold more entries than are valid: the tail holds VALID ids that repeat earlier ones,
    with non-zero rows."""
    ids = distinct_rows(oracle, ncat, 128, 8)
    n = ids.numel()
    cap = n + 37
    pad_ids = torch.cat([ids, ids[torch.arange(cap - n, device="cuda") % n]])
    rows = (torch.rand((cap, width), device="cuda") * 2 - 1).to(TORCH[kind])
    table = (torch.rand((ncat, width), device="cuda") * 2 - 1).to(TORCH[kind])
    return ids, n, pad_ids, rows, table


def same(a, b):
    return all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


@pytest.mark.parametrize("rule", R.RULES)
def test_count_sources_ignore_the_tail(ce, oracle, rule):
    kind, width, ncat = "f16", 64, 2000
    ids, n, pad_ids, rows, table = padded_problem(oracle, kind, width, ncat)
    start = (table,) + moments(rule, ncat, width, 0.5)
    want = clones(*start)
    adam(ce, rule, want[0], ids, rows[:n].contiguous(), want[1], want[2], bias_factor=0.3)      # the truncated input
    check_step(rule, kind, start, ids, rows[:n], want, bias_factor=0.3)
    cap = pad_ids.numel()
    sources = {
        "host count": dict(count=n),
        "count word int32": dict(count=torch.tensor([n], dtype=torch.int32, device="cuda")),
        "count word int64": dict(count=torch.tensor([n], dtype=torch.int64, device="cuda")),
        "last id": dict(last_id=torch.tensor([n - 1], dtype=torch.int32, device="cuda")),
        "one piece": dict(counts=torch.tensor([n], dtype=torch.int32, device="cuda"), piece_rows=cap),
    }
    for name, kw in sources.items():
        got = clones(*start)
        adam(ce, rule, got[0], pad_ids, rows, got[1], got[2], bias_factor=0.3, **kw)
        assert same(got, want), name
    # a count above the capacity (the backward wrote nothing then) and a negative one change nothing
    for word in (cap + 1, -1):
        for dtype in (torch.int32, torch.int64):
            got = clones(*start)
            adam(ce, rule, got[0], pad_ids, rows, got[1], got[2], count=torch.tensor([word], dtype=dtype, device="cuda"))
            assert same(got, start), word
    got = clones(*start)
    adam(ce, rule, got[0], pad_ids, rows, got[1], got[2], last_id=torch.tensor([cap], dtype=torch.int32, device="cuda"))
    assert same(got, start)


@pytest.mark.parametrize("counts_dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("rule", R.RULES)
def test_three_pieces(ce, rule, counts_dtype):
    """Pieces with counts {0, 1, piece_rows}; the slots past a piece's count hold valid ids of the piece's range with
    non-zero rows."""
    kind, width, ncat, piece = "f32", 32, 900, 40
    table = torch.rand((ncat, width), device="cuda") * 2 - 1
    ids = torch.cat([torch.randperm(300, device="cuda")[:piece] + 300 * p for p in range(3)]).to(torch.int64)
    rows = torch.rand((3 * piece, width), device="cuda") * 2 - 1
    counts = torch.tensor([0, 1, piece], dtype=counts_dtype, device="cuda")
    start = (table,) + moments(rule, ncat, width, 0.25)
    got = clones(*start)
    adam(ce, rule, got[0], ids, rows, got[1], got[2], counts=counts, piece_rows=piece, weight_decay=0.01)
    valid = torch.cat([torch.arange(piece, piece + 1), torch.arange(2 * piece, 3 * piece)]).cuda()
    check_step(rule, kind, start, ids[valid], rows[valid], got, weight_decay=0.01)
    want = clones(*start)
    adam(ce, rule, want[0], ids[valid].contiguous(), rows[valid].contiguous(), want[1], want[2], weight_decay=0.01)
    assert same(got, want)


@pytest.mark.parametrize("kind", ["f32", "f16"])
@pytest.mark.parametrize("rule", R.RULES)
def test_a_misaligned_moment_narrows_the_lanes(ce, oracle, rule, kind):
    """exp_avg 4 bytes off a 16-byte boundary under an fp32 table (lanes of one element), 8 bytes off under an fp16
    table (lanes of two: a 16-bit table's narrowest lane moves 8 bytes of state, so 4 bytes off is refused); for adam,
    exp_avg_sq off by other amounts on top.  Bit-identical to the aligned run (gradients of +-2^-3 .. 2^-5 keep the
    row-wise sum exact in any order)."""
    width, ncat = 256, 1500
    ids = distinct_rows(oracle, ncat, 64, 8)
    table = (torch.rand((ncat, width), device="cuda") * 2 - 1).to(TORCH[kind])
    mag = torch.tensor([2.0 ** -3, 2.0 ** -4, 2.0 ** -5], device="cuda")[torch.randint(0, 3, (ids.numel(), width), device="cuda")]
    rows = (mag * (torch.randint(0, 2, mag.shape, device="cuda") * 2 - 1)).to(TORCH[kind])
    start = (table,) + moments(rule, ncat, width, 0.5)

    def offset(t, elements):
        flat = torch.zeros((t.numel() + elements,), dtype=t.dtype, device="cuda")
        view = flat[elements:].view(t.shape)
        view.copy_(t)
        assert view.data_ptr() % 16 == (4 * elements) % 16 and view.is_contiguous()
        return view

    want = clones(*start)
    adam(ce, rule, want[0], ids, rows, want[1], want[2], bias_factor=0.7, weight_decay=0.01)
    check_step(rule, kind, start, ids, rows, want, bias_factor=0.7, weight_decay=0.01)
    unit = 1 if kind == "f32" else 2                     # fp32 elements of state per narrowest lane
    for m_off, v_off in ((1, 0), (0, 2), (1, 2), (3, 1)):
        got = (start[0].clone(), offset(start[1], m_off * unit), offset(start[2], v_off * unit))
        adam(ce, rule, got[0], ids, rows, got[1], got[2], bias_factor=0.7, weight_decay=0.01)
        assert same(got, want), (m_off, v_off)
    if kind == "f16":
        with pytest.raises(ValueError, match="aligned"):
            adam(ce, rule, start[0].clone(), ids, rows, offset(start[1], 1), start[2].clone())


@pytest.mark.parametrize("rule", R.RULES)
def test_lr_and_bias_factor_from_device_words(ce, oracle, rule):
    kind, width, ncat = "bf16", 128, 2000
    ids, n, _, rows, table = padded_problem(oracle, kind, width, ncat)
    rows = rows[:n].contiguous()
    lr, c = float(np.float32(0.0371)), float(np.float32(ce.adam_bias_factor(5, BETAS)))
    start = (table,) + moments(rule, ncat, width, 0.125)
    want = clones(*start)
    adam(ce, rule, want[0], ids, rows, want[1], want[2], lr=lr, bias_factor=c)
    assert not np.array_equal(bits(want[0]), bits(table))
    check_step(rule, kind, start, ids, rows, want, lr=lr, bias_factor=c)
    lr_word = torch.tensor([lr], dtype=torch.float32, device="cuda")
    c_word = torch.tensor([c], dtype=torch.float32, device="cuda")
    for kw in (dict(lr=lr_word, bias_factor=c), dict(lr=lr, bias_factor=c_word), dict(lr=lr_word, bias_factor=c_word)):
        got = clones(*start)
        adam(ce, rule, got[0], ids, rows, got[1], got[2], **kw)
        assert same(got, want), sorted(kw)


# ---- the clock ---------------------------------------------------------------------------------------------------------
def test_clock_after_200_advances(ce):
    betas = (0.9, 0.999)
    powers, c = ce.new_adam_clock("cuda")
    seen = []
    for t in range(1, 201):
        ce.adam_clock_advance(powers, c, betas)
        if t in (1, 2, 10, 200):
            seen.append((t, powers.cpu().numpy().copy(), float(c.item())))
    for t, p, got in seen:
        assert p[0] == t
        assert abs(p[1] - betas[0] ** t) <= 1e-12 * betas[0] ** t and abs(p[2] - betas[1] ** t) <= 1e-12 * betas[1] ** t
        want = np.float32(ce.adam_bias_factor(t, betas))
        assert np.nextafter(want, np.float32(0)) <= np.float32(got) <= np.nextafter(want, np.float32(2)), (t, got, want)


@pytest.mark.parametrize("bias_correction", [True, False])
@pytest.mark.parametrize("rule", R.RULES)
def test_updater_apply_reads_the_clock(ce, oracle, rule, bias_correction):
    """SparseAdamUpdater.apply advances the clock and updates with its word: the same bits as ops.sparse_row_adam given
    float(bias_factor) (1.0 without bias correction), three steps."""
    from cuembed_amd import optim
    kind, width, ncat = "f16", 64, 2000
    ids, n, pad_ids, rows, table = padded_problem(oracle, kind, width, ncat)
    word = torch.tensor([n], dtype=torch.int64, device="cuda")
    up = optim.SparseAdamUpdater(table.clone(), LR, betas=BETAS, eps=EPS, weight_decay=0.01, rowwise=rule == "rowwise_adam",
                                 bias_correction=bias_correction)
    want = (table.clone(),) + moments(rule, ncat, width)
    for t in (1, 2, 3):
        up.apply(pad_ids, rows, count=word)
        c = float(up.bias_factor.item())
        assert abs(c - ce.adam_bias_factor(t, BETAS)) <= 2.0 ** -23 * c and float(up.powers[0].item()) == t
        adam(ce, rule, want[0], pad_ids, rows, want[1], want[2], count=word, weight_decay=0.01,
             bias_factor=c if bias_correction else 1.0)
        assert same((up.table, up.exp_avg, up.exp_avg_sq), want), t
    assert not np.array_equal(bits(up.table), bits(table))


# ---- SparseAdamUpdater: the whole backward + update without a read-back -----------------------------------------------
def _reference_step(ce, rule, state, gy, idx, offsets, weights, **kw):
    """embedding_backward (compressed, HOST-known count) followed by ops.sparse_row_adam: what backward_and_apply must
    equal bit for bit."""
    table = state[0]
    ncat = table.shape[0]
    if offsets is None:
        t_idx, t_sid, t_w, remap = ce.transpose_fixed_hotness(idx, idx.shape[0], idx.shape[1], weights,
                                                              num_categories=ncat, remapped=True)
    else:
        sid = ce.extract_row_ids_from_csr(offsets, nnz=idx.numel(), dtype=idx.dtype)
        t_idx, t_sid, t_w, remap = ce.transpose(sid, idx, weights, num_categories=ncat, remapped=True)
    nu = int(remap[-1].item()) + 1
    rows, ids = ce.embedding_backward(gy, nu, t_idx, t_sid, remap, t_w)
    before = clones(*state)
    adam(ce, rule, table, ids, rows, state[1], state[2], count=nu, **kw)
    return before, ids, rows


@pytest.mark.parametrize("layout", ["fixed", "csr"])
@pytest.mark.parametrize("rule", R.RULES)
def test_backward_and_apply_equals_backward_plus_sparse_row_adam(ce, oracle, rule, layout):
    """(Integer-valued gradients and weights: a run that crosses workgroups arrives through atomics in any order, so
    two backward calls only agree bit for bit where every sum is exact.)"""
    from cuembed_amd import optim
    kind, ncat, width, batch = "f16", 5000, 64, 700
    if layout == "fixed":
        idx = torch.from_numpy(oracle.generate_indices(ncat, batch, 8, alpha=1.15).astype(np.int32)).cuda().view(batch, 8)
        offsets = weights = None
    else:
        lengths = torch.randint(0, 12, (batch,))
        offsets = torch.cat([torch.zeros(1, dtype=torch.int64), lengths.cumsum(0)]).to(torch.int32).cuda()
        nnz = int(lengths.sum())
        idx = torch.from_numpy(oracle.generate_indices(ncat, nnz, 1, alpha=1.15)[:nnz].astype(np.int32)).cuda()
        weights = torch.randint(1, 3, (nnz,), device="cuda").to(TORCH[kind])
    gy = torch.randint(-3, 4, (batch, width), device="cuda").to(TORCH[kind])
    table = (torch.rand((ncat, width), device="cuda") * 2 - 1).to(TORCH[kind])
    ce.capacity_overflowed(reset=True)      # (the word is sticky and process-wide: other tests raise it on purpose)
    up = optim.SparseAdamUpdater(table.clone(), LR, betas=BETAS, eps=EPS, weight_decay=0.01, rowwise=rule == "rowwise_adam")
    for _ in range(2):                      # (the second call reuses the object's buffers)
        up.backward_and_apply(gy, idx, offsets, weights)
    want = (table.clone(),) + moments(rule, ncat, width)
    for t in (1, 2):
        c = float(np.float32(ce.adam_bias_factor(t, BETAS)))
        before, ids, rows = _reference_step(ce, rule, want, gy, idx, offsets, weights, bias_factor=c, weight_decay=0.01)
        check_step(rule, kind, before, ids, rows, want, bias_factor=c, weight_decay=0.01)
    assert same((up.table, up.exp_avg, up.exp_avg_sq), want)
    assert not ce.capacity_overflowed()


@pytest.mark.parametrize("rule", R.RULES)
def test_step_under_hip_graph_capture(ce, oracle, rule):
    """forward + backward_and_apply captured on a side stream (straight-line work only) and replayed three times with new
    indices in the same buffers: bit-identical to the eager sequence, so the clock advanced inside the graph."""
    from cuembed_amd import optim
    ncat, W, B, H = 5000, 64, 512, 16
    table0 = torch.from_numpy(oracle.allocate_forward(ncat, W, B, H, alpha=1.15)["table"]).cuda()
    batches = [torch.from_numpy(oracle.generate_indices(ncat, B, H, alpha=al)).cuda().view(B, H)
               for al in (1.15, 0.0, 1.05, 1.3)]
    gy = torch.from_numpy(oracle.allocate_grad_y(B * W).reshape(B, W)).cuda()

    def run(captured):
        idx = batches[0].clone()
        out = torch.empty((B, W), device="cuda")
        up = optim.SparseAdamUpdater(table0.clone(), LR, betas=BETAS, eps=EPS, weight_decay=0.01,
                                     rowwise=rule == "rowwise_adam")
        outs, factors = [], []

        def step():
            ce.embedding_forward(up.table, idx.view(-1), num_hots=H, out=out)
            up.backward_and_apply(gy, idx)

        if not captured:
            for b in batches:
                idx.copy_(b)
                step()
                outs.append(out.clone())
                factors.append(up.bias_factor.clone())
            torch.cuda.synchronize()
            return up, outs, factors
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            step()                               # warm-up outside capture: this is step 1 of the sequence
            outs.append(out.clone())
            factors.append(up.bias_factor.clone())
            torch.cuda.current_stream().synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                step()
        torch.cuda.synchronize()
        # the capture itself ran nothing; replay steps 2..4
        for b in batches[1:]:
            idx.copy_(b)
            g.replay()
            outs.append(out.clone())
            factors.append(up.bias_factor.clone())
        torch.cuda.synchronize()
        return up, outs, factors

    eager, eager_outs, eager_c = run(False)
    graph, graph_outs, graph_c = run(True)
    assert float(eager.powers[0].item()) == 4.0 and float(graph.powers[0].item()) == 4.0
    assert same((graph.table, graph.exp_avg, graph.exp_avg_sq, graph.powers.view(torch.int32)),
                (eager.table, eager.exp_avg, eager.exp_avg_sq, eager.powers.view(torch.int32)))
    assert not np.array_equal(bits(eager.table), bits(table0))
    for a, b in zip(eager_outs + eager_c, graph_outs + graph_c):
        assert np.array_equal(bits(a), bits(b))
    assert len({float(c.item()) for c in graph_c}) == 4          # four different steps


def test_exchange_result_apply_to(ce):
    """SparseGradResult.apply_to feeds (ids, rows, counts, piece) to SparseAdamUpdater.apply."""
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
    up = optim.SparseAdamUpdater(table.clone(), LR, rowwise=True)
    result.apply_to(up)
    valid = torch.cat([torch.arange(r * piece, r * piece + counts[r]) for r in range(world)]).cuda()
    ids = tail[:, :piece].reshape(-1)[valid]
    check_step("rowwise_adam", "f32", (table,) + moments("rowwise_adam", ncat, width), ids, rows[valid],
               (up.table, up.exp_avg, up.exp_avg_sq), bias_factor=float(up.bias_factor.item()))


# ---- stochastic rounding: the fp32 value from the kernel on an fp32 twin --------------------------------------------------
SEED = 0xC0FFEE1234567
SR_KIND = {"fp16": "f16", "bf16": "bf16"}


def pat(t):
    return t.detach().contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


@pytest.mark.parametrize("width", [8, 50, 256, 1000, 2056])
@pytest.mark.parametrize("kind", ["fp16", "bf16"])
@pytest.mark.parametrize("rule", R.RULES)
def test_stochastic_rounding_equals_the_rounded_fp32_twin(ce, rule, kind, width):
    """The rule on an fp32 copy of the same stored values stores the fp32 value x that the 16-bit kernel rounds; x pushed
    through the rounding rule with the Philox fields of (seed, step, row, column) must be the 16-bit table, and the
    moments must be those of the round-to-nearest run.  (Row-wise: gradients of +-{2^-3, 2^-4, 2^-5}, whose sum of
    squares is exact in any summation order: the twin's lanes hold 4 elements, the 16-bit table's 8.)"""
    ncat, entries = 300, 37          # an odd count: one group's second in-flight entry is dead
    rng = np.random.default_rng(1000 * width + 1)
    table = S.nearest(rng.standard_normal((ncat, width)).astype(np.float32), kind)
    if rule == "adam":
        grad = rng.standard_normal((entries, width))
    else:
        grad = rng.choice([2.0 ** -3, 2.0 ** -4, 2.0 ** -5], size=(entries, width)) * rng.choice([-1.0, 1.0], size=(entries, width))
    grad = S.nearest(grad.astype(np.float32), kind)
    ids = rng.permutation(ncat)[:entries].astype(np.int64)
    d_ids = torch.from_numpy(ids).cuda()
    dt = TORCH[SR_KIND[kind]]
    t = torch.from_numpy(np.ascontiguousarray(table).view(np.int16)).view(dt).cuda()
    g = torch.from_numpy(np.ascontiguousarray(grad).view(np.int16)).view(dt).cuda()
    m0 = torch.from_numpy((rng.random((ncat, width)) * 0.5 - 0.25).astype(np.float32)).cuda()
    v0 = torch.from_numpy((rng.random((ncat, width) if rule == "adam" else (ncat,)) * 0.5 + 0.125).astype(np.float32)).cuda()
    kw = dict(lr=0.0371, bias_factor=0.61, weight_decay=0.01)
    near = clones(t, m0, v0)
    adam(ce, rule, near[0], d_ids, g, near[1], near[2], **kw)
    twin = (t.float(), m0.clone(), v0.clone())
    adam(ce, rule, twin[0], d_ids, g.float(), twin[1], twin[2], **kw)
    x = twin[0].cpu().numpy()
    assert np.array_equal(pat(near[0]), S.nearest(x, kind))                     # (the twin is a twin)
    sr = clones(t, m0, v0)
    adam(ce, rule, sr[0], d_ids, g, sr[1], sr[2], stochastic_rounding=True, seed=SEED, step=9, **kw)
    fields = S.fields(SEED, 9, ids, width)
    want = table.copy()
    want[ids] = ce.stochastic_round_array(dt, torch.from_numpy(x[ids]).reshape(-1),
                                          torch.from_numpy(fields.astype(np.int32)).reshape(-1)).numpy().reshape(entries, width)
    got = pat(sr[0])
    assert np.array_equal(got, want)
    assert np.array_equal(want[ids], S.stochastic(x[ids], fields, kind))           # (the library's rule is the reference's)
    assert same(sr[1:], near[1:]) and same(sr[1:], twin[1:])
    assert not np.array_equal(bits(sr[1]), bits(m0))
    assert (got[ids] != S.nearest(x[ids], kind)).any()
    # the step from a device word; another step draws other bits
    again = clones(t, m0, v0)
    adam(ce, rule, again[0], d_ids, g, again[1], again[2], stochastic_rounding=True, seed=SEED,
         step=torch.tensor([9], dtype=torch.int64, device="cuda"), **kw)
    assert np.array_equal(pat(again[0]), want)
    other = clones(t, m0, v0)
    adam(ce, rule, other[0], d_ids, g, other[1], other[2], stochastic_rounding=True, seed=SEED, step=10, **kw)
    assert not np.array_equal(pat(other[0]), want)


def test_updater_with_stochastic_rounding_advances_its_step(ce):
    from cuembed_amd import optim
    table = (torch.rand((200, 64), device="cuda") * 2 - 1).half()
    ids = torch.randperm(200, device="cuda")[:50]
    rows = (torch.rand((50, 64), device="cuda") * 2 - 1).half()
    up = optim.SparseAdamUpdater(table.clone(), LR, stochastic_rounding=True, seed=SEED)
    want = (table.clone(),) + moments("adam", 200, 64)
    for t in (1, 2):
        up.apply(ids, rows)
        adam(ce, "adam", want[0], ids, rows, want[1], want[2], bias_factor=float(up.bias_factor.item()),
             stochastic_rounding=True, seed=SEED, step=t - 1)
        assert same((up.table, up.exp_avg, up.exp_avg_sq), want)
    assert int(up.rounding_step.item()) == 2


# ---- torch.optim front ends ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["f32", "f16"])
@pytest.mark.parametrize("rule", R.RULES)
def test_optimizers_after_a_sparse_backward(ce, rule, kind):
    """SparseAdam / RowwiseAdam on the gradient of cuemb_embedding(..., sparse_grad=True), three steps against the
    reference; then state_dict() -> a new optimizer -> the same next step."""
    from cuembed_amd import cuembed_pyt as P
    from cuembed_amd import optim
    ncat, width, batch, hot = 4000, 64, 300, 6
    w = torch.nn.Parameter((torch.rand((ncat, width), device="cuda") * 2 - 1).to(TORCH[kind]))
    idx = (torch.rand((batch * hot,), device="cuda") ** 3 * ncat).long().clamp_(max=ncat - 1)
    off = torch.arange(0, batch * hot + 1, hot, device="cuda")
    scale = (torch.rand((batch, width), device="cuda") * 2 - 1).to(TORCH[kind])

    def backward():
        w.grad = None
        (P.cuemb_embedding(w, idx, off, sparse_grad=True) * scale).sum().backward()
        assert w.grad.is_sparse

    cls = optim.SparseAdam if rule == "adam" else optim.RowwiseAdam
    opt = cls([w], lr=LR, betas=BETAS, eps=EPS, weight_decay=0.01)
    for t in (1, 2, 3):
        backward()
        g = w.grad
        ids, rows = g._indices()[0].clone(), g._values().clone()
        st = opt.state[w]
        before = clones(w.detach(), st["exp_avg"], st["exp_avg_sq"])
        opt.step()
        assert st["step"] == t
        c = ce.adam_bias_factor(t, BETAS)
        check_step(rule, kind, before, ids, rows, (w.detach(), st["exp_avg"], st["exp_avg_sq"]), bias_factor=c,
                   weight_decay=0.01)
    # state_dict() -> a new optimizer -> the same next step
    backward()
    twin_w = torch.nn.Parameter(w.detach().clone())
    twin_w.grad = torch.sparse_coo_tensor(w.grad._indices().clone(), w.grad._values().clone(), size=w.grad.shape,
                                          is_coalesced=True)
    twin = cls([twin_w], lr=0.5)
    twin.load_state_dict(opt.state_dict())
    opt.step()
    twin.step()
    assert np.array_equal(bits(twin_w), bits(w)) and twin.state[twin_w]["step"] == 4
    for key in ("exp_avg", "exp_avg_sq"):
        assert np.array_equal(bits(twin.state[twin_w][key]), bits(opt.state[w][key]))
        assert twin.state[twin_w][key].dtype == torch.float32


def test_optimizers_reject_an_uncoalesced_gradient_on_the_gpu(ce):
    from cuembed_amd import optim
    w = torch.nn.Parameter(torch.rand((3000, 32), device="cuda"))
    w.grad = torch.sparse_coo_tensor(torch.tensor([[5, 5, 9]], device="cuda"), torch.ones((3, 32), device="cuda"),
                                     size=(3000, 32))
    before = w.detach().clone()
    opt = optim.SparseAdam([w], lr=0.1)
    with pytest.raises(ValueError, match="COALESCED"):
        opt.step()
    assert torch.equal(w.detach(), before) and opt.state[w]["step"] == 0


# ---- the torch op ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", R.RULES)
def test_torch_op_eager_and_compiled(ce, oracle, rule):
    from cuembed_amd import cuembed_pyt as P
    kind, width, ncat = "f16", 64, 2000
    rowwise = rule == "rowwise_adam"
    ids, n, pad_ids, rows, table = padded_problem(oracle, kind, width, ncat)
    word = torch.tensor([n], dtype=torch.int32, device="cuda")
    c_word = torch.tensor([0.4], dtype=torch.float32, device="cuda")
    start = (table,) + moments(rule, ncat, width, 0.25)
    want = clones(*start)
    adam(ce, rule, want[0], pad_ids, rows, want[1], want[2], count=word, bias_factor=c_word, weight_decay=0.01)
    assert not np.array_equal(bits(want[0]), bits(table))
    op = clones(*start)
    P.cuembed_sparse_row_adam_(op[0], pad_ids, rows, exp_avg=op[1], exp_avg_sq=op[2], lr=LR, bias_factor=c_word,
                               betas=BETAS, eps=EPS, weight_decay=0.01, rowwise=rowwise, count=word)
    assert same(op, want)
    sr_want, sr_op = clones(*start), clones(*start)
    adam(ce, rule, sr_want[0], pad_ids, rows, sr_want[1], sr_want[2], count=n, stochastic_rounding=True, seed=SEED, step=3)
    P.cuembed_sparse_row_adam_(sr_op[0], pad_ids, rows, exp_avg=sr_op[1], exp_avg_sq=sr_op[2], lr=LR, betas=BETAS, eps=EPS,
                               rowwise=rowwise, count=n, stochastic_rounding=True, seed=SEED, step=3)
    assert same(sr_op, sr_want) and not np.array_equal(bits(sr_want[0]), bits(want[0]))

    def fn(t, m, v, i, r, c, b):
        torch.ops.cuembed_pyt.cuembed_sparse_row_adam_(t, m, v, i, r, rowwise, LR, 1.0, BETAS[0], BETAS[1], EPS, 0.01, None,
                                                       b, -1, c, None, 0)
        return t + 0

    comp = clones(*start)
    try:
        got = torch.compile(fn, fullgraph=True)(comp[0], comp[1], comp[2], pad_ids, rows, word, c_word)
    except Exception as e:  # noqa: BLE001 - no working inductor toolchain on the box: trace with aot_eager instead
        print("inductor unavailable (%s): aot_eager" % type(e).__name__)
        torch._dynamo.reset()
        comp = clones(*start)
        got = torch.compile(fn, fullgraph=True, backend="aot_eager")(comp[0], comp[1], comp[2], pad_ids, rows, word, c_word)
    assert same(comp, want) and np.array_equal(bits(got), bits(want[0]))


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
for rowwise in (False, True):
    a_t, b_t = table.clone(), table.clone()
    a_m, b_m = torch.zeros((500, 32), device="cuda"), torch.zeros((500, 32), device="cuda")
    shape = (500,) if rowwise else (500, 32)
    a_v, b_v = torch.zeros(shape, device="cuda"), torch.zeros(shape, device="cuda")
    ce.sparse_row_adam(a_t, ids, rows, exp_avg=a_m, exp_avg_sq=a_v, lr=0.05, bias_factor=0.3, rowwise=rowwise, count=word)
    P.cuembed_sparse_row_adam_(b_t, ids, rows, exp_avg=b_m, exp_avg_sq=b_v, lr=0.05, bias_factor=0.3, rowwise=rowwise,
                               count=word)
    assert torch.equal(a_t, b_t) and not torch.equal(a_t, table), rowwise
    assert torch.equal(a_m, b_m) and torch.equal(a_v, b_v) and float(a_v.max()) > 0, rowwise
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
