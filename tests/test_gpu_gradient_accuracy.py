"""EmbeddingBackward on arbitrary data against exact fp64 sums, for every mapping a user can select.

The backward keeps fp32 partial sums and rounds to the gradient's type once per flush (tests/exact_sums.py): a run
inside one workgroup is the correctly rounded fp32 sum, a run across workgroups arrives through one hardware atomic
per workgroup.  Integer test data (the bit-exact tests) cannot see a partial rounded to 16 bits too often, a weight
applied at 16-bit precision or a flushed subnormal; here grads are U(-1, 1) and weights U(0, 1) (fixed seeds), and
every element must satisfy |got - exact| <= error_bound, with the rounding count derived from backward_launch_shape.
For 16-bit types the design's own claim is asserted too: its max and RMS error are no larger than the reference
arithmetic's (the oracle: the running sum rounded to the gradient's type at every lookup).

Regimes: "unit" (U(-1, 1)); "small" (fp16, grads * 2^-20: every input is subnormal, the 60,000-lookup run's sum
leaves the subnormal range while its per-workgroup partials reach the 16-bit atomics as subnormals); "large" (fp16,
values near +-2^15 whose prefix sums exceed 65504 inside a run: rows whose exact sum fits must come out finite and
within the bound -- where the oracle's per-lookup fp16 sum already gives inf -- rows beyond 65520 must be +-inf).
"""
import numpy as np
import pytest
import torch

import exact_sums as X

pytestmark = pytest.mark.gpu

TORCH = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
KINDS = ["f32", "f16", "bf16"]


@pytest.fixture(scope="module")
def ce():
    import cuembed_amd
    assert torch.cuda.is_available()
    return cuembed_amd


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def elem(oracle, kind, a32):
    """fp32 values -> (the oracle's array, device tensor, exact fp64 values of the rounded elements)."""
    if kind == "f32":
        a = np.ascontiguousarray(a32, dtype=np.float32)
        return a, dev(a), a.astype(np.float64)
    if kind == "f16":
        h = np.ascontiguousarray(a32).astype(np.float16)
        return h, dev(h), h.astype(np.float64)
    b = oracle.to_bf16_bits(a32)
    return b, dev(b.view(np.int16)).view(torch.bfloat16), oracle.from_bf16_bits(b).astype(np.float64)


def host64(oracle, kind, t):
    if kind == "bf16":
        return oracle.from_bf16_bits(t.view(torch.int16).cpu().numpy().view(np.uint16)).astype(np.float64)
    return t.cpu().numpy().astype(np.float64)


def oracle64(oracle, kind, a):
    return oracle.from_bf16_bits(a).astype(np.float64) if kind == "bf16" else a.astype(np.float64)


def _coo(oracle, rng, ncat, B, H, alpha, csr, idx_t, long_run=0):
    """Index-sorted COO (stable transpose) of a fixed-hotness or CSR batch; long_run > 0 plants one row looked up by
    that many samples."""
    a = oracle.allocate_forward(ncat, 8, B, H, alpha=alpha, is_csr=csr)
    ids = a["indices"].astype(np.int64)
    if csr:
        off = a["offsets"].astype(np.int64)
        sid = oracle.extract_row_ids_from_csr(off, dtype=np.int64)
    else:
        sid = np.repeat(np.arange(B, dtype=np.int64), H)
    if long_run:
        first = np.unique(sid, return_index=True)[1][:long_run]       # one lookup of each of the first samples
        ids[first] = ncat - 1
    w32 = rng.uniform(0.0, 1.0, ids.shape[0]).astype(np.float32)
    ti, ts, tw = oracle.transpose(sid.astype(idx_t), ids.astype(idx_t), w32, stable=True)
    return ti, ts, tw


def _grads(rng, regime, B, W):
    g = rng.uniform(-1.0, 1.0, (B, W))
    if regime == "small":
        g = g * 2.0 ** -20
    elif regime == "large":
        g = np.sign(g) * 2.0 ** 15 * (0.875 + 0.125 * np.abs(g))
    return g.astype(np.float32)


def _shape_block(ce, kind, idx_t, W, nnz, weighted):
    s = ce.backward_launch_shape(TORCH[kind], torch.int32 if idx_t == np.int32 else torch.int64, W, nnz, weighted)
    return s["segments_per_block"] * s["segment_len"], s


def _check(kind, regime, got, ref, flushes, ora=None, label=""):
    """Every element within the bound; large regime: overflowing rows are +-inf; 16-bit: no worse than the oracle."""
    exact, scale, walk = ref["exact"], ref["scale"], ref["walk"]
    bound = X.error_bound(kind, exact, scale, walk, flushes)
    if regime == "large":
        fits = np.abs(exact) + bound < X.FP16_INF_FROM
        over = np.abs(exact) - bound >= X.FP16_INF_FROM
        one = (np.asarray(flushes) <= 1)[:, None] & np.ones_like(fits)     # partials past 65504 stay fp32 only
        assert np.all(np.abs(got - exact)[fits & one] <= bound[fits & one]), label
        assert np.all(np.isinf(got[over & one]) & (np.sign(got[over & one]) == np.sign(exact[over & one]))), label
        assert (fits & one).sum() > 100 and (over & one).sum() > 100, label
        if ora is not None:       # the reference's fp16 running sum overflows on rows whose total fits; fp32 does not
            assert np.any(np.isinf(ora) & fits & one), label
        return
    err = np.abs(got - exact)
    worst = np.unravel_index(np.argmax(err - bound), err.shape)
    assert np.all(err <= bound), (label, worst, got[worst], exact[worst], bound[worst], flushes[worst[0]])
    if ora is not None and kind != "f32":
        e_ora = np.abs(ora - exact)
        assert err.max() <= e_ora.max(), (label, err.max(), e_ora.max())
        assert np.sqrt((err ** 2).mean()) <= np.sqrt((e_ora ** 2).mean()), label


# (path, kind, W, weighted, regime): every path with every element type, with and without weights; the index type
# and the layout alternate from case to case
_PATHS = [("default", 2), ("default", 36), ("default", 256), ("default", 1024), ("slices2", 64), ("slices4", 128),
          ("seg8", 64), ("seg4096", 32), ("big", 128), ("long60k", 32)]
CASES = []
for _path, _W in _PATHS:
    for _kind in KINDS:
        if _kind != "f16" and _W == 2:
            continue                    # fp32 / bf16 rows of 2 elements: covered by W = 36's odd split
        for _weighted in (False, True):
            CASES.append((_path, _kind, _W, _weighted, "unit"))
CASES += [("long60k", "f16", 32, False, "small"), ("long60k", "f16", 32, True, "small"),
          ("default", "f16", 64, False, "small"), ("default", "f16", 36, False, "large"),
          ("default", "f16", 64, True, "large"), ("seg8", "f16", 256, False, "large")]


def _case_id(c):
    return "-".join([c[0], c[1], "W%d" % c[2], "weighted" if c[3] else "plain", c[4]])


@pytest.mark.parametrize("case", CASES, ids=[_case_id(c) for c in CASES])
def test_backward_full_and_compressed_within_fp64_bound(ce, oracle, case):
    path, kind, W, weighted, regime = case
    n_case = CASES.index(case)
    idx_t = np.int32 if n_case % 2 == 0 else np.int64
    # (the planted run needs 60,000 non-empty bags, the big case all of its 2^20 lookups)
    csr = (n_case // 2) % 2 == 1 and path not in ("long60k", "big")
    rng = np.random.default_rng(1000 + n_case)
    long_run = 0
    if path == "big":
        ncat, B, H, alpha = 200_000, 16_384, 64, 1.05          # 2^20 lookups: the column-sliced heuristics
    elif path == "long60k":
        ncat, B, H, alpha, long_run = 5_000, 61_000, 4, 1.15, 60_000
    elif regime == "large":
        ncat, B, H, alpha = 15_000, 4_000, 10, 0.0             # short runs: every prefix sum stays in fp32
    else:
        ncat, B, H, alpha = (4_000, 2_000, 16, 1.05) if W >= 256 else (20_000, 6_000, 12, 1.05)
    ti, ts, tw32 = _coo(oracle, rng, ncat, B, H, alpha, csr, idx_t, long_run)
    nnz = ti.shape[0]
    gy_o, gy_d, gy64 = elem(oracle, kind, _grads(rng, regime, B, W))
    w_o = w_d = w64 = None
    if weighted:
        w_o, w_d, w64 = elem(oracle, kind, tw32)
    tuning = {"slices2": dict(column_slices=2), "slices4": dict(column_slices=4), "seg8": dict(segment_len=8),
              "seg4096": dict(segment_len=4096)}.get(path, {})
    ce.set_backward_tuning(**tuning)
    try:
        block_len, shape = _shape_block(ce, kind, idx_t, W, nnz, weighted)
        if path == "big":
            assert nnz >= 1 << 20 and shape["column_slices"] > 1, shape
        if path.startswith("slices"):
            assert shape["column_slices"] == tuning["column_slices"], shape
        ref = X.backward(gy64, ts, ti, ncat, w64)
        flushes = X.flushes_from_shape(ti, ncat, block_len)
        if long_run:
            assert ref["run_len"].max() >= long_run
        if regime == "small":
            assert np.all(np.abs(gy64) < 2.0 ** -14)
            if long_run:
                hot = int(np.argmax(ref["run_len"]))
                assert np.mean(np.abs(ref["exact"][hot]) >= 2.0 ** -14) > 0.25        # the sum leaves the subnormals
                assert flushes[hot] > 1 and np.sqrt(block_len) * 2.0 ** -20 < 2.0 ** -14  # subnormal partials
        want, _ = oracle.embedding_backward(gy_o, W, ncat, ti, ts, None, w_o)
        ora = oracle64(oracle, kind, want)
        # full gradient
        got, _ = ce.embedding_backward(gy_d, ncat, dev(ti), dev(ts), None, w_d)
        _check(kind, regime, host64(oracle, kind, got), ref, flushes, ora, "full")
        # compressed gradient: the same rows, num_unique of them in ascending order
        remap = oracle.compute_compressed_grad_indices(ti)
        nu = int(remap[-1]) + 1
        uniq = np.unique(ti).astype(np.int64)
        sub = {k: v[uniq] for k, v in ref.items()}
        got, inv = ce.embedding_backward(gy_d, nu, dev(ti), dev(ts), dev(remap), w_d)
        assert np.array_equal(inv.cpu().numpy().astype(np.int64), uniq)
        _check(kind, regime, host64(oracle, kind, got), sub, flushes[uniq], ora[uniq], "compressed")
    finally:
        ce.set_backward_tuning(0, 0)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
def test_backward_device_count_padded_blocked_and_uncoalesced(ce, oracle, kind, weighted):
    """num_unique on the device (pad_to_capacity: padding rows exactly zero), the sample-blocked UNCOALESCED gradient
    (one row per (block, table row), densified in fp64 so that no consumer's rounding is counted) and the
    blocked-coalesced gradient (a row that an earlier block stored is read, added to and stored again)."""
    rng = np.random.default_rng(77 if weighted else 78)
    idx_t = np.int64 if weighted else np.int32
    ncat, B, H, W = 3_000, 8_000, 16, 64
    a = oracle.allocate_forward(ncat, 8, B, H, alpha=1.15)
    ids = a["indices"].astype(idx_t)
    w32 = rng.uniform(0, 1, ids.shape[0]).astype(np.float32)
    _, w_host_d, _ = elem(oracle, kind, w32)
    gy_o, gy_d, gy64 = elem(oracle, kind, _grads(rng, "unit", B, W))
    sid = np.repeat(np.arange(B, dtype=idx_t), H)
    ti, ts, tw32 = oracle.transpose(sid, ids, w32, stable=True)
    w_o = w_d = w64 = None
    if weighted:
        w_o, w_d, w64 = elem(oracle, kind, tw32)
    nnz = ti.shape[0]
    ref = X.backward(gy64, ts, ti, ncat, w64)
    block_len, _ = _shape_block(ce, kind, idx_t, W, nnz, weighted)
    flushes = X.flushes_from_shape(ti, ncat, block_len)
    want, _ = oracle.embedding_backward(gy_o, W, ncat, ti, ts, None, w_o)
    ora = oracle64(oracle, kind, want)
    uniq = np.unique(ti).astype(np.int64)
    nu = uniq.shape[0]
    sub = {k: v[uniq] for k, v in ref.items()}

    # num_unique left on the device, buffers padded to capacity
    remap = oracle.compute_compressed_grad_indices(ti)
    cap = nu + 300
    g = torch.full((cap, W), 7.0, dtype=TORCH[kind], device="cuda")
    inv = torch.full((cap,), -3, dtype=torch.int32 if idx_t == np.int32 else torch.int64, device="cuda")
    ce.embedding_backward(gy_d, None, dev(ti), dev(ts), dev(remap), w_d, grad_embedding=g, inverse_mapping=inv,
                          pad_to_capacity=True)
    g64 = host64(oracle, kind, g)
    assert np.array_equal(inv[:nu].cpu().numpy().astype(np.int64), uniq)
    _check(kind, "unit", g64[:nu], sub, flushes[uniq], ora[uniq], "device count")
    assert np.all(g64[nu:] == 0) and not np.any(np.signbit(g64[nu:])), "padding rows must be +0"
    pad_ids = inv[nu:].cpu().numpy()
    assert np.all(np.isin(pad_ids, uniq))
    # without padding: rows past the device-side count are left as they were
    g2 = torch.full((cap, W), 7.0, dtype=TORCH[kind], device="cuda")
    ce.embedding_backward(gy_d, None, dev(ti), dev(ts), dev(remap), w_d, grad_embedding=g2, inverse_mapping=inv)
    g2_64 = host64(oracle, kind, g2)
    _check(kind, "unit", g2_64[:nu], sub, flushes[uniq], ora[uniq], "device count, unpadded")
    assert np.all(g2_64[nu:] == 7.0)

    for P in (2, 3):
        L = ce.transpose_sample_block_length(nnz, P)
        t_idx, t_sid, t_w = ce.transpose_fixed_hotness(dev(ids), B, H, w_host_d if weighted else None,
                                                       num_categories=ncat, sample_blocks=P)
        t_w = t_w if weighted else None
        bi, bs = t_idx.cpu().numpy().astype(np.int64), t_sid.cpu().numpy().astype(np.int64)
        bw = host64(oracle, kind, t_w) if weighted else None
        # the blocked order holds the same lookups: its fp64 sums are the fully sorted order's
        # uncoalesced: one gradient row per (block, row), one launch over the whole order
        r = ce.compute_compressed_grad_indices(t_idx)
        n_pairs = int(r[-1].item()) + 1
        rows, pinv = ce.embedding_backward(gy_d, n_pairs, t_idx, t_sid, r, t_w)
        pinv = pinv.cpu().numpy().astype(np.int64)
        dense = np.zeros((ncat, W))
        np.add.at(dense, pinv, host64(oracle, kind, rows))
        pair_fl = X.flushes_from_shape(r.cpu().numpy(), n_pairs, block_len)
        fl = np.zeros(ncat, np.int64)
        np.add.at(fl, pinv, pair_fl)
        assert np.bincount(pinv, minlength=ncat).max() <= P
        chk = X.backward(gy64, bs, bi, ncat, bw)          # the same sums from the blocked order's own COO
        assert np.allclose(chk["exact"], ref["exact"], rtol=0, atol=1e-9 * (1 + ref["scale"].max()))
        _check(kind, "unit", dense[uniq], sub, fl[uniq], ora[uniq], "uncoalesced P=%d" % P)
        # blocked-coalesced: workgroups restart in every block of L lookups, a row's pieces add up
        pairs, table, nu_dev = ce.compute_compressed_grad_indices_blocked(t_idx, P)
        assert int(nu_dev.item()) == nu
        grad, binv = ce.embedding_backward(gy_d, nu, t_idx, t_sid, pairs, t_w, sample_blocks=P, block_row_ids=table)
        assert np.array_equal(binv.cpu().numpy().astype(np.int64), uniq)
        rank = (table.cpu().numpy().astype(np.int64) & (ce.SHARED_ROW_BIT - 1))[pairs.cpu().numpy().astype(np.int64)]
        bfl = X.flushes_from_shape(rank, nu, block_len, piece_len=L)
        assert bfl.max() >= P                # rows that several blocks add to
        _check(kind, "unit", host64(oracle, kind, grad), sub, bfl, ora[uniq], "blocked P=%d" % P)


@pytest.mark.parametrize("kind,W", [("f16", 256), ("bf16", 64), ("f32", 33), ("f16", 4)])
def test_exchange_merge_sums_arbitrary_rows(ce, kind, W):
    """ops.exchange_merge: arbitrary 16-bit (or fp32) rows, each id repeated 1-3 times, padding ids dropped"""
    from cuembed_amd import ops
    from oracle import oracle as O
    rng = np.random.default_rng(31 + W)
    num_categories, distinct = 100_000, 5_000
    pool = np.sort(rng.choice(num_categories, size=distinct, replace=False)).astype(np.int64)
    copies = rng.integers(1, 4, distinct)
    ids = np.concatenate([np.repeat(pool, copies), np.full(500, num_categories, np.int64)])
    perm = rng.permutation(ids.shape[0])
    ids = ids[perm]
    _, rows_d, rows64 = elem(O, kind, rng.uniform(-1, 1, (ids.shape[0], W)).astype(np.float32))
    capacity = distinct + 100
    out_ids = torch.zeros((capacity + 1,), dtype=torch.int64, device="cuda")
    out_rows = torch.full((capacity + 1, W), 5.0, dtype=TORCH[kind], device="cuda")
    flag = torch.zeros((1,), dtype=torch.int64, device="cuda")
    count = torch.zeros((1,), dtype=torch.int64, device="cuda")
    ops.exchange_merge(dev(ids), rows_d, num_categories, 0, 10, out_ids, out_rows, None, flag, count)
    torch.cuda.synchronize()
    assert int(count.item()) == distinct and int(flag.item()) == 0
    assert np.array_equal(out_ids.cpu().numpy()[:distinct], pool)
    keep = ids < num_categories
    order = np.argsort(ids[keep], kind="stable")
    rank = np.searchsorted(pool, ids[keep][order])
    ref = X.backward(rows64[keep][order], np.arange(order.shape[0]), rank, distinct)
    block_len, _ = _shape_block(ce, kind, np.int64, W, ids.shape[0], False)
    flushes = X.flushes_from_shape(rank, distinct, block_len)
    got = host64(O, kind, out_rows)
    _check(kind, "unit", got[:distinct], ref, flushes, None, "merge")
    assert np.all(got[distinct:] == 0)


SPARSE_KINDS = [False, True, "blocked", "uncoalesced", "padded", "fastest"]


@pytest.mark.parametrize("kind", ["f16", "bf16"])
@pytest.mark.parametrize("sparse", SPARSE_KINDS, ids=[str(s) for s in SPARSE_KINDS])
def test_torch_surface_16_bit_gradients(ce, oracle, kind, sparse):
    """cuemb_embedding with 16-bit tables: params.grad (densified) for every sparse_grad kind and, with the weights
    requiring grad, weights.grad (the weight-gradient extension) against fp64."""
    from cuembed_amd import cuembed_pyt as P
    rng = np.random.default_rng(5 + SPARSE_KINDS.index(sparse))
    ncat, B, W = 6_000, 3_000, 64
    lens = rng.integers(0, 25, B)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    nnz = int(off[-1])
    idx = (ncat * rng.random(nnz) ** 3).astype(np.int64)
    _, table_d, table64 = elem(oracle, kind, rng.uniform(-1, 1, (ncat, W)).astype(np.float32))
    _, w_d, w64 = elem(oracle, kind, rng.uniform(0, 1, nnz).astype(np.float32))
    _, gy_d, gy64 = elem(oracle, kind, _grads(rng, "unit", B, W))
    sample = np.repeat(np.arange(B), lens)
    for weight_grad in (False, True):
        params = table_d.clone().requires_grad_(True)
        weights = w_d.clone().requires_grad_(weight_grad)
        y = P.cuemb_embedding(params, dev(idx), dev(off), weights, sparse_grad=sparse)
        y.backward(gy_d)
        g = params.grad
        g = g.to_dense() if g.is_sparse else g
        order = np.argsort(idx, kind="stable")
        ref = X.backward(gy64, sample[order], idx[order], ncat, w64[order])
        # one launch over the whole order at this size (fewer than 2^20 lookups: one sample block)
        block_len, _ = _shape_block(ce, kind, np.int64, W, nnz, True)
        flushes = np.maximum(X.flushes_from_shape(idx[order], ncat, block_len),
                             X.flushes_conservative(ref["run_len"]))
        _check(kind, "unit", host64(oracle, kind, g), ref, flushes, None, "%s grad" % sparse)
        if weight_grad:
            exact, scale = X.weight_grad(table64, idx, gy64, sample)
            got = host64(oracle, kind, weights.grad)
            assert np.all(np.abs(got - exact) <= X.weight_grad_bound(kind, W, exact, scale)), sparse
