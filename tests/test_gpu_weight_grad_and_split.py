"""The weight gradient and the split forward on arbitrary data against fp64, and IEEE edge values through the
bit-exact forward branches.

* embedding_weight_grad: an fp32 dot product per lookup (16-bit tables: v_dot2_f32_f16 / v_dot2_f32_bf16), rounded
  once: |got - exact| <= EPS_out * |exact| + W * 2^-24 * sum |t * g| + floor -- with fp16 grad_y of ~2^-20 (subnormal
  inputs: a packed dot that flushes them returns 0) too.
* set_forward_reduction_order("split"): fp32 partial pooled rows per wave (cross-lane folds + LDS), rounded once;
  the bound is per element, relative to that element's sum |terms| (tests/exact_sums.py).
* The bit-exact forward branches (LDS-staged, wave-shuffle and global index sources, wide load with one and with
  several samples, concat, non-temporal row loads) on tables holding +-0, +-inf, NaN, subnormals, rows whose fp32 sum
  overflows the output type and fp32 sums exactly halfway between two 16-bit values: the oracle's bits (NaN as NaN).
"""
import numpy as np
import pytest
import torch

import exact_sums as X

pytestmark = pytest.mark.gpu

TORCH = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}


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


def raw_bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32).cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("W", [8, 36, 64, 256, 1024])
def test_weight_grad_within_fp64_bound(ce, oracle, kind, W):
    """W = 8: two lanes per row (the fallback walk), 36: a masked lane group, 256 / 1024: rows wider than a wave.
    Fixed hotness and CSR with an empty bag; fp16 also with grad_y ~ 2^-20 (subnormal)."""
    rng = np.random.default_rng(40 + W)
    ncat, B, H = 3_000, 700, 9
    _, table_d, table64 = elem(oracle, kind, rng.uniform(0.0, 1.0, (ncat, W)).astype(np.float32))
    lens = rng.integers(0, 2 * H, B)
    lens[5] = 0
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    regimes = [1.0, 2.0 ** -20] if kind == "f16" else [1.0]
    for n_reg, magnitude in enumerate(regimes):
        _, gy_d, gy64 = elem(oracle, kind, (rng.uniform(-1, 1, (B, W)) * magnitude).astype(np.float32))
        if magnitude < 1:
            assert np.all(np.abs(gy64) < 2.0 ** -14) and np.mean(gy64 != 0) > 0.95     # (below 2^-25: 0)
        for csr in (False, True):
            idx_t = np.int64 if (csr ^ bool(n_reg)) else np.int32
            if csr:
                idx = rng.integers(0, ncat, int(off[-1])).astype(idx_t)
                got = ce.embedding_weight_grad(table_d, dev(idx), gy_d, offsets=dev(off.astype(idx_t)))
                sample = np.repeat(np.arange(B), lens)
            else:
                idx = rng.integers(0, ncat, B * H).astype(idx_t)
                got = ce.embedding_weight_grad(table_d, dev(idx), gy_d, num_hots=H)
                sample = np.repeat(np.arange(B), H)
            exact, scale = X.weight_grad(table64, idx, gy64, sample)
            bound = X.weight_grad_bound(kind, W, exact, scale)
            g = host64(oracle, kind, got)
            worst = int(np.argmax(np.abs(g - exact) - bound))
            assert np.all(np.abs(g - exact) <= bound), (magnitude, csr, worst, g[worst], exact[worst], bound[worst])
            if magnitude < 1:               # the products of subnormal grads are not lost: no result above 2^-24 is 0
                assert np.all(g[np.abs(exact) > 2.0 ** -24] != 0)


# ---------------------------------------------------------------------------------------------------------------------
def _split_taken(ce, kind, idx_t, W, B, H, csr, weighted):
    """LaunchGatherReduce's condition for GatherReduceSplitKernel under the "split" order."""
    s = ce.forward_launch_shape(TORCH[kind], idx_t, W, B, H, csr, weighted, "sum")
    lanes = s["lanes_per_row"]
    fits = (lanes <= 64 and 64 % lanes == 0) or lanes == 128
    return fits and B * lanes // 64 < 2048 and (csr or H >= 8)


@pytest.mark.parametrize("kind,fp16_math", [("f32", False), ("f16", False), ("bf16", False), ("f16", True)],
                         ids=["f32", "f16", "bf16", "f16-fp16math"])
@pytest.mark.parametrize("W", [8, 64, 256, 1024])
def test_split_forward_per_element_bound(ce, oracle, kind, fp16_math, W):
    if kind == "f32" and W == 1024:
        W = 512                         # (4 KiB rows take 256 lanes: not a split launch)
    rng = np.random.default_rng(60 + W)
    ncat, B, H = 2_000, 37, 61
    t_o, t_d, t64 = elem(oracle, kind, rng.uniform(-1, 1, (ncat, W)).astype(np.float32))
    idx = rng.integers(0, ncat, B * H).astype(np.int32)
    w_o, w_d, w64 = elem(oracle, kind, rng.uniform(0, 1, 2 * B * H).astype(np.float32))   # (enough for the CSR batch)
    lens = rng.integers(0, 2 * H, B)
    lens[3] = 0
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    idx_csr = rng.integers(0, ncat, int(off[-1])).astype(np.int64)
    fixed_off = np.arange(0, B * H + 1, H)
    assert ce.get_forward_reduction_order() == "sequential"
    ce.set_forward_reduction_order("split")
    try:
        for mode, weighted in [("sum", False), ("mean", False), ("mean", True), ("sum", True)]:
            for csr in (False, True):
                ids, o = (idx_csr, off) if csr else (idx, fixed_off)
                wo = w_o[:ids.shape[0]] if weighted else None
                wd = w_d[:ids.shape[0]] if weighted else None
                ww = w64[:ids.shape[0]] if weighted else None
                assert _split_taken(ce, kind, torch.int64 if csr else torch.int32, W, B, H, csr, weighted)
                got = ce.embedding_forward(t_d, dev(ids), dev(o) if csr else None, wd, num_hots=0 if csr else H,
                                           mode=mode, fp16_math=fp16_math)
                g = host64(oracle, kind, got)
                exact, scale, hot = X.forward(t64, ids, o, ww, mean=mode == "mean")
                want = oracle.embedding_forward(t_o, ids, o if csr else None, wo, num_hots=0 if csr else H, mode=mode,
                                                fp16_math=fp16_math)
                ora = oracle.from_bf16_bits(want).astype(np.float64) if kind == "bf16" else want.astype(np.float64)
                X.assert_split_forward_within_bound(kind, fp16_math, g, exact, scale, hot, ora, mode == "mean",
                                                    (mode, weighted, csr))
    finally:
        ce.set_forward_reduction_order("sequential")
    assert ce.get_forward_reduction_order() == "sequential"


# ---------------------------------------------------------------------------------------------------------------------
def _edge_table(rng, kind, rows, W):
    """A table of edge values of `kind` (as fp32 values exactly representable in it) plus ordinary rows."""
    if kind == "f16":
        sub, big, step = 2.0 ** -24, 60000.0, 2.0 ** -10       # smallest subnormal, near max, ulp at 1
    elif kind == "bf16":
        sub, big, step = 2.0 ** -133, 3.0e38, 2.0 ** -7
    else:
        sub, big, step = 2.0 ** -149, 3.0e38, 2.0 ** -23
    specials = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, sub, -sub, 3 * sub, 1000 * sub, big, -big,
                         1.0, step / 2, 1.0 + step, -1.0, 0.5], dtype=np.float64)
    t = rng.uniform(-1, 1, (rows, W))
    t[: rows // 2] = specials[rng.integers(0, specials.shape[0], (rows // 2, W))]
    return t.astype(np.float32)


def _to(kind, oracle, t32):
    if kind == "f32":
        return t32, dev(t32)
    if kind == "f16":
        h = t32.astype(np.float16)
        return h, dev(h)
    b = oracle.to_bf16_bits(t32)
    return b, dev(b.view(np.int16)).view(torch.bfloat16)


def _same(got_t, want, label):
    """bit for bit, except that any NaN equals any NaN"""
    g = raw_bits(got_t).reshape(want.shape)
    w = np.ascontiguousarray(want).view(g.dtype)
    if want.dtype == np.uint16:                                     # bf16 bits
        nan_g = (g.view(np.uint16) & 0x7fff) > 0x7f80
        nan_w = (w.view(np.uint16) & 0x7fff) > 0x7f80
    else:
        nan_g = np.isnan(g.view(want.dtype))
        nan_w = np.isnan(want)
    assert np.array_equal(nan_g, nan_w), label
    assert np.array_equal(g[~nan_g], w[~nan_w]), label


@pytest.mark.parametrize("kind", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("W", [64, 36], ids=["W64", "W36"])
def test_ieee_edge_values_through_the_bit_exact_forward_branches(ce, oracle, kind, W):
    """W = 64: LDS-staged (fixed hotness) and wave-shuffle (CSR) index sources; W = 36: lane groups that do not
    divide a wave -- the global index source."""
    rng = np.random.default_rng(90 + W)
    ncat = 512
    t32 = _edge_table(rng, kind, ncat, W)
    # rows whose fp32 sum is exactly halfway between two 16-bit values: 1 + half an ulp of the element type, made of
    # two representable halves (1 and ulp / 2); rows whose sum overflows the element type (big + big)
    neg0, zero_row, half_row, tie_row, over_row = ncat - 5, ncat - 4, ncat - 3, ncat - 2, ncat - 1
    step = {"f16": 2.0 ** -10, "bf16": 2.0 ** -7, "f32": 2.0 ** -23}[kind]
    big = {"f16": 60000.0, "bf16": 3.0e38, "f32": 3.0e38}[kind]
    t32[neg0] = -0.0
    t32[zero_row] = 0.0
    t32[half_row] = 1.0
    t32[tie_row] = step / 2
    t32[over_row] = big
    t_o, t_d = _to(kind, oracle, t32)
    w_o, w_d = _to(kind, oracle, rng.choice([0.5, 1.0, 0.25, -1.0], 4096).astype(np.float32))
    B, H = 48, 8
    idx = rng.integers(0, ncat, B * H).astype(np.int32)
    idx[:H] = [half_row, tie_row] + [zero_row] * (H - 2)          # sample 0: exactly 1 + ulp / 2
    idx[H:2 * H] = [over_row, over_row] + [zero_row] * (H - 2)    # sample 1: overflows; the others: edge rows
    cases = []
    for csr in (False, True):
        for wide in ("never", "always", "always4"):
            for rl in (None, "streaming"):
                cases.append((csr, wide, rl))
    # a weighted mean whose weights sum to exactly 0, and a bag of one lookup of -0.0
    zero_w = np.array([0.5, -0.5, 1.0, -1.0] * 2, dtype=np.float32)
    try:
        for csr, wide, rl in cases:
            ce.set_forward_wide_load(wide)
            for W_idx_t in (np.int32, np.int64):
                ids = idx.astype(W_idx_t)
                off = np.arange(0, B * H + 1, H).astype(W_idx_t)
                for mode, weighted in (("sum", False), ("sum", True), ("mean", False), ("mean", True)):
                    wo = w_o[:ids.shape[0]] if weighted else None
                    wd = w_d[:ids.shape[0]] if weighted else None
                    want = oracle.embedding_forward(t_o, ids, off if csr else None, wo, num_hots=0 if csr else H,
                                                    mode=mode)
                    got = ce.embedding_forward(t_d, dev(ids), dev(off) if csr else None, wd,
                                               num_hots=0 if csr else H, mode=mode, row_loads=rl)
                    _same(got, want, (csr, wide, rl, W_idx_t, mode, weighted))
            if not csr:    # concat
                want = oracle.embedding_forward(t_o, idx, None, None, num_hots=H, mode="concat")
                got = ce.embedding_forward(t_d, dev(idx), None, None, num_hots=H, mode="concat", row_loads=rl)
                _same(got.reshape(-1, W), want, ("concat", wide, rl))
            # weights that sum to exactly 0 (mean) and a single lookup of -0.0 (the oracle adds to +0)
            zi = idx[:8].copy()
            zw_o, zw_d = _to(kind, oracle, zero_w)
            zoff = np.array([0, 8], dtype=np.int32)
            want = oracle.embedding_forward(t_o, zi, zoff if csr else None, zw_o, num_hots=0 if csr else 8, mode="mean")
            got = ce.embedding_forward(t_d, dev(zi), dev(zoff) if csr else None, zw_d, num_hots=0 if csr else 8,
                                       mode="mean", row_loads=rl)
            _same(got, want, ("zero weight sum", csr, wide, rl))
            one = np.array([neg0], dtype=np.int32)
            want = oracle.embedding_forward(t_o, one, np.array([0, 1], np.int32) if csr else None, None,
                                            num_hots=0 if csr else 1)
            got = ce.embedding_forward(t_d, dev(one), dev(np.array([0, 1], np.int32)) if csr else None, None,
                                       num_hots=0 if csr else 1, row_loads=rl)
            _same(got, want, ("-0.0", csr, wide, rl))
            assert not np.any(np.signbit(host64(oracle, kind, got)))          # +0, like the oracle
    finally:
        ce.set_forward_wide_load("auto")
