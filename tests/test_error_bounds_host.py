"""The fp64 bounds of tests/exact_sums.py are neither vacuous nor too tight (no GPU needed).

For every bound the GPU accuracy tests use, the arithmetic the design claims is simulated in numpy -- fp32 partial sums
per workgroup, one 16-bit rounding per flush, fp32 dot products, fp32 partial pooled rows -- and must PASS it; each of
the faults that integer test data cannot see must FAIL it:
  * one lookup dropped from one run;
  * the reference's arithmetic: the running sum rounded to 16 bits after every lookup, on long runs;
  * fp16 subnormal inputs flushed to zero (a packed dot or a conversion that does not honour denormals);
  * fp16 subnormal partials flushed to zero by the cross-workgroup atomics;
  * the split forward's LDS partial rows kept in the element type instead of fp32.
"""
import numpy as np
import pytest

import exact_sums as X

BLOCK = 256          # lookups per workgroup of the simulated launch


def _coo(rng, lengths, B):
    """An index-sorted COO with the given run lengths (rows 0, 2, 4, ...) and random sample ids."""
    ti = np.repeat(2 * np.arange(len(lengths)), lengths)
    ts = rng.integers(0, B, ti.shape[0])
    return ti, ts


def _lengths(rng):
    """short runs (most of them inside one workgroup), some that cross workgroups, and one of 60,000 lookups"""
    return np.concatenate([rng.integers(1, 13, 600), [300, 700, 2048], rng.integers(1, 5, 50), [60000],
                           rng.integers(1, 9, 40)])


def _design_backward(kind, gy32, ti, ts, rows, w32=None, flush_subnormal_inputs=False, flush_subnormal_atomics=False):
    """What the segmented scatter-add computes: the terms in fp32, each workgroup's piece of a run summed in fp32;
    a run inside one workgroup is stored once (one rounding), a run that crosses workgroups arrives as one 16-bit
    atomic per piece (the piece's fp32 partial rounded, then the rounded addition)."""
    x = gy32
    if flush_subnormal_inputs:
        x = np.where(np.abs(x) < 2.0 ** -14, np.float32(0), x)
    terms = x[ts]
    if w32 is not None:
        terms = terms * w32[:, None]
    n = ti.shape[0]
    cut = np.ones(n, dtype=bool)
    cut[1:] = ti[1:] != ti[:-1]
    cut[np.arange(0, n, BLOCK)] = True
    head = np.flatnonzero(cut)
    piece = np.add.reduceat(terms.astype(np.float32), head, axis=0, dtype=np.float32)
    run_head = np.ones(head.shape[0], dtype=bool)
    run_head[1:] = ti[head[1:]] != ti[head[:-1]]
    shared = np.zeros(head.shape[0], dtype=bool)                 # pieces of a run that crosses workgroups
    shared[:-1] |= ~run_head[1:]
    shared[1:] |= ~run_head[1:]
    out = np.zeros((rows, gy32.shape[1]), np.float32)
    solo = ~shared
    out[ti[head[solo]]] = X.round_to(kind, piece[solo])
    for p in np.flatnonzero(shared):                              # the atomics, in any order: nz order here
        part = X.round_to(kind, piece[p])
        if flush_subnormal_atomics and kind == "f16":
            part = np.where(np.abs(part) < 2.0 ** -14, np.float32(0), part)
        r = ti[head[p]]
        out[r] = X.round_to(kind, out[r] + part)
    return out.astype(np.float64)


def _reference_backward(kind, gy32, ti, ts, rows):
    """The reference's arithmetic: the running sum rounded to the gradient's type after every lookup."""
    g = X.round_to(kind, gy32)
    out = np.zeros((rows, gy32.shape[1]), np.float32)
    for i in range(ti.shape[0]):
        out[ti[i]] = X.round_to(kind, out[ti[i]] + g[ts[i]])
    return out.astype(np.float64)


def _grads(rng, kind, B, W, magnitude=1.0):
    return X.round_to(kind, rng.uniform(-1, 1, (B, W)).astype(np.float32) * np.float32(magnitude))


def _reference_and_bound(kind, gy32, ti, ts, rows, w32=None):
    ref = X.backward(gy32.astype(np.float64), ts, ti, rows, None if w32 is None else w32.astype(np.float64))
    fl = X.flushes_from_shape(ti, rows, BLOCK)
    return ref, X.error_bound(kind, ref["exact"], ref["scale"], ref["walk"], fl)


def test_helper_sums_and_counts_are_exact():
    """reduceat over runs == a per-lookup fp64 loop; the rounding count follows the workgroup boundaries"""
    rng = np.random.default_rng(1)
    ti, ts = _coo(rng, [3, 1, 300, 5, 600], 40)
    gy = rng.uniform(-1, 1, (40, 4))
    w = rng.uniform(0, 1, ti.shape[0])
    got = X.backward(gy, ts, ti, 10, w)
    want = np.zeros((10, 4))
    for i in range(ti.shape[0]):
        want[ti[i]] += gy[ts[i]] * w[i]
    assert np.allclose(got["exact"], want, rtol=0, atol=1e-12)
    assert got["run_len"].tolist() == [3, 0, 1, 0, 300, 0, 5, 0, 600, 0]
    # runs at nz 0..2, 3, 4..303, 304..308, 309..908 with workgroups of 256 lookups
    assert X.flushes_from_shape(ti, 10, 256).tolist() == [1, 0, 1, 0, 3, 0, 1, 0, 5, 0]
    # pieces of 450 lookups, workgroups restarting in each: the 600-run becomes 309..449 (1), 450..899 (crosses
    # 450 + 256: 3) and 900..908 (1)
    assert X.flushes_from_shape(ti, 10, 256, piece_len=450)[8] == 1 + 3 + 1
    assert X.flushes_from_shape(ti, 10, 256, extra=2).tolist() == [3, 0, 3, 0, 5, 0, 3, 0, 7, 0]


def test_helper_is_fast_at_a_million_lookups():
    import time
    rng = np.random.default_rng(2)
    n, W, B = 1 << 20, 128, 1 << 14
    ti = np.sort((200_000 * rng.random(n) ** 3).astype(np.int64))
    ts = rng.integers(0, B, n)
    gy = rng.uniform(-1, 1, (B, W))
    t0 = time.time()
    ref = X.backward(gy, ts, ti, 200_000)
    X.flushes_from_shape(ti, 200_000, 2048)
    assert time.time() - t0 < 30
    assert ref["run_len"].sum() == n


@pytest.mark.parametrize("kind", ["f16", "bf16", "f32"])
@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
def test_backward_bound_accepts_the_design_and_rejects_a_dropped_lookup(kind, weighted):
    rng = np.random.default_rng(3)
    B, W = 70_000, 16
    ti, ts = _coo(rng, _lengths(rng), B)
    rows = int(ti[-1]) + 1
    gy = _grads(rng, kind, B, W)
    w = X.round_to(kind, rng.uniform(0, 1, ti.shape[0]).astype(np.float32)) if weighted else None
    ref, bound = _reference_and_bound(kind, gy, ti, ts, rows, w)
    got = _design_backward(kind, gy, ti, ts, rows, w)
    assert np.all(np.abs(got - ref["exact"]) <= bound)
    # one lookup of a short run dropped: the one with the largest weight among the first 100 runs' second lookups
    second = np.flatnonzero(np.diff(np.concatenate([[-1], ti])) != 0)[:100] + 1
    second = second[ti[second] == ti[second - 1]]
    victim = int(second[np.argmax(w[second])] if weighted else second[0])
    keep = np.arange(ti.shape[0]) != victim
    bad = _design_backward(kind, gy, ti[keep], ts[keep], rows, None if w is None else w[keep])
    assert np.any(np.abs(bad - ref["exact"]) > bound)


@pytest.mark.parametrize("kind", ["f16", "bf16"])
@pytest.mark.parametrize("signs", ["mixed", "positive"])
def test_backward_bound_rejects_per_lookup_16_bit_rounding(kind, signs):
    """Runs of 5 ... 60,000 lookups.  With gradients of mixed sign every run that the design rounds once (or a few
    times) is off by many more roundings in the reference's arithmetic; with gradients of one sign the reference's
    running sum on the 60,000-lookup run stalls once its spacing exceeds twice the addend."""
    rng = np.random.default_rng(4)
    B, W = 70_000, 8
    ti, ts = _coo(rng, [5, 12, 40, 200, 3000, 9000, 60000], B)
    rows = int(ti[-1]) + 1
    gy = _grads(rng, kind, B, W)
    if signs == "positive":
        gy = np.abs(gy)
    ref, bound = _reference_and_bound(kind, gy, ti, ts, rows)
    assert np.all(np.abs(_design_backward(kind, gy, ti, ts, rows) - ref["exact"]) <= bound)
    err = np.abs(_reference_backward(kind, gy, ti, ts, rows) - ref["exact"])
    if signs == "positive":
        assert np.all(err[12] > bound[12])                          # the 60,000-lookup run, every column
    else:
        assert np.any(err > bound)


def test_backward_bound_rejects_flushed_fp16_subnormals():
    """grads * 2^-20: every input is an fp16 subnormal; the short runs' sums leave the subnormal range, and the long
    runs' per-workgroup partials (256 lookups: ~2^-17) are subnormal when they reach the atomics."""
    rng = np.random.default_rng(5)
    B, W = 70_000, 16
    ti, ts = _coo(rng, _lengths(rng), B)
    rows = int(ti[-1]) + 1
    gy = _grads(rng, "f16", B, W, 2.0 ** -20)
    assert np.all(np.abs(gy) < 2.0 ** -14)
    ref, bound = _reference_and_bound("f16", gy, ti, ts, rows)
    assert np.all(np.abs(_design_backward("f16", gy, ti, ts, rows) - ref["exact"]) <= bound)
    long_row = int(np.argmax(ref["run_len"]))
    assert np.mean(np.abs(ref["exact"][long_row]) >= 2.0 ** -14) > 0.5     # sums that leave the subnormal range
    flushed_in = _design_backward("f16", gy, ti, ts, rows, flush_subnormal_inputs=True)
    assert np.any(np.abs(flushed_in - ref["exact"]) > bound)
    flushed_atomics = _design_backward("f16", gy, ti, ts, rows, flush_subnormal_atomics=True)
    assert np.any(np.abs(flushed_atomics - ref["exact"])[long_row] > bound[long_row])


def _dot_design(kind, t32, g32, flush_subnormals=False):
    """fp32 products and an fp32 running sum (what v_dot2_f32_* promises), rounded once."""
    if flush_subnormals:
        g32 = np.where(np.abs(g32) < 2.0 ** -14, np.float32(0), g32)
        t32 = np.where(np.abs(t32) < 2.0 ** -14, np.float32(0), t32)
    acc = np.zeros(t32.shape[0], np.float32)
    for e in range(t32.shape[1]):
        acc = (acc + t32[:, e] * g32[:, e]).astype(np.float32)
    return X.round_to(kind, acc).astype(np.float64)


@pytest.mark.parametrize("kind", ["f16", "bf16", "f32"])
@pytest.mark.parametrize("W", [8, 64, 1024])
def test_weight_grad_bound(kind, W):
    rng = np.random.default_rng(6 + W)
    n = 4000
    t = X.round_to(kind, rng.uniform(0, 1, (n, W)).astype(np.float32))
    for magnitude in (1.0, 2.0 ** -20) if kind == "f16" else (1.0,):
        g = X.round_to(kind, rng.uniform(-1, 1, (n, W)).astype(np.float32) * np.float32(magnitude))
        exact, scale = X.weight_grad(t.astype(np.float64), np.arange(n), g.astype(np.float64), np.arange(n))
        bound = X.weight_grad_bound(kind, W, exact, scale)
        assert np.all(np.abs(_dot_design(kind, t, g) - exact) <= bound)
        # a product rounded to the element type before it is added: caught (except in rows so wide that the
        # worst-case width * 2^-24 term of the fp32 dot product exceeds it)
        if kind != "f32" and W <= 64:
            per_product = X.round_to(kind, X.round_to(kind, t * g).astype(np.float64).sum(axis=1))
            assert np.any(np.abs(per_product - exact) > bound)
        if magnitude < 1:
            assert np.any(np.abs(_dot_design(kind, t, g, flush_subnormals=True) - exact) > bound)


def _split_design(kind, table32, idx, off, w32=None, mean=False, lds_kind="f32", slices=8):
    """GatherReduceSplitKernel: slice k of a bag pools lookups [k*chunk, (k+1)*chunk) in fp32, the partial rows are
    added in slice order (the cross-lane folds and the LDS stage), the mean scales by 1 / sum(w), one rounding."""
    B, W = off.shape[0] - 1, table32.shape[1]
    out = np.zeros((B, W), np.float32)
    for s in range(B):
        lo, hi = int(off[s]), int(off[s + 1])
        hot = hi - lo
        chunk = -(-hot // slices) if hot else 0
        total = np.zeros(W, np.float32)
        wsum = np.float32(0)
        for k in range(slices):
            a, b = min(lo + k * chunk, hi), min(lo + (k + 1) * chunk, hi)
            part = np.zeros(W, np.float32)
            for j in range(a, b):
                x = table32[idx[j]]
                if w32 is not None:
                    x = (x * w32[j]).astype(np.float32)
                    wsum = np.float32(wsum + w32[j])
                part = (part + x).astype(np.float32)
            part = X.round_to(lds_kind, part) if lds_kind != "f32" else part
            total = (total + part).astype(np.float32)
        if mean:
            ws = wsum if w32 is not None else np.float32(hot)
            total = (total * np.float32(0.0 if ws == 0 else 1.0 / ws)).astype(np.float32)
        out[s] = total
    return X.round_to(kind, out).astype(np.float64)


@pytest.mark.parametrize("kind", ["f16", "bf16", "f32"])
@pytest.mark.parametrize("mode", ["sum", "mean", "weighted_mean"])
def test_split_forward_bound_rejects_element_type_lds_partials(kind, mode):
    rng = np.random.default_rng(7)
    B, H, W, ncat = 24, 61, 32, 500
    table = X.round_to(kind, rng.uniform(-1, 1, (ncat, W)).astype(np.float32))
    idx = rng.integers(0, ncat, B * H)
    off = np.arange(0, B * H + 1, H)
    w = X.round_to(kind, rng.uniform(0, 1, B * H).astype(np.float32)) if mode == "weighted_mean" else None
    mean = mode != "sum"
    exact, scale, hot = X.forward(table.astype(np.float64), idx, off, None if w is None else w.astype(np.float64), mean)
    bound = X.forward_split_bound(kind, exact, scale, hot)
    assert np.all(np.abs(_split_design(kind, table, idx, off, w, mean) - exact) <= bound)
    if kind != "f32":
        bad = _split_design(kind, table, idx, off, w, mean, lds_kind=kind)
        assert np.any(np.abs(bad - exact) > bound)
