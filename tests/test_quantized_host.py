"""CPU-side checks of the 8-bit row-wise quantized tables: the quantizer recipe against torch's own CPU prepack (byte
for byte, which pins the format to torch on whichever machine the suite runs), the forward's error bound against
torch's CPU lookup (must pass) and three wrong implementations (must fail), the C ABI, the launch-shape rules and the
argument contract of the host layer (every rejection raised before any launch)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import quantized_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cuembed_amd.h")
SYMBOLS = ("cuembed_quantized_row_bytes", "cuembed_quantize_rows", "cuembed_dequantize_rows",
           "cuembed_embedding_forward_quantized", "cuembed_quantized_forward_launch_shape")


# ---- the format is torch's --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("regime", R.REGIMES)
def test_recipe_equals_torch_cpu_prepack_byte_for_byte(regime, kind):
    for width in R.WIDTHS:
        x = torch.from_numpy(R.make_table(regime, 97, width, seed=width))
        if kind == "f16":
            x = x.clamp(-6e4, 6e4).half()          # (lognormal(0, 3) exceeds fp16's range: inf is not table data)
            want = torch.ops.quantized.embedding_bag_byte_prepack(x)
        elif kind == "bf16":
            x = x.bfloat16()
            want = torch.ops.quantized.embedding_bag_byte_prepack(x.float())   # (torch's prepack has no bf16 input)
        else:
            want = torch.ops.quantized.embedding_bag_byte_prepack(x)
        got = R.quantize(x.float().numpy())
        assert want.dtype == torch.uint8 and tuple(want.shape) == (97, width + 8)
        assert np.array_equal(got, want.numpy()), (regime, kind, width)


def test_dequant_references_agree_with_torch_unpack():
    """torch's CPU unpack fuses code * scale + bias into one rounding; the library's dequantizer rounds twice (so that
    any fp32 machine reproduces it): both sit within their roundings of the fp64 values."""
    q = R.quantize(R.make_table("normal", 50, 64, seed=3))
    want = torch.ops.quantized.embedding_bag_byte_unpack(torch.from_numpy(q)).numpy()
    exact = R.dequant64(q)
    codes, scale, _ = R.split(q)
    product = codes.astype(np.float64) * scale.astype(np.float64)[:, None]
    assert (np.abs(want - exact) <= 2.0 ** -24 * np.abs(exact)).all()
    assert (np.abs(R.dequant32(q) - exact) <= 2.0 ** -24 * (product + np.abs(exact))).all()


# ---- the bound: what it must accept and what it must reject ------------------------------------------------------------
def _batch(hot, weighted, seed, rows=500, width=64, batch=32):
    rng = np.random.default_rng(seed)
    q = R.quantize(R.make_table("normal", rows, width, seed=seed + 1))
    idx = rng.integers(0, rows, batch * hot)
    w = rng.uniform(-1.0, 1.0, batch * hot).astype(np.float32) if weighted else None
    return q, idx, w


def _fp32_lookup(q, idx, hot, w, drop_bias_at=None, neighbour_scale=False, half_running_sum=False):
    """A sequential fp32 lookup (value = code * scale + bias, acc += w * value), optionally broken."""
    codes, scale, bias = R.split(q)
    f = np.float32
    batch = idx.size // hot
    out = np.zeros((batch, codes.shape[1]), dtype=f)
    for s in range(batch):
        acc = np.zeros(codes.shape[1], dtype=f)
        for j in range(hot):
            r = idx[s * hot + j]
            sc = scale[(r + 1) % scale.size] if neighbour_scale else scale[r]
            b = f(0) if (drop_bias_at is not None and j == drop_bias_at) else bias[r]
            v = ((codes[r].astype(f) * sc).astype(f) + b).astype(f)
            if w is not None:
                v = (v * w[s * hot + j]).astype(f)
            acc = (acc + v).astype(f)
            if half_running_sum:
                acc = acc.astype(np.float16).astype(f)
        out[s] = acc
    return out


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("hot", [1, 7, 64, 300])
def test_bound_accepts_torch_cpu_lookup(hot, weighted):
    q, idx, w = _batch(hot, weighted, seed=hot)
    batch = idx.size // hot
    offsets = np.arange(0, idx.size + 1, hot)
    got = torch.ops.quantized.embedding_bag_byte_rowwise_offsets(
        torch.from_numpy(q), torch.from_numpy(idx), torch.from_numpy(offsets), False, 0, False,
        None if w is None else torch.from_numpy(w), None, True).numpy()
    assert got.shape == (batch, q.shape[1] - 8)
    exact, bound = R.pooled64(q, idx, num_hots=hot, weights=w)
    assert R.worst_ratio(got, exact, bound) <= 1.0
    # ... and the plain sequential fp32 loop
    assert R.worst_ratio(_fp32_lookup(q, idx, hot, w), exact, bound) <= 1.0


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("hot", [1, 7, 64, 300])
def test_bound_rejects_wrong_implementations(hot, weighted):
    q, idx, w = _batch(hot, weighted, seed=100 + hot)
    exact, bound = R.pooled64(q, idx, num_hots=hot, weights=w)
    wrong = dict(bias_dropped_for_one_lookup=_fp32_lookup(q, idx, hot, w, drop_bias_at=hot // 2),
                 neighbouring_rows_scale=_fp32_lookup(q, idx, hot, w, neighbour_scale=True))
    if hot > 1:      # (with one lookup there is no running sum to round)
        wrong["running_sum_rounded_to_fp16"] = _fp32_lookup(q, idx, hot, w, half_running_sum=True)
    for name, got in wrong.items():
        outside = np.abs(got.astype(np.float64) - exact) > bound
        # (the GPU test fails on ONE element outside; a tenth of all elements shows the miss is not marginal)
        assert outside.mean() > 0.1, name


def test_bound_is_far_below_the_quantisation_step():
    """At its tightest element the bound is a small fraction of |exact| and far below one 8-bit step of the row."""
    for hot in (1, 7, 64, 300):
        q, idx, _ = _batch(hot, False, seed=7)
        exact, bound = R.pooled64(q, idx, num_hots=hot)
        _, scale, _ = R.split(q)
        assert bound.max() < 1e-2 * scale.min() * np.sqrt(hot) * hot


def test_mean_and_fp16_bounds_extend_the_sum_bound():
    q, idx, w = _batch(7, True, seed=5)
    w = np.abs(w) + 0.25
    s_exact, s_bound = R.pooled64(q, idx, num_hots=7, weights=w)
    m_exact, m_bound = R.pooled64(q, idx, num_hots=7, weights=w, mode="mean")
    recip = 1.0 / w.astype(np.float64).reshape(-1, 7).sum(1)
    assert np.allclose(m_exact, s_exact * recip[:, None], rtol=1e-15)
    assert np.allclose(m_bound, s_bound * recip[:, None] + 2.0 ** -24 * np.abs(m_exact), rtol=1e-12)
    _, h_bound = R.pooled64(q, idx, num_hots=7, weights=w, out="f16")
    assert np.allclose(h_bound, s_bound + 2.0 ** -11 * np.abs(s_exact) + 2.0 ** -25, rtol=1e-12)
    # empty bags: zeros, zero bound
    e, b = R.pooled64(q, idx[:6], offsets=np.array([0, 0, 6, 6]), mode="mean")
    assert not e[0].any() and not e[2].any() and not b[0].any()


# ---- C ABI ---------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_in_plain_c_and_exported():
    from cuembed_amd import build
    pre = subprocess.run(["gcc", "-E", "-P", HEADER], check=True, stdout=subprocess.PIPE, text=True).stdout
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, pre), name
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", HEADER], check=True)
    L = ctypes.CDLL(build.build())
    for name in SYMBOLS:
        assert hasattr(L, name), name
    assert "c_api_quantized.hip" in build.UNITS
    L.cuembed_quantized_row_bytes.restype = ctypes.c_int64
    assert L.cuembed_quantized_row_bytes(256) == 264


def test_launch_shapes():
    import cuembed_amd as ce
    shape = ce.quantized_forward_launch_shape
    i32, i64, f16, f32 = torch.int32, torch.int64, torch.float16, torch.float32
    # config 2: 16 codes per lane (one 16-byte load), 16 lanes per row, four samples per wavefront, four wavefronts per
    # workgroup, the indices of a workgroup staged in LDS -- on every device large or small
    for cus, xcds in ((32, 1), (128, 4), (256, 8)):
        assert shape(i32, f16, 256, 65536, 64, compute_units=cus, xcds=xcds) == dict(
            codes_per_lane=16, lanes_per_row=16, samples_per_block=16, grid=4096, lds_bytes=16 * 64 * 4, staged=True)
    # batch 1,024: a grid of fewer than two workgroups per compute unit is cut into smaller workgroups, down to one
    # wavefront -- so the shape follows the device it is told about
    assert shape(i32, f16, 256, 1024, 64, compute_units=32, xcds=1)["samples_per_block"] == 16     # 64 >= 64
    mid = shape(i32, f16, 256, 1024, 64, compute_units=128, xcds=4)
    assert (mid["samples_per_block"], mid["grid"]) == (4, 256)                                     # 256 >= 256
    small = shape(i32, f16, 256, 1024, 64, compute_units=256, xcds=8)
    assert (small["samples_per_block"], small["grid"], small["lds_bytes"]) == (4, 256, 4 * 64 * 4)  # never below a wavefront
    assert shape(i32, f16, 256, 64, 64, compute_units=256, xcds=8)["samples_per_block"] == 4
    assert shape(i32, f16, 64, 2048, 8, compute_units=256, xcds=8)["samples_per_block"] == 16      # 4 lanes: a wavefront is 16
    assert shape(i32, f16, 64, 2048, 8, compute_units=32, xcds=1)["samples_per_block"] == 32
    # weights are staged with the indices, in the output's type
    assert shape(i64, f32, 256, 65536, 64, is_weighted=True)["lds_bytes"] == 16 * 64 * (8 + 4)
    assert shape(i64, f16, 256, 65536, 64, is_weighted=True)["lds_bytes"] == 16 * 64 * (8 + 2)
    # a bag too long for the staging budget (16 KiB): fewer samples per workgroup first, then no staging at all (and
    # the workgroup keeps its size)
    assert shape(i64, f32, 256, 65536, 300, is_weighted=True) == dict(
        codes_per_lane=16, lanes_per_row=16, samples_per_block=4, grid=16384, lds_bytes=4 * 300 * 12, staged=True)
    assert shape(i64, f32, 256, 65536, 3000, is_weighted=True) == dict(
        codes_per_lane=16, lanes_per_row=16, samples_per_block=16, grid=4096, lds_bytes=0, staged=False)
    # CSR: one wavefront per workgroup, nothing staged
    assert shape(i32, f16, 256, 65536, 0, is_csr=True) == dict(
        codes_per_lane=16, lanes_per_row=16, samples_per_block=4, grid=16384, lds_bytes=0, staged=False)
    # lanes follow the row: 16 codes where the row divides into 16s (and fits a 256-thread workgroup), else 8, else
    # 4-byte lanes; lanes need not be a power of two
    assert (shape(i32, f16, 36, 65536, 8)["codes_per_lane"], shape(i32, f16, 36, 65536, 8)["lanes_per_row"]) == (4, 9)
    assert (shape(i32, f16, 100, 65536, 8)["codes_per_lane"], shape(i32, f16, 100, 65536, 8)["lanes_per_row"]) == (4, 25)
    assert (shape(i32, f16, 24, 65536, 8)["codes_per_lane"], shape(i32, f16, 24, 65536, 8)["lanes_per_row"]) == (8, 3)
    assert (shape(i32, f16, 512, 65536, 8)["codes_per_lane"], shape(i32, f16, 512, 65536, 8)["lanes_per_row"]) == (16, 32)
    assert (shape(i32, f16, 4096, 65536, 8)["codes_per_lane"], shape(i32, f16, 4096, 65536, 8)["lanes_per_row"]) == (16, 256)
    assert (shape(i32, f16, 8192, 65536, 8)["codes_per_lane"], shape(i32, f16, 8192, 65536, 8)["lanes_per_row"]) == (8, 1024)
    assert shape(i32, f16, 4, 65536, 8) == dict(codes_per_lane=4, lanes_per_row=1, samples_per_block=128, grid=512,
                                                lds_bytes=128 * 8 * 4, staged=True)


# ---- argument contract (CPU tensors: every rejection comes before the device check, hence before any launch) ----------
def _q(rows=20, width=16):
    return torch.zeros((rows, width + 8), dtype=torch.uint8)


def test_forward_rejects_misuse_before_any_launch():
    import cuembed_amd as ce
    fwd = ce.embedding_forward_quantized
    idx = torch.zeros(12, dtype=torch.int64)
    off = torch.tensor([0, 5, 12])
    with pytest.raises(TypeError, match="uint8"):
        fwd(_q().float(), idx, num_hots=4)
    with pytest.raises(TypeError, match="2-D"):
        fwd(_q().view(-1), idx, num_hots=4)
    with pytest.raises(ValueError, match="contiguous"):
        fwd(_q(20, 40)[:, :24], idx, num_hots=4)
    with pytest.raises(ValueError, match="multiple of 4"):
        fwd(_q(20, 18), idx, num_hots=4)
    with pytest.raises(ValueError, match="multiple of 4"):
        fwd(torch.zeros((20, 8), dtype=torch.uint8), idx, num_hots=4)          # no codes at all
    with pytest.raises(ValueError, match="mode"):
        fwd(_q(), idx, num_hots=4, mode="max")
    with pytest.raises(ValueError, match="row_loads"):
        fwd(_q(), idx, num_hots=4, row_loads="nt")
    with pytest.raises(TypeError, match="float32 or torch.float16"):
        fwd(_q(), idx, num_hots=4, out_dtype=torch.bfloat16)
    with pytest.raises(TypeError, match="int32 or int64"):
        fwd(_q(), idx.to(torch.int16), num_hots=4)
    with pytest.raises(TypeError, match="weights must have the output's dtype"):
        fwd(_q(), idx, num_hots=4, weights=torch.ones(12), out_dtype=torch.float16)
    with pytest.raises(TypeError, match="weights must have the output's dtype"):
        fwd(_q(), idx, num_hots=4, weights=torch.ones(12).half(), out_dtype=torch.float32)
    with pytest.raises(ValueError, match="concat does not take weights"):
        fwd(_q(), idx, num_hots=4, weights=torch.ones(12).half(), mode="concat")
    with pytest.raises(ValueError, match="CSR layout does not support concat"):
        fwd(_q(), idx, offsets=off, mode="concat")
    with pytest.raises(ValueError, match="either CSR"):
        fwd(_q(), idx, offsets=off, num_hots=4)
    with pytest.raises(ValueError, match="either CSR"):
        fwd(_q(), idx)
    with pytest.raises(ValueError, match="requires grad"):
        fwd(_q(), idx, num_hots=4, weights=torch.ones(12, dtype=torch.float16, requires_grad=True))
    with pytest.raises(ValueError, match="multiple of num_hots"):
        fwd(_q(), idx, num_hots=5)
    with pytest.raises(ValueError, match="one entry per index"):
        fwd(_q(), idx, num_hots=4, weights=torch.ones(8).half())
    with pytest.raises(ValueError, match="sample_order"):
        fwd(_q(), idx, num_hots=4, sample_order=torch.arange(3, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="GPU"):          # everything else in order: only the device is wrong
        fwd(_q(), idx, num_hots=4)
    with pytest.raises(RuntimeError, match="GPU"):
        fwd(_q(), idx, offsets=off, weights=torch.ones(12).half(), mode="mean")


def test_quantizer_and_dequantizer_reject_misuse_before_any_launch():
    import cuembed_amd as ce
    with pytest.raises(TypeError, match="float32, float16 or bfloat16"):
        ce.quantize_rows(torch.zeros((4, 8), dtype=torch.float64))
    with pytest.raises(ValueError, match="rows, width"):
        ce.quantize_rows(torch.zeros(8))
    with pytest.raises(ValueError, match="multiple of 4"):
        ce.quantize_rows(torch.zeros((4, 6)))
    with pytest.raises(ValueError, match="requires grad"):
        ce.quantize_rows(torch.zeros((4, 8), requires_grad=True))
    with pytest.raises(RuntimeError, match="GPU"):
        ce.quantize_rows(torch.zeros((4, 8)))
    with pytest.raises(TypeError, match="uint8"):
        ce.dequantize_rows(torch.zeros((4, 16)))
    with pytest.raises(TypeError, match="float32 or torch.float16"):
        ce.dequantize_rows(_q(), dtype=torch.bfloat16)
    with pytest.raises(TypeError, match="int32 or int64"):
        ce.dequantize_rows(_q(), ids=torch.zeros(3))
    with pytest.raises(RuntimeError, match="GPU"):
        ce.dequantize_rows(_q(), ids=torch.zeros(3, dtype=torch.int32))
    assert ce.quantized_row_bytes(256) == 264


def test_bag_module_contract():
    import cuembed_amd as ce
    bag = ce.QuantizedEmbeddingBag(_q(20, 16), mode="mean", out_dtype=torch.float32)
    assert (bag.num_embeddings, bag.embedding_dim) == (20, 16)
    with pytest.raises(ValueError, match="mode"):
        ce.QuantizedEmbeddingBag(_q(), mode="concat")
    with pytest.raises(TypeError, match="uint8"):
        ce.QuantizedEmbeddingBag(torch.zeros((4, 16)))
    with pytest.raises(RuntimeError, match="GPU"):
        bag(torch.zeros(4, dtype=torch.int64), torch.tensor([0, 4]))
    with pytest.raises(RuntimeError, match="GPU"):
        ce.QuantizedEmbeddingBag.from_float(torch.zeros((4, 8)))
