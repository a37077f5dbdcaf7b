"""CPU-side checks of the fused 4-bit row-wise tables: the numpy recipe against torch's own CPU prepack (byte for byte,
which pins the format to torch), the value reference against torch's CPU 4-bit lookup, the launch-shape rules and the
argument contract of bits=4 (every rejection raised before any launch)."""
import numpy as np
import pytest
import torch

import quantized_4bit_reference as R4
import quantized_reference as R


@pytest.mark.parametrize("kind", ["f32", "f16"])
@pytest.mark.parametrize("regime", R.REGIMES)
def test_recipe_equals_torch_cpu_prepack_byte_for_byte(regime, kind):
    for width in R4.WIDTHS:
        x = torch.from_numpy(R.make_table(regime, 97, width, seed=width))
        x[0] = 0.0                                  # an all-zero row
        x[1] = x[1, 0] * (1 + torch.arange(width) % 2 * 2.0 ** -12)   # a near-constant row
        if kind == "f16":
            x = x.clamp(-6e4, 6e4).half()           # (lognormal(0, 3) exceeds fp16's range: inf is not table data)
        want = torch.ops.quantized.embedding_bag_4bit_prepack(x)
        assert want.dtype == torch.uint8 and tuple(want.shape) == (97, width // 2 + 4)
        assert np.array_equal(R4.quantize(x.float().numpy()), want.numpy()), (regime, kind, width)


def test_dequant64_agrees_with_torch_cpu_lookup_of_single_rows():
    """Bags of one row each: torch's CPU 4-bit lookup returns that row's values, to fp32 rounding of code * scale + bias."""
    q = R4.quantize(R.make_table("normal", 50, 48, seed=3))
    ids = torch.arange(50)
    got = torch.ops.quantized.embedding_bag_4bit_rowwise_offsets(torch.from_numpy(q), ids, torch.arange(51), False, 0,
                                                                 False, None, None, True).numpy()
    exact = R4.dequant64(q)
    codes, scale, bias = R4.split(q)
    magnitude = codes * scale.astype(np.float64)[:, None] + np.abs(bias.astype(np.float64))[:, None]
    assert got.shape == exact.shape and (np.abs(got - exact) <= 2.0 ** -23 * magnitude).all()
    assert (np.abs(R4.dequant32(q) - exact) <= 2.0 ** -23 * magnitude).all()


def _q4(rows=20, width=16):
    return torch.zeros((rows, width // 2 + 4), dtype=torch.uint8)


def test_bits_4_rejects_misuse_before_any_launch():
    import cuembed_amd as ce
    fwd = ce.embedding_forward_quantized
    idx = torch.zeros(12, dtype=torch.int64)
    for call in (lambda: ce.quantize_rows(torch.zeros((4, 8)), bits=3), lambda: ce.dequantize_rows(_q4(), bits=3),
                 lambda: fwd(_q4(), idx, num_hots=4, bits=3), lambda: ce.QuantizedEmbeddingBag(_q4(), bits=16),
                 lambda: ce.quantized_forward_launch_shape(torch.int32, torch.float16, 256, 64, 8, bits=2),
                 lambda: ce.quantized_row_bytes(256, bits=2)):
        with pytest.raises(ValueError, match="bits must be 8 or 4"):
            call()
    with pytest.raises(ValueError, match="W % 8"):
        ce.quantize_rows(torch.zeros((4, 12)), bits=4)
    with pytest.raises(ValueError, match="W % 8"):
        fwd(_q4(20, 12), idx, num_hots=4, bits=4)
    with pytest.raises(TypeError, match=r"uint8 tensor \[rows, width/2 \+ 4\]"):
        fwd(_q4().float(), idx, num_hots=4, bits=4)
    with pytest.raises(TypeError, match="weights must have the output's dtype"):
        fwd(_q4(), idx, num_hots=4, weights=torch.ones(12), out_dtype=torch.float16, bits=4)
    with pytest.raises(ValueError, match="requires grad"):
        fwd(_q4(), idx, num_hots=4, weights=torch.ones(12, dtype=torch.float16, requires_grad=True), bits=4)
    with pytest.raises(ValueError, match="requires grad"):
        ce.quantize_rows(torch.zeros((4, 8), requires_grad=True), bits=4)
    with pytest.raises(ValueError, match="more than 1024"):         # 8 codes per lane: 1,025 lanes
        ce.quantized_forward_launch_shape(torch.int32, torch.float16, 8200, 64, 8, bits=4)
    with pytest.raises(RuntimeError, match="GPU"):                  # everything else in order: only the device is wrong
        fwd(_q4(), idx, num_hots=4, bits=4)
    with pytest.raises(RuntimeError, match="GPU"):
        ce.QuantizedEmbeddingBag.from_float(torch.zeros((4, 8)), bits=4)
    bag = ce.QuantizedEmbeddingBag(_q4(20, 16), bits=4)
    assert (bag.num_embeddings, bag.embedding_dim, ce.quantized_row_bytes(256, bits=4)) == (20, 16, 132)


def test_launch_shapes():
    import cuembed_amd as ce

    def shape(width, batch=65536, hot=64, **kw):
        return ce.quantized_forward_launch_shape(torch.int32, torch.float16, width, batch, hot, bits=4, **kw)

    # config 2: 32 codes per lane (one 16-byte load), 8 lanes per row, eight samples per wavefront, indices staged
    assert shape(256) == dict(codes_per_lane=32, lanes_per_row=8, samples_per_block=32, grid=2048, lds_bytes=32 * 64 * 4,
                              staged=True)
    assert (shape(48)["codes_per_lane"], shape(48)["lanes_per_row"]) == (16, 3)
    assert (shape(24)["codes_per_lane"], shape(24)["lanes_per_row"]) == (8, 3)
    assert (shape(96)["codes_per_lane"], shape(96)["lanes_per_row"]) == (32, 3)
    # the 32-code lanes stay inside a 256-thread workgroup: wider rows take 16 codes per lane
    assert (shape(8192)["codes_per_lane"], shape(8192)["lanes_per_row"]) == (32, 256)
    assert (shape(16384)["codes_per_lane"], shape(16384)["lanes_per_row"]) == (16, 1024)
    # CSR: one wavefront per workgroup, nothing staged; small grids are cut down to a wavefront
    assert shape(256, hot=0, is_csr=True) == dict(codes_per_lane=32, lanes_per_row=8, samples_per_block=8, grid=8192,
                                                  lds_bytes=0, staged=False)
    assert shape(256, batch=1024)["samples_per_block"] == 8
