"""Fused 4-bit row-wise tables on the GPU: the quantizer against torch's CPU prepack (exact bytes), the dequantizer
and concat against the two-rounding fp32 model (exact bits), the pooled forward against the fp64 value of the same fused
bytes under the bound of tests/quantized_reference.py (every element), bits that depend on nothing but the bag, one HIP
graph replay and the three torch ops."""
import numpy as np
import pytest
import torch

import quantized_4bit_reference as R4
import quantized_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROWS, BATCH = 1000, 70                      # more than one workgroup, the last one partial
HOTS = (1, 3, 4, 5, 7, 8, 9, 17)            # 1, U - 1, U, U + 1, 2U + 1 for both batch sizes U = 4 and U = 8 of the gather
_NP = {"f32": np.float32, "f16": np.float16}
_TORCH = {"f32": torch.float32, "f16": torch.float16}
_TABLES = {}


@pytest.fixture(scope="module")
def ce():
    import cuembed_amd
    return cuembed_amd


def _table(width):
    """ROWS rows as fp32: N(0, 9), U(0, 1), 30 + U(-1, 1) and constant rows interleaved (sums of 17 lookups fit fp16),
    row 0 all zero.  Computed once per width."""
    if width not in _TABLES:
        parts = [R.make_table("normal", ROWS // 4, width, seed=width), R.make_table("uniform", ROWS // 4, width, seed=width + 17),
                 R.make_table("offset", ROWS // 4, width, seed=width + 34) - np.float32(1e4 - 30.0),
                 R.make_table("constant", ROWS // 4, width, seed=width + 51)]
        x = np.ascontiguousarray(np.stack(parts, axis=1).reshape(-1, width))
        x[0] = 0.0
        _TABLES[width] = x
    return _TABLES[width]


def _fused(ce, width):
    """(device table, its bytes on the host) of _table(width), quantized on the device."""
    q = ce.quantize_rows(torch.from_numpy(_table(width)).to(DEV), bits=4)
    return q, q.cpu().numpy()


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16).numpy()


@pytest.mark.parametrize("kind", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("width", R4.WIDTHS + (2056,))       # 2,056: a row the quantizer reads twice
def test_quantizer_writes_torch_cpu_prepack_bytes(ce, width, kind):
    x = torch.from_numpy(_table(width)[:300])
    x = {"f32": x, "f16": x.half(), "bf16": x.bfloat16()}[kind]
    got = ce.quantize_rows(x.to(DEV), bits=4)
    want = torch.ops.quantized.embedding_bag_4bit_prepack(x.float() if kind == "bf16" else x)    # (no bf16 input there)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (300, width // 2 + 4)
    assert torch.equal(got.cpu(), want)


@pytest.mark.parametrize("width", R4.WIDTHS)
def test_dequantizer_and_concat_are_bit_equal_to_the_two_rounding_model(ce, width):
    q, q_np = _fused(ce, width)
    want = {"f32": R4.dequant32(q_np)}
    want["f16"] = want["f32"].astype(np.float16)
    rng = np.random.default_rng(width)
    for out in ("f32", "f16"):
        assert np.array_equal(_bits(ce.dequantize_rows(q, dtype=_TORCH[out], bits=4)), _bits(torch.from_numpy(want[out])))
        for idt in (torch.int32, torch.int64):
            ids_np = rng.integers(0, ROWS, (37, 5))
            ids = torch.from_numpy(ids_np).to(DEV, idt)
            got = ce.dequantize_rows(q, ids, dtype=_TORCH[out], bits=4)
            assert tuple(got.shape) == (37, 5, width)
            assert np.array_equal(_bits(got), _bits(torch.from_numpy(want[out][ids_np])))
            concat = ce.embedding_forward_quantized(q, ids.view(-1), num_hots=5, mode="concat", out_dtype=_TORCH[out], bits=4)
            assert torch.equal(concat, got)


def _csr_offsets(rng):
    """Bag lengths drawn from HOTS and 0, with empty bags first, last and inside."""
    lengths = rng.choice((0,) + HOTS, BATCH)
    lengths[[0, BATCH // 3, BATCH - 1]] = 0
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


@pytest.mark.parametrize("out", ["f32", "f16"])
@pytest.mark.parametrize("layout", ["fixed", "csr"])
@pytest.mark.parametrize("width", R4.WIDTHS)
def test_forward_meets_the_bound_on_every_element(ce, width, layout, out):
    """|got - exact| <= bound for every output element: int32 / int64 indices and offsets x weighted or not x sum /
    mean.  Weights: U(-1, 1) for sum, U(0.25, 1.25) for mean (a weight sum near zero makes the mean itself
    ill-conditioned, as tests/test_gpu_quantized.py explains)."""
    q, q_np = _fused(ce, width)
    rng = np.random.default_rng(1000 * width + (layout == "csr"))
    worst = 0.0
    for hot in HOTS if layout == "fixed" else (0,):
        off_np = _csr_offsets(rng) if layout == "csr" else None
        nnz = int(off_np[-1]) if layout == "csr" else BATCH * hot
        idx_np = rng.integers(0, ROWS, nnz)
        for mode in ("sum", "mean"):
            for weighted in (False, True):
                w_np = None
                if weighted:
                    w_np = (rng.uniform(-1, 1, nnz) if mode == "sum" else rng.uniform(0.25, 1.25, nnz)).astype(_NP[out])
                exact, bound = R4.pooled64(q_np, idx_np, offsets=off_np, num_hots=hot, weights=w_np, mode=mode, out=out)
                for idt in (torch.int32, torch.int64):
                    got = ce.embedding_forward_quantized(
                        q, torch.from_numpy(idx_np).to(DEV, idt),
                        offsets=None if off_np is None else torch.from_numpy(off_np).to(DEV, idt),
                        weights=None if w_np is None else torch.from_numpy(w_np).to(DEV), num_hots=hot, mode=mode,
                        out_dtype=_TORCH[out], bits=4)
                    assert got.dtype == _TORCH[out] and tuple(got.shape) == (BATCH, width)
                    got_np = got.float().cpu().numpy()
                    ratio = R.worst_ratio(got_np, exact, bound)
                    worst = max(worst, ratio)
                    assert np.isfinite(got_np).all() and ratio <= 1.0, (width, layout, out, hot, mode, weighted, idt, ratio)
                    if off_np is not None:      # empty bags give zeros
                        assert not got_np[np.diff(off_np) == 0].any()
    print("worst |got - exact| / bound: %.3f (W=%d, %s, %s)" % (worst, width, layout, out))


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("width", R4.WIDTHS)
def test_result_depends_on_nothing_but_the_bag(ce, width, weighted):
    q, _ = _fused(ce, width)
    hot = 9
    idx = torch.randint(0, ROWS, (BATCH, hot), device=DEV, dtype=torch.int32)
    w = (torch.rand((BATCH, hot), device=DEV) * 2 - 1).half() if weighted else None
    for mode in ("sum", "mean"):
        def fwd(**kw):
            return ce.embedding_forward_quantized(q, idx.view(-1), weights=w, mode=mode, bits=4, **kw)
        a = fwd(num_hots=hot)
        for odt in (torch.int32, torch.int64):     # fixed hotness against the CSR form of the same bags
            off = torch.arange(0, BATCH * hot + 1, hot, device=DEV, dtype=odt)
            assert torch.equal(a, fwd(offsets=off))
        assert torch.equal(a, fwd(offsets=off, sample_order=torch.randperm(BATCH, device=DEV).int()))
        assert torch.equal(a, fwd(num_hots=hot, row_loads="default")) and torch.equal(a, fwd(num_hots=hot, row_loads="streaming"))
        small = ce.embedding_forward_quantized(q, idx[:3].reshape(-1), num_hots=hot, mode=mode, bits=4,
                                               weights=None if w is None else w[:3].contiguous())
        assert torch.equal(a[:3], small)           # a batch of 3 (another launch shape) against the batch of 70


def test_forward_replays_from_a_hip_graph(ce):
    """One captured forward with out= given, replayed three times on fresh indices and weights copied into the captured
    buffers: each replay equals the eager call."""
    width, hot = 256, 9
    q, _ = _fused(ce, width)
    idx = torch.randint(0, ROWS, (BATCH * hot,), device=DEV, dtype=torch.int32)
    w = torch.rand(BATCH * hot, device=DEV).half()
    out = torch.empty((BATCH, width), dtype=torch.float16, device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ce.embedding_forward_quantized(q, idx, num_hots=hot, weights=w, mode="mean", out=out, bits=4)    # warm-up
        torch.cuda.current_stream().synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            ce.embedding_forward_quantized(q, idx, num_hots=hot, weights=w, mode="mean", out=out, bits=4)
    torch.cuda.synchronize()
    for _ in range(3):
        idx.copy_(torch.randint(0, ROWS, (BATCH * hot,), device=DEV, dtype=torch.int32))
        w.copy_(torch.rand(BATCH * hot, device=DEV).half())
        out.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, ce.embedding_forward_quantized(q, idx, num_hots=hot, weights=w, mode="mean", bits=4))


def test_torch_ops(ce):
    from cuembed_amd import cuembed_pyt as P
    ops = torch.ops.cuembed_pyt
    width, hot = 96, 5
    table = torch.from_numpy(_table(width)).to(DEV)
    q = P.quantize_rows(table, bits=4)
    assert torch.equal(q, ce.quantize_rows(table, bits=4))
    idx = torch.randint(0, ROWS, (BATCH, hot), device=DEV)
    off = torch.arange(0, BATCH * hot + 1, hot, device=DEV)
    w = torch.rand(BATCH * hot, device=DEV)
    assert torch.equal(P.dequantize_rows(q, idx, torch.float16, bits=4), ce.dequantize_rows(q, idx, torch.float16, bits=4))
    for mode in ("sum", "mean"):
        want = ce.embedding_forward_quantized(q, idx.view(-1), offsets=off, weights=w, mode=mode, out_dtype=torch.float32, bits=4)
        assert torch.equal(P.cuemb_embedding_quantized(q, idx.view(-1), off, w, mode, torch.float32, bits=4), want)
        assert torch.equal(ops.cuemb_embedding_quantized_4bit(q, idx, None, w, mode, torch.float32, -1, None, None), want)
    assert torch.equal(P.cuemb_embedding_quantized(q, idx, mode="concat", bits=4),
                       ce.embedding_forward_quantized(q, idx.view(-1), num_hots=hot, mode="concat", bits=4))
    for op, args in [(ops.quantize_rows_4bit, (table.half(),)), (ops.dequantize_rows_4bit, (q, idx, torch.float16)),
                     (ops.dequantize_rows_4bit, (q, None, torch.float32)),
                     (ops.cuemb_embedding_quantized_4bit, (q, idx.view(-1), off, w.half(), "mean", torch.float16, 1, None, None)),
                     (ops.cuemb_embedding_quantized_4bit, (q, idx, None, None, "concat", torch.float32, -1, None, None))]:
        torch.library.opcheck(op, args, test_utils=("test_schema", "test_faketensor"))
