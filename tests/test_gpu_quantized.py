"""8-bit row-wise quantized tables on the GPU: the quantizer against the recipe (exact bytes), the dequantizer and
concat against the two-rounding fp32 recipe (exact bits), the pooled forward against the fp64 value of the same fused
bytes under the derived bound of tests/quantized_reference.py (every element, none skipped), order / determinism bit
for bit, interop with torch's CPU prepack, the full-size config-2 batch, HIP graph replay and the torch ops."""
import numpy as np
import pytest
import torch

import quantized_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
HOTS = (1, 7, 64, 300)
_NP = {"f32": np.float32, "f16": np.float16}
_TORCH = {"f32": torch.float32, "f16": torch.float16}


@pytest.fixture(scope="module")
def ce():
    import cuembed_amd
    return cuembed_amd


def _as_kind(x, kind):
    """fp32 numpy data as a torch tensor of `kind` (fp16: clamped to the type's range first -- lognormal(0, 3) exceeds
    it, and inf is not table data)."""
    t = torch.from_numpy(x)
    if kind == "f16":
        return t.clamp(-6e4, 6e4).half()
    if kind == "bf16":
        return t.bfloat16()
    return t


def _mixed_table(width, rows_per_regime=200, seed=0):
    """Rows of every data regime, interleaved, as fp32."""
    parts = [R.make_table(regime, rows_per_regime, width, seed=seed + 17 * k) for k, regime in enumerate(R.REGIMES)]
    x = np.stack(parts, axis=1).reshape(-1, width)
    return np.ascontiguousarray(x)


def _tame_table(width, rows_per_regime=100, seed=0):
    """The same mix with sums that stay inside fp16's range over 600 lookups: N(0, 9), U(0, 1), 30 + U(-1, 1) in place
    of 1e4 + U(-1, 1), constant rows; no lognormal(0, 3) rows (single values reach 1e5)."""
    parts = [R.make_table("normal", rows_per_regime, width, seed=seed),
             R.make_table("uniform", rows_per_regime, width, seed=seed + 17),
             R.make_table("offset", rows_per_regime, width, seed=seed + 34) - np.float32(1e4 - 30.0),
             R.make_table("constant", rows_per_regime, width, seed=seed + 51)]
    return np.ascontiguousarray(np.stack(parts, axis=1).reshape(-1, width))


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16).numpy()


# ---- quantizer ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("regime", R.REGIMES)
def test_quantizer_writes_the_recipes_bytes(ce, regime, kind):
    """Device bytes == recipe bytes.  Rows whose scale would be subnormal are left out of the data on purpose
    (quantized_reference.make_table says why)."""
    for width in R.WIDTHS:
        x = _as_kind(R.make_table(regime, 1003, width, seed=3 * width), kind)
        got = ce.quantize_rows(x.to(DEV))
        assert got.dtype == torch.uint8 and tuple(got.shape) == (1003, width + 8)
        want = R.quantize(x.float().numpy())
        _, scale, _ = R.split(want)
        assert ((scale == 0) | (scale >= np.finfo(np.float32).tiny)).all()      # no subnormal scale in the data
        assert np.array_equal(got.cpu().numpy(), want), (regime, kind, width)


@pytest.mark.parametrize("width", [1028, 2052, 4096, 8192])
def test_wide_rows(ce, width):
    """Rows beyond what a lane group keeps in registers (the quantizer reads them twice), the 4-byte-lane fall-back on
    long rows, and the widest rows of the forward (256 lanes of 16 codes, 1,024 lanes of 8)."""
    x = torch.from_numpy(R.make_table("normal", 77, width, seed=width))
    q = ce.quantize_rows(x.to(DEV))
    want = R.quantize(x.numpy())
    assert np.array_equal(q.cpu().numpy(), want)
    assert np.array_equal(_bits(ce.dequantize_rows(q)), R.dequant32(want).view(np.int32))
    idx = np.random.default_rng(width).integers(0, 77, 9 * 5)
    exact, bound = R.pooled64(want, idx, num_hots=5)
    got = ce.embedding_forward_quantized(q, torch.from_numpy(idx).to(DEV), num_hots=5, out_dtype=torch.float32)
    assert R.worst_ratio(got.cpu().numpy(), exact, bound) <= 1.0


def test_interop_with_torch_cpu_prepack(ce):
    """A table prepacked by torch on the CPU and copied over is the device-quantised table, byte for byte -- and
    therefore gives the same lookup bits."""
    for kind in ("f32", "f16"):
        x = _as_kind(_mixed_table(64), kind)
        theirs = torch.ops.quantized.embedding_bag_byte_prepack(x).to(DEV)
        ours = ce.quantize_rows(x.to(DEV))
        assert torch.equal(theirs, ours)
        idx = torch.randint(0, x.shape[0], (50 * 9,), device=DEV)
        a = ce.embedding_forward_quantized(theirs, idx, num_hots=9)
        b = ce.embedding_forward_quantized(ours, idx, num_hots=9)
        assert np.array_equal(_bits(a), _bits(b))
        # and torch's own CPU lookup on those bytes sits inside the bound around the same exact values
        off = torch.arange(0, idx.numel() + 1, 9)
        cpu = torch.ops.quantized.embedding_bag_byte_rowwise_offsets(theirs.cpu(), idx.cpu(), off, False, 0, False, None,
                                                                     None, True).numpy()
        exact, bound = R.pooled64(theirs.cpu().numpy(), idx.cpu().numpy(), num_hots=9)
        assert R.worst_ratio(cpu, exact, bound) <= 1.0


# ---- dequantizer and concat ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", R.WIDTHS)
def test_dequantizer_and_concat_are_bit_equal_to_the_two_rounding_recipe(ce, width):
    q_np = R.quantize(_mixed_table(width, rows_per_regime=60))
    q = torch.from_numpy(q_np).to(DEV)
    want32 = R.dequant32(q_np)
    with np.errstate(over="ignore"):          # (the lognormal and 1e4 rows exceed fp16: inf on both sides)
        want16 = want32.astype(np.float16)
    assert np.array_equal(_bits(ce.dequantize_rows(q)), want32.view(np.int32))
    assert np.array_equal(_bits(ce.dequantize_rows(q, dtype=torch.float16)), want16.view(np.int16))
    rng = np.random.default_rng(width)
    for idt in (torch.int32, torch.int64):
        ids_np = rng.integers(0, q_np.shape[0], (37, 5))
        ids = torch.from_numpy(ids_np).to(DEV, idt)
        got = ce.dequantize_rows(q, ids)
        assert tuple(got.shape) == (37, 5, width)
        assert np.array_equal(_bits(got), want32[ids_np].view(np.int32))
        assert np.array_equal(_bits(ce.dequantize_rows(q, ids, dtype=torch.float16)), want16[ids_np].view(np.int16))
        c32 = ce.embedding_forward_quantized(q, ids.view(-1), num_hots=5, mode="concat", out_dtype=torch.float32)
        c16 = ce.embedding_forward_quantized(q, ids.view(-1), num_hots=5, mode="concat")
        assert tuple(c32.shape) == (37, 5, width) and c16.dtype == torch.float16
        assert np.array_equal(_bits(c32), want32[ids_np].view(np.int32))
        assert np.array_equal(_bits(c16), want16[ids_np].view(np.int16))


# ---- forward against fp64 -------------------------------------------------------------------------------------------
def _ragged_offsets(rng, batch, hot):
    """Bag lengths in [0, 2 * hot] with empty bags among them (first, last and a few inside), one of exactly `hot`."""
    lengths = rng.integers(0, 2 * hot + 1, batch)
    lengths[[0, batch // 3, batch - 1]] = 0
    lengths[1] = hot
    lengths[2] = 2 * hot
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


@pytest.mark.parametrize("hot", HOTS)
@pytest.mark.parametrize("width", R.WIDTHS)
@pytest.mark.parametrize("layout", ["fixed", "csr", "csr_ordered"])
def test_forward_meets_the_bound_on_every_element(ce, layout, width, hot):
    """|got - exact| <= bound for every output element of every case: int32 / int64 indices and offsets x weighted or
    not x sum / mean x fp32 / fp16 output.  The data mixes all regimes (1e4-offset rows among N(0, 9) rows: large
    biases next to small ones); for fp16 output the mix is the tame one, whose sums fit the type.  Weights: U(-1, 1) for sum; for mean U(0.25, 1.25), because a weight sum near zero
    makes the mean itself ill-conditioned (its reciprocal amplifies the rounding of the weight sum without limit) and
    no fp32 implementation, the existing combiner included, could meet a bound that only allows one extra rounding."""
    rng = np.random.default_rng(1000 * width + hot)
    tables = {}
    for out, make in (("f32", _mixed_table), ("f16", _tame_table)):
        q = ce.quantize_rows(torch.from_numpy(make(width, rows_per_regime=100, seed=hot)).to(DEV))
        tables[out] = (q, q.cpu().numpy())
    rows = 400                                   # (ids below the smaller table's size)
    batch = 41
    if layout == "fixed":
        offsets_np = None
        nnz = batch * hot
    else:
        offsets_np = _ragged_offsets(rng, batch, hot)
        nnz = int(offsets_np[-1])
    idx_np = rng.integers(0, rows, nnz)
    order = None
    if layout == "csr_ordered":
        order = torch.from_numpy(rng.permutation(batch).astype(np.int32)).to(DEV)
    worst = 0.0
    for out in ("f32", "f16"):
        q, q_np = tables[out]
        for mode in ("sum", "mean"):
            for weighted in (False, True):
                w_np = None
                if weighted:
                    w_np = (rng.uniform(-1, 1, nnz) if mode == "sum" else rng.uniform(0.25, 1.25, nnz)).astype(_NP[out])
                exact, bound = R.pooled64(q_np, idx_np, offsets=offsets_np, num_hots=0 if offsets_np is not None else hot,
                                          weights=w_np, mode=mode, out=out)
                for idt in (torch.int32, torch.int64):
                    got = ce.embedding_forward_quantized(
                        q, torch.from_numpy(idx_np).to(DEV, idt),
                        offsets=None if offsets_np is None else torch.from_numpy(offsets_np).to(DEV, idt),
                        weights=None if w_np is None else torch.from_numpy(w_np).to(DEV),
                        num_hots=hot if offsets_np is None else 0, mode=mode, out_dtype=_TORCH[out], sample_order=order)
                    assert got.dtype == _TORCH[out] and tuple(got.shape) == (batch, width)
                    got_np = got.float().cpu().numpy()
                    assert np.isfinite(got_np).all()
                    ratio = R.worst_ratio(got_np, exact, bound)
                    worst = max(worst, ratio)
                    assert ratio <= 1.0, (layout, width, hot, out, mode, weighted, idt, ratio)
                    if offsets_np is not None:      # empty bags give zeros
                        empty = np.diff(offsets_np) == 0
                        assert empty.any() and not got_np[empty].any()
    print("worst |got - exact| / bound: %.3f (%s, W=%d, H=%d)" % (worst, layout, width, hot))


# (hotness, index type, weighted, output, width, lanes per row): a sample's indices (+ weights) exceed the 16 KiB staging
# budget, so the kernel reads them through the wavefront shuffle (lanes | 64) or from global memory (9 lanes)
UNSTAGED = [(1400, torch.int64, True, "f32", 64, 4), (1400, torch.int64, True, "f32", 36, 9),     # 12 B x 1400
            (1700, torch.int64, True, "f16", 64, 4), (1700, torch.int64, True, "f16", 36, 9),     # 10 B x 1700
            (4100, torch.int32, False, "f32", 256, 16), (4100, torch.int32, False, "f16", 256, 16)]   # 4 B x 4100


@pytest.mark.parametrize("hot,idt,weighted,out,width,lanes", UNSTAGED,
                         ids=lambda v: str(v).replace("torch.", "") if not isinstance(v, bool) else ("w" if v else "u"))
def test_fixed_hotness_too_long_to_stage(ce, hot, idt, weighted, out, width, lanes):
    """The fixed-hotness forward's two index sources besides LDS staging (begin = sample * num_hots): every element
    inside pooled64's bound, and bit-identical to the CSR form of the same bags.  fp16 output: mean, or a sum whose
    weights are scaled by 1 / H -- every exact value is checked to fit fp16 first."""
    batch = 5 if hot < 4000 else 3
    shape = ce.quantized_forward_launch_shape(idt, _TORCH[out], width, batch, hot, is_weighted=weighted, compute_units=0)
    assert shape["staged"] is False and shape["lanes_per_row"] == lanes and shape["lds_bytes"] == 0
    assert hot * (idt.itemsize + (_TORCH[out].itemsize if weighted else 0)) > 16 * 1024
    rng = np.random.default_rng(hot + width)
    q = ce.quantize_rows(torch.from_numpy(_tame_table(width, rows_per_regime=100, seed=hot)).to(DEV))
    q_np = q.cpu().numpy()
    idx_np = rng.integers(0, q_np.shape[0], batch * hot)
    idx = torch.from_numpy(idx_np).to(DEV, idt)
    off = torch.arange(0, batch * hot + 1, hot, device=DEV, dtype=idt)
    for mode in ("sum", "mean"):
        w_np = None
        if weighted:
            w_np = (rng.uniform(-1, 1, batch * hot) / (hot if out == "f16" else 1) if mode == "sum"
                    else rng.uniform(0.25, 1.25, batch * hot)).astype(_NP[out])
        elif out == "f16" and mode == "sum":
            continue                                  # (4,100 unweighted values of up to 31 do not fit fp16: mean only)
        exact, bound = R.pooled64(q_np, idx_np, num_hots=hot, weights=w_np, mode=mode, out=out)
        if out == "f16":
            assert np.abs(exact).max() < 65504.0       # finite in fp16, from the exact values alone
        w = None if w_np is None else torch.from_numpy(w_np).to(DEV)
        got = ce.embedding_forward_quantized(q, idx, num_hots=hot, weights=w, mode=mode, out_dtype=_TORCH[out])
        got_np = got.float().cpu().numpy()
        assert np.isfinite(got_np).all() and got_np.any()
        ratio = R.worst_ratio(got_np, exact, bound)
        print("worst |got - exact| / bound: %.3f (H=%d, W=%d, %s, %s)" % (ratio, hot, width, out, mode))
        assert ratio <= 1.0, (hot, width, out, mode, ratio)
        as_csr = ce.embedding_forward_quantized(q, idx, offsets=off, weights=w, mode=mode, out_dtype=_TORCH[out])
        assert np.array_equal(_bits(got), _bits(as_csr)), (hot, width, out, mode)


@pytest.mark.parametrize("out", ["f32", "f16"])
@pytest.mark.parametrize("width", [36, 256])
def test_weighted_mean_of_a_zero_weight_sum_is_zero(ce, width, out):
    """Pairs of +w, -w (representable in the weight type) sum to exactly zero in any fp32 order: the mean of such a bag
    is zeros, as the docstring promises, next to ordinary bags in the same batch -- fixed hotness and CSR."""
    rng = np.random.default_rng(width)
    q = ce.quantize_rows(torch.from_numpy(_tame_table(width, rows_per_regime=100, seed=5)).to(DEV))
    q_np = q.cpu().numpy()

    def weights_of(lengths, zero_bags):
        parts = []
        for s, n in enumerate(lengths):
            w = rng.uniform(0.25, 1.25, n).astype(_NP[out])
            if s in zero_bags:
                assert n % 2 == 0 and n > 0
                w[1::2] = -w[0::2]
            parts.append(w)
        return np.concatenate(parts)

    batch, hot = 12, 6
    layouts = [(np.full(batch, hot), {0, 5, 11}, None)]
    lengths = np.array([4, 0, 7, 2, 9, 6, 0, 1, 30, 3, 8, 2])
    layouts.append((lengths, {0, 3, 5, 8, 11}, np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)))
    for lengths, zero_bags, off_np in layouts:
        w_np = weights_of(lengths, zero_bags)
        assert w_np.dtype == _NP[out]
        idx_np = rng.integers(0, q_np.shape[0], int(lengths.sum()))
        exact, bound = R.pooled64(q_np, idx_np, offsets=off_np, num_hots=0 if off_np is not None else hot, weights=w_np,
                                  mode="mean", out=out)
        zero = np.zeros(batch, dtype=bool)
        zero[sorted(zero_bags)] = True
        assert not exact[zero].any() and exact[~zero & (lengths > 0)].any(axis=1).all()
        for idt in (torch.int32, torch.int64):
            got = ce.embedding_forward_quantized(
                q, torch.from_numpy(idx_np).to(DEV, idt), offsets=None if off_np is None else torch.from_numpy(off_np).to(DEV, idt),
                weights=torch.from_numpy(w_np).to(DEV), num_hots=0 if off_np is not None else hot, mode="mean",
                out_dtype=_TORCH[out])
            got_np = got.float().cpu().numpy()
            assert (got_np[zero] == 0.0).all(), (width, out, off_np is not None)          # exact zeros (of either sign)
            assert R.worst_ratio(got_np, exact, bound) <= 1.0
            assert got_np[~zero & (lengths > 0)].any(axis=1).all()


# ---- order and determinism, bit for bit ------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [36, 256, 512])
@pytest.mark.parametrize("weighted", [False, True])
def test_result_depends_on_nothing_but_the_bag(ce, width, weighted):
    rows, hot, big = 5000, 64, 65536
    q = ce.quantize_rows(torch.from_numpy(R.make_table("normal", rows, width, seed=1)).to(DEV))
    idx = torch.randint(0, rows, (big, hot), device=DEV, dtype=torch.int32)
    w = (torch.rand((big, hot), device=DEV) * 2 - 1).half() if weighted else None
    for mode in ("sum", "mean"):
        a = ce.embedding_forward_quantized(q, idx.view(-1), num_hots=hot, weights=w, mode=mode)
        # the same call twice
        assert torch.equal(a, ce.embedding_forward_quantized(q, idx.view(-1), num_hots=hot, weights=w, mode=mode))
        # fixed hotness against the CSR form of the same bags (both offset types, with and without a sample order)
        for odt in (torch.int32, torch.int64):
            off = torch.arange(0, big * hot + 1, hot, device=DEV, dtype=odt)
            assert torch.equal(a, ce.embedding_forward_quantized(q, idx.view(-1), offsets=off, weights=w, mode=mode))
        order = torch.randperm(big, device=DEV).int()
        assert torch.equal(a, ce.embedding_forward_quantized(q, idx.view(-1), offsets=off, weights=w, mode=mode,
                                                             sample_order=order))
        # a sample pooled in a batch of 64 against the same sample in the batch of 65,536 (other launch shapes)
        for lo in (0, 31337):
            small = ce.embedding_forward_quantized(q, idx[lo:lo + 64].reshape(-1), num_hots=hot, mode=mode,
                                                   weights=None if w is None else w[lo:lo + 64].contiguous())
            assert torch.equal(a[lo:lo + 64], small)
        # row loads: default against streaming against the device decision (both values of the word)
        for kw in (dict(row_loads="default"), dict(row_loads="streaming"),
                   dict(row_loads_device=torch.tensor([1, 0, 0, 0], dtype=torch.int32, device=DEV)),
                   dict(row_loads_device=torch.tensor([0, 0, 0, 0], dtype=torch.int32, device=DEV), row_loads="streaming")):
            assert torch.equal(a, ce.embedding_forward_quantized(q, idx.view(-1), num_hots=hot, weights=w, mode=mode, **kw))
    # fp32 output rounds the same sums once less
    a32 = ce.embedding_forward_quantized(q, idx.view(-1), num_hots=hot, out_dtype=torch.float32,
                                         weights=None if w is None else w.float())
    if not weighted:
        assert torch.equal(a32.half(), ce.embedding_forward_quantized(q, idx.view(-1), num_hots=hot))


def test_bag_module_applies_hints_without_changing_a_bit(ce):
    from cuembed_amd import policy
    rows, width, batch = 3000, 128, 20000
    table = torch.randn(rows, width, device=DEV).half()
    bag = ce.QuantizedEmbeddingBag.from_float(table)
    assert torch.equal(bag.qtable, ce.quantize_rows(table))
    lengths = torch.randint(0, 120, (batch,), device=DEV)
    off = torch.cat([torch.zeros(1, dtype=torch.long, device=DEV), lengths.cumsum(0)])
    idx = torch.randint(0, rows, (int(off[-1]),), device=DEV)
    assert idx.numel() >= policy.ORDER_MIN_LOOKUPS           # large enough for the bag order to be applied
    w = torch.rand(idx.numel(), device=DEV).half()
    plain = ce.embedding_forward_quantized(bag.qtable, idx, off, w)
    assert torch.equal(bag(idx, off, w), plain)
    assert torch.equal(ce.QuantizedEmbeddingBag(bag.qtable, hints=None)(idx, off, w), plain)
    assert torch.equal(bag.dequantize(idx[:10]), ce.dequantize_rows(bag.qtable, idx[:10]))


# ---- full size ---------------------------------------------------------------------------------------------------
def test_config2_full_size_against_fp64_on_the_device(ce):
    """10 M x 256 quantised on the device from an fp16 table, batch 65,536, hotness 64, alpha = 1.15 from the harness
    generator; all 65,536 output rows against the fp64 value of the fused bytes, computed with torch on the device in
    chunks of 1,024 samples."""
    from cuembed_amd import harness
    rows, width, batch, hot = 10_000_000, 256, 65536, 64
    table = torch.empty((rows, width), dtype=torch.float16, device=DEV).normal_(0, 3)
    q = ce.quantize_rows(table)
    # spot-check the quantizer at this size: the recipe on the first, a middle and the last rows
    for lo in (0, rows // 2 + 12345, rows - 1000):
        assert np.array_equal(q[lo:lo + 1000].cpu().numpy(), R.quantize(table[lo:lo + 1000].float().cpu().numpy()))
    del table
    idx = torch.from_numpy(harness.generate_indices(rows, batch, hot, alpha=1.15)).to(DEV)
    assert idx.numel() == batch * hot
    got = ce.embedding_forward_quantized(q, idx, num_hots=hot)
    assert got.dtype == torch.float16
    worst = torch.zeros((), dtype=torch.float64, device=DEV)
    for lo in range(0, batch, 1024):
        r = idx[lo * hot:(lo + 1024) * hot].long()
        fused = q[r].view(1024, hot, width + 8)
        codes = fused[:, :, :width].double()
        scale = fused[:, :, width:width + 4].contiguous().view(torch.float32).double()
        bias = fused[:, :, width + 4:].contiguous().view(torch.float32).double()
        exact = (codes * scale + bias).sum(1)
        bound = (hot + 2) * 2.0 ** -24 * (codes * scale + bias.abs()).sum(1) + 2.0 ** -11 * exact.abs() + 2.0 ** -25
        err = (got[lo:lo + 1024].double() - exact).abs()
        assert bool((err <= bound).all()), "rows %d..%d" % (lo, lo + 1024)
        worst = torch.maximum(worst, (err / bound).max())
    print("config 2, 65,536 rows: worst |got - exact| / bound = %.3f" % float(worst))


# ---- HIP graph -----------------------------------------------------------------------------------------------------
def test_forward_replays_from_a_hip_graph(ce):
    """One captured forward (no host read-back, no allocation inside the library), replayed three times on fresh
    indices and weights copied into the captured buffers: each replay equals the eager call."""
    rows, width, batch, hot = 20000, 256, 4096, 32
    q = ce.quantize_rows(torch.randn(rows, width, device=DEV))
    idx = torch.randint(0, rows, (batch * hot,), device=DEV, dtype=torch.int32)
    w = torch.rand(batch * hot, device=DEV).half()
    out = torch.empty((batch, width), dtype=torch.float16, device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ce.embedding_forward_quantized(q, idx, num_hots=hot, weights=w, mode="mean", out=out)    # warm-up: code loaded
        torch.cuda.current_stream().synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            ce.embedding_forward_quantized(q, idx, num_hots=hot, weights=w, mode="mean", out=out)
    torch.cuda.synchronize()
    for _ in range(3):
        idx.copy_(torch.randint(0, rows, (batch * hot,), device=DEV, dtype=torch.int32))
        w.copy_(torch.rand(batch * hot, device=DEV).half())
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        want = ce.embedding_forward_quantized(q, idx, num_hots=hot, weights=w, mode="mean")
        assert torch.equal(out, want)


# ---- torch ops ------------------------------------------------------------------------------------------------------
def _compiled(fn):
    def run(*a):
        try:
            return torch.compile(fn, fullgraph=True)(*a)
        except Exception as e:  # noqa: BLE001 - no working inductor toolchain on the box: trace with aot_eager instead
            print("inductor unavailable (%s): aot_eager" % type(e).__name__)
            torch._dynamo.reset()
            return torch.compile(fn, fullgraph=True, backend="aot_eager")(*a)
    return run


def test_torch_ops(ce):
    from cuembed_amd import cuembed_pyt as P
    ops = torch.ops.cuembed_pyt
    assert str(ops.quantize_rows.default._schema) == "cuembed_pyt::quantize_rows(Tensor table) -> Tensor"
    assert str(ops.dequantize_rows.default._schema) == (
        "cuembed_pyt::dequantize_rows(Tensor qtable, Tensor? ids, ScalarType dtype) -> Tensor")
    assert str(ops.cuemb_embedding_quantized.default._schema) == (
        "cuembed_pyt::cuemb_embedding_quantized(Tensor qtable, Tensor indices, Tensor? offsets, Tensor? weights, str mode, "
        "ScalarType out_dtype, int row_loads, Tensor? sample_order, Tensor? row_loads_device) -> Tensor")
    rows, width, batch, hot = 700, 64, 96, 6
    table = torch.randn(rows, width, device=DEV)
    q = P.quantize_rows(table)
    assert torch.equal(q, ce.quantize_rows(table))
    idx = torch.randint(0, rows, (batch, hot), device=DEV)
    assert torch.equal(P.dequantize_rows(q, idx, torch.float16), ce.dequantize_rows(q, idx, torch.float16))
    assert torch.equal(P.dequantize_rows(q), ce.dequantize_rows(q))
    w = torch.rand(batch * hot, device=DEV)
    # mixed index / offset dtypes, CSR and fixed hotness
    for idt in (torch.int32, torch.int64):
        for odt in (torch.int32, torch.int64):
            off = torch.arange(0, batch * hot + 1, hot, device=DEV, dtype=odt)
            flat = idx.view(-1).to(idt)
            for mode in ("sum", "mean"):
                want = ce.embedding_forward_quantized(q, flat, offsets=off, weights=w, mode=mode, out_dtype=torch.float32)
                assert torch.equal(P.cuemb_embedding_quantized(q, flat, off, w, mode, torch.float32), want)
                assert torch.equal(ops.cuemb_embedding_quantized(q, idx.to(idt), None, w, mode, torch.float32, -1, None,
                                                                 None), want)
    assert torch.equal(P.cuemb_embedding_quantized(q, idx, mode="concat"),
                       ce.embedding_forward_quantized(q, idx.view(-1), num_hots=hot, mode="concat"))
    # schema, fake kernel and real kernel agree on the output's metadata
    off = torch.arange(0, batch * hot + 1, hot, device=DEV)
    for op, args in [(ops.quantize_rows, (table.half(),)), (ops.dequantize_rows, (q, idx, torch.float16)),
                     (ops.dequantize_rows, (q, None, torch.float32)),
                     (ops.cuemb_embedding_quantized, (q, idx.view(-1), off, w.half(), "mean", torch.float16, 1, None, None)),
                     (ops.cuemb_embedding_quantized, (q, idx, None, None, "concat", torch.float32, -1, None, None))]:
        torch.library.opcheck(op, args, test_utils=("test_schema", "test_faketensor"))
    # torch.compile of a function that calls the lookup
    def fn(q, idx, off, w):
        return P.cuemb_embedding_quantized(q, idx, off, w, "sum", torch.float32) * 2.0

    want = ce.embedding_forward_quantized(q, idx.view(-1), offsets=off, weights=w, out_dtype=torch.float32) * 2.0
    assert torch.equal(_compiled(fn)(q, idx.view(-1), off, w), want)

    def roundtrip(t, ids):
        return P.dequantize_rows(P.quantize_rows(t), ids, torch.float32)

    assert torch.equal(_compiled(roundtrip)(table, idx), ce.dequantize_rows(q, idx))
    # rejections of the native ops are Python exceptions
    with pytest.raises(RuntimeError, match="uint8"):
        ops.dequantize_rows(table, None, torch.float32)
    with pytest.raises(RuntimeError, match="output's dtype"):
        ops.cuemb_embedding_quantized(q, idx.view(-1), off, w, "sum", torch.float16, -1, None, None)
    with pytest.raises(RuntimeError, match="mode"):
        ops.cuemb_embedding_quantized(q, idx.view(-1), off, None, "concat", torch.float16, -1, None, None)
