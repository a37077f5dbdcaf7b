"""GPU parity of the quantized mixed-width forward (one launch for a group of fused 8-bit tables of DIFFERENT widths):
torch.equal against torch.cat of T calls of embedding_forward_quantized, and per table slice the fp64 bound of
quantized_reference.pooled64.

The groups are the smallest at which each path of the kernel can go wrong (tables of 7 to 1,000 rows):
    A (16, 128, 32, 64)     N = 16; 1, 8, 2, 4 lanes per bag: the cross-lane walk
    B (8, 24, 136)          N = 8; 1, 3, 17 lanes: the broadcast walk (3 and 17 do not divide 64)
    C (4, 12, 1028, 36)     N = 4; 257 lanes: the column loop, a second pass of one lane
    D (4112, 16)            N = 16; 257 lanes: the column loop at the wide lane
    E                       A's tables, one inside a byte buffer at a 4-byte offset: the launch narrowed to N = 4
B in (1, 67, 300): partial last workgroups, several workgroups per table, more bags of a one-lane table than a workgroup
holds.  CSR bag lengths from {0, 1, 3, 4, 5, 8, 9, 17, 70}: empty bags, both unroll boundaries, a bag longer than a chunk
of 64 lanes.  H = 9 with a one-lane table is 256 bags per workgroup: staged with int32 ids (9,216 bytes), not staged with
int64 ids or with int32 ids and fp32 weights (18,432 bytes)."""
import ctypes

import numpy as np
import pytest
import torch

from quantized_reference import make_table, pooled64, quantize, worst_ratio

pytestmark = pytest.mark.gpu

ROWS = (1000, 7, 300, 64)
REGIMES = ("normal", "offset", "lognormal", "uniform")        # "offset": biases of 1e4 under codes of 1e-2
TAME = ("normal", "offset", "constant", "uniform")            # fp16 results: biases of 30, no lognormal(0, 3) (values of 1e5)
GROUPS = {"A": (16, 128, 32, 64), "B": (8, 24, 136), "C": (4, 12, 1028, 36), "D": (4112, 16), "E": (16, 128, 32, 64)}
CODES = {"A": 16, "B": 8, "C": 4, "D": 16, "E": 4}
LENGTHS = (0, 1, 3, 4, 5, 8, 9, 17, 70)
F16, F32, I32, I64 = torch.float16, torch.float32, torch.int32, torch.int64
# (group, B, H or 0 for CSR, mode, weighted, out dtype, index dtype, offset dtype)
CASES = [
    ("A", 1, 0, "sum", False, F16, I32, I32), ("A", 67, 0, "mean", True, F32, I64, I64),
    ("A", 300, 0, "sum", True, F16, I32, I64), ("A", 300, 9, "sum", False, F16, I32, I32),
    ("A", 300, 9, "mean", True, F32, I32, I32), ("A", 67, 70, "sum", False, F32, I64, I32),
    ("A", 67, 1, "mean", False, F16, I64, I32), ("B", 67, 0, "mean", False, F16, I32, I32),
    ("B", 300, 9, "sum", True, F32, I64, I32), ("C", 1, 0, "mean", True, F32, I64, I32),
    ("C", 67, 0, "sum", False, F32, I32, I64), ("C", 300, 0, "mean", True, F16, I32, I32),
    ("C", 300, 9, "mean", False, F16, I32, I32), ("C", 300, 9, "sum", True, F16, I64, I32),
    ("C", 67, 70, "mean", True, F16, I32, I32), ("C", 67, 1, "sum", False, F32, I32, I32),
    ("D", 67, 0, "sum", True, F16, I64, I64), ("D", 1, 9, "mean", False, F32, I32, I32),
    ("E", 67, 0, "mean", True, F16, I32, I32), ("E", 300, 9, "sum", False, F32, I32, I32),
]


@pytest.fixture(scope="module")
def ce():
    import cuembed_amd
    assert torch.cuda.is_available()
    return cuembed_amd


_GROUPS = {}


def group_of(ce, name, tame=False):
    """(fused tables on the host, the group), made once per (name, tame) and never changed.  tame: sums of 70 weighted
    rows stay inside fp16's range."""
    key = (name, tame)
    if key not in _GROUPS:
        data = [make_table((TAME if tame else REGIMES)[t], ROWS[t], w, seed=10 + t) for t, w in enumerate(GROUPS[name])]
        if tame:
            data[1] = data[1] - np.float32(1e4 - 30.0)
        host = [quantize(x) for x in data]
        dev = [torch.from_numpy(q).cuda() for q in host]
        if name == "E":
            buf = torch.zeros(dev[2].numel() + 64, dtype=torch.uint8, device="cuda")
            first = (4 - buf.data_ptr()) % 16
            dev[2] = buf[first:first + dev[2].numel()].view(dev[2].shape).copy_(dev[2])
            assert dev[2].data_ptr() % 8 == 4
        _GROUPS[key] = (host, ce.QuantizedMixedTableGroup(dev))
        assert _GROUPS[key][1].codes_per_lane() == CODES[name]
    return _GROUPS[key]


def draw_batch(widths, batch, hot, weight_dtype, seed, mode="sum"):
    """(ids [nnz] int64, offsets [T * B + 1] int64 or None, weights [nnz], the offsets in any case) on the host; the ids
    of table t's bags are rows of table t.  CSR: bag 0 has 70 lookups and, where there is one, bag 1 none.  Weights of
    either sign for a sum; positive ones for a mean, as in test_gpu_quantized.py: pooled64's bound takes the weight sum
    as exact, which a sum that cancels is not in fp32."""
    rng = np.random.default_rng(seed)
    T = len(widths)
    lengths = np.full(T * batch, hot) if hot else rng.choice(LENGTHS, T * batch)
    if not hot:
        lengths[0] = 70
        lengths[1:2] = 0
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    ids = np.concatenate([rng.integers(0, ROWS[t], offsets[(t + 1) * batch] - offsets[t * batch]) for t in range(T)])
    low, high = (-1.0, 2.0) if mode == "sum" else (0.25, 1.25)
    weights = torch.from_numpy(rng.uniform(low, high, ids.size).astype(np.float32)).to(weight_dtype)
    return ids.astype(np.int64), (None if hot else offsets), weights, offsets


def per_table(t, batch, ids, weights, all_offsets):
    lo, hi = int(all_offsets[t * batch]), int(all_offsets[(t + 1) * batch])
    return ids[lo:hi], all_offsets[t * batch:(t + 1) * batch + 1] - lo, weights[lo:hi]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-b%d-h%d-%s-%s" % (c[0], c[1], c[2], c[3], "w" if c[4] else "u"))
def test_group_call_has_the_bits_of_single_table_calls_and_holds_the_fp64_bound(ce, case):
    name, batch, hot, mode, weighted, out_dtype, index_dtype, offset_dtype = case
    host, group = group_of(ce, name, tame=out_dtype == F16)
    widths, T, D = GROUPS[name], len(GROUPS[name]), sum(GROUPS[name])
    ids, offsets, weights, all_offsets = draw_batch(widths, batch, hot, out_dtype, batch + hot, mode)
    if hot == 9:     # both branches of the staging decision run
        staged = 256 * 9 * (index_dtype.itemsize + (out_dtype.itemsize if weighted else 0)) <= 16384
        shape = ce.quantized_mixed_group_launch_shape(out_dtype, index_dtype, widths, batch, hot, weighted,
                                                      4 if name == "E" else 0)
        assert shape["staged"] == staged and shape["codes_per_lane"] == CODES[name]
    d_ids = torch.from_numpy(ids).to(index_dtype).cuda()
    d_off = None if hot else torch.from_numpy(offsets).to(offset_dtype).cuda()
    d_w = weights.cuda() if weighted else None
    kw = dict(num_hots=hot, mode=mode, out_dtype=out_dtype)
    got = ce.embedding_forward_quantized_mixed_group(group, d_ids, d_off, d_w, **kw)
    assert got.shape == (batch, D) and got.dtype == out_dtype and got.is_contiguous()
    singles = []
    for t in range(T):
        i, o, w = per_table(t, batch, ids, weights, all_offsets)
        singles.append(ce.embedding_forward_quantized(
            group.tables[t], torch.from_numpy(i).to(index_dtype).cuda(),
            None if hot else torch.from_numpy(o).to(offset_dtype).cuda(), w.cuda() if weighted else None,
            batch_size=batch, **kw))
        exact, bound = pooled64(host[t], i, None if hot else o, hot, w.double().numpy() if weighted else None, mode,
                                "f16" if out_dtype == F16 else "f32")
        assert out_dtype == F32 or np.abs(exact).max() < 65504.0       # finite in fp16, from the exact values alone
        c = group.column_base[t]
        ratio = worst_ratio(got[:, c:c + widths[t]].double().cpu().numpy(), exact, bound)
        print("table %d: worst |error| / bound = %.3f" % (t, ratio))
        assert ratio <= 1.0, (t, ratio)
    assert torch.equal(got, torch.cat(singles, dim=1))
    assert torch.equal(ce.embedding_forward_quantized_mixed_group(group, d_ids, d_off, d_w, row_loads="streaming", **kw), got)
    out = torch.full((batch, D), float("nan"), dtype=out_dtype, device="cuda")
    assert ce.embedding_forward_quantized_mixed_group(group, d_ids, d_off, d_w, out=out, **kw) is out
    assert torch.equal(out, got)                                     # (NaN != NaN: every element was overwritten)
    if not hot and batch > 1:
        assert not bool(out[1, :widths[0]].any())                    # the empty bag (table 0, sample 1) reads as zeros


@pytest.mark.parametrize("name", ["A", "C"])
def test_torch_op_and_module_return_the_same_tensor(ce, name):
    from cuembed_amd import cuembed_pyt as P
    _, group = group_of(ce, name, tame=True)
    widths, batch, T = GROUPS[name], 67, len(GROUPS[name])
    ids, offsets, weights, _ = draw_batch(widths, batch, 0, F16, 3, "mean")
    d_ids, d_off, d_w = torch.from_numpy(ids).cuda(), torch.from_numpy(offsets).cuda(), weights.cuda()
    want = ce.embedding_forward_quantized_mixed_group(group, d_ids, d_off, d_w, mode="mean")
    assert torch.equal(P.cuemb_embedding_quantized_mixed_group(group, d_ids, d_off, d_w, mode="mean"), want)
    bags = ce.QuantizedMixedEmbeddingBagGroup(group, mode="mean", bounds_check="raise")
    assert torch.equal(bags(d_ids, d_off, d_w), want) and bags.last_check is not None
    fixed, _, _, _ = draw_batch(widths, batch, 5, F16, seed=4)
    d_fixed = torch.from_numpy(fixed).view(T, batch, 5).cuda()
    want = ce.embedding_forward_quantized_mixed_group(group, d_fixed, num_hots=5, out_dtype=F32)
    assert torch.equal(P.cuemb_embedding_quantized_mixed_group(group, d_fixed, out_dtype=F32), want)
    bad = d_fixed.clone()
    bad[1, 2, 3] = ROWS[1]                                           # at table 1's row count (valid for table 0)
    repaired = bad.clone()
    repaired[1, 2, 3] = 0
    repairing = ce.QuantizedMixedEmbeddingBagGroup(group, out_dtype=F32, bounds_check="repair")
    assert torch.equal(repairing(bad), ce.embedding_forward_quantized_mixed_group(group, repaired, num_hots=5,
                                                                                  out_dtype=F32))
    with pytest.raises(IndexError):
        ce.QuantizedMixedEmbeddingBagGroup(group, bounds_check="raise")(bad)


def test_one_call_under_graph_capture_is_one_kernel_node(ce):
    """The descriptor is built before the capture; the indices are rewritten in place between replays."""
    _, group = group_of(ce, "A", tame=True)
    widths, batch = GROUPS["A"], 67
    ids, offsets, _, _ = draw_batch(widths, batch, 0, F16, seed=5)
    idx, off = torch.from_numpy(ids).cuda(), torch.from_numpy(offsets).cuda()
    out = torch.empty((batch, sum(widths)), dtype=F16, device="cuda")
    group.descriptor(batch, group.codes_per_lane())

    def step():
        ce.embedding_forward_quantized_mixed_group(group, idx, off, mode="mean", out=out)

    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        step()                               # warm-up outside capture (module loading)
        torch.cuda.current_stream().synchronize()
        g = torch.cuda.CUDAGraph(keep_graph=True)
        with torch.cuda.graph(g, stream=s):
            step()
    hip = ce._lib.lib()                      # (the HIP runtime's symbols resolve through the library that links it)
    hip.hipGraphGetNodes.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t)]
    hip.hipGraphNodeGetType.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]
    count, node, kind = ctypes.c_size_t(0), ctypes.c_void_p(), ctypes.c_int(-1)
    assert hip.hipGraphGetNodes(ctypes.c_void_p(g.raw_cuda_graph()), None, ctypes.byref(count)) == 0 and count.value == 1
    assert hip.hipGraphGetNodes(ctypes.c_void_p(g.raw_cuda_graph()), ctypes.byref(node), ctypes.byref(count)) == 0
    assert hip.hipGraphNodeGetType(node, ctypes.byref(kind)) == 0 and kind.value == 0      # hipGraphNodeTypeKernel
    for seed in (6, 7, 8):                   # the offsets stay; the ids are redrawn per table
        rng = np.random.default_rng(seed)
        fresh = np.concatenate([rng.integers(0, ROWS[t], int(offsets[(t + 1) * batch] - offsets[t * batch]))
                                for t in range(len(widths))])
        idx.copy_(torch.from_numpy(fresh).cuda())
        out.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, ce.embedding_forward_quantized_mixed_group(group, idx, off, mode="mean")), seed
