"""GPU parity of the 4-bit mixed-width forward (one launch for a group of fused 4-bit tables of DIFFERENT widths):
torch.equal against torch.cat of T calls of embedding_forward_quantized(bits=4), and per table slice the fp64 bound of
quantized_4bit_reference.pooled64.

The groups are the smallest at which each path of the kernel can go wrong (tables of 7 to 1,000 rows):
    A (32, 256, 64, 128)    N = 32; 1, 8, 2, 4 lanes per bag: the cross-lane walk (a 20-byte row pitch puts the 16-byte
                            loads at every 4-byte alignment)
    B (16, 48, 272)         N = 16; 1, 3, 17 lanes: the broadcast walk (3 and 17 do not divide 64)
    C (8, 24, 2056, 40)     N = 8; 257 lanes: the column loop, a second pass of one lane
    D (8224, 32)            N = 32; 257 lanes: the column loop at the widest lane (the single-table call takes N = 16)
B in (1, 67, 300): partial last workgroups, several workgroups per table, more bags of a one-lane table than a workgroup
holds.  CSR bag lengths from {0, 1, 3, 4, 5, 7, 8, 9, 17, 70}: empty bags, both sides of the batches of 4 and 8 lookups
and their tails, a bag longer than a chunk of 64 lanes.  H = 9 with a one-lane table is 256 bags per workgroup: staged
with int32 ids (9,216 bytes; 13,824 with fp16 weights), not staged with int64 ids or with int32 ids and fp32 weights
(18,432 bytes)."""
import numpy as np
import pytest
import torch

from quantized_4bit_reference import pooled64, quantize
from quantized_reference import make_table, worst_ratio

pytestmark = pytest.mark.gpu

ROWS = (1000, 7, 300, 64)
REGIMES = ("normal", "offset", "constant", "uniform")         # "offset" moved to 30 + U(-1, 1): sums of 70 rows fit fp16
GROUPS = {"A": (32, 256, 64, 128), "B": (16, 48, 272), "C": (8, 24, 2056, 40), "D": (8224, 32)}
CODES = {"A": 32, "B": 16, "C": 8, "D": 32}
LENGTHS = (0, 1, 3, 4, 5, 7, 8, 9, 17, 70)
F16, F32, I32, I64 = torch.float16, torch.float32, torch.int32, torch.int64
# (group, B, H or 0 for CSR, mode, weighted, out dtype, index dtype, offset dtype)
CASES = [
    ("A", 1, 0, "sum", False, F16, I32, I32), ("A", 67, 0, "mean", True, F32, I64, I64),
    ("A", 300, 0, "sum", True, F16, I32, I64), ("A", 300, 9, "sum", False, F16, I32, I32),
    ("A", 300, 9, "mean", False, F32, I64, I32), ("A", 300, 9, "mean", True, F32, I32, I32),
    ("A", 67, 70, "sum", False, F32, I64, I32), ("A", 67, 1, "mean", False, F16, I64, I32),
    ("B", 67, 0, "mean", False, F16, I32, I32), ("B", 300, 9, "sum", True, F32, I64, I32),
    ("B", 1, 0, "sum", True, F32, I32, I64), ("C", 1, 0, "mean", True, F32, I64, I32),
    ("C", 67, 0, "sum", False, F32, I32, I64), ("C", 300, 0, "mean", True, F16, I32, I32),
    ("C", 300, 9, "mean", True, F16, I32, I32), ("C", 67, 70, "sum", True, F16, I64, I32),
    ("D", 67, 0, "sum", True, F16, I64, I64), ("D", 1, 9, "mean", False, F32, I32, I32),
]


@pytest.fixture(scope="module")
def ce():
    import cuembed_amd
    assert torch.cuda.is_available()
    return cuembed_amd


_GROUPS = {}


def group_of(ce, name):
    """(fp32 tables and their fused bytes on the host, the group), made once per name and never changed."""
    if name not in _GROUPS:
        data = [make_table(REGIMES[t], ROWS[t], w, seed=10 + t) for t, w in enumerate(GROUPS[name])]
        data[1] = data[1] - np.float32(1e4 - 30.0)
        host = [quantize(x) for x in data]
        group = ce.QuantizedMixedTableGroup([torch.from_numpy(q).cuda() for q in host], bits=4)
        assert group.bits == 4 and group.widths == GROUPS[name] and group.codes_per_lane() == CODES[name]
        _GROUPS[name] = (data, host, group)
    return _GROUPS[name]


def draw_batch(widths, batch, hot, weight_dtype, seed, mode="sum"):
    """(ids [nnz] int64, offsets [T * B + 1] int64 or None, weights [nnz], the offsets in any case) on the host; the ids
    of table t's bags are rows of table t.  CSR: bag 0 has 70 lookups and, where there is one, bag 1 none.  Weights of
    either sign for a sum; positive ones for a mean: pooled64's bound takes the weight sum as exact, which a sum that
    cancels is not in fp32."""
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


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-b%d-h%d-%s-%s" % (c[0], c[1], c[2], c[3], "w" if c[4] else "u"))
def test_group_call_has_the_bits_of_single_table_calls_and_holds_the_fp64_bound(ce, case):
    name, batch, hot, mode, weighted, out_dtype, index_dtype, offset_dtype = case
    _, host, group = group_of(ce, name)
    widths, T, D = GROUPS[name], len(GROUPS[name]), sum(GROUPS[name])
    ids, offsets, weights, all_offsets = draw_batch(widths, batch, hot, out_dtype, batch + hot, mode)
    if hot == 9:     # both branches of the staging decision run
        most = max(256 // min(w // CODES[name], 256) for w in widths)
        staged = most * 9 * (index_dtype.itemsize + (out_dtype.itemsize if weighted else 0)) <= 16384
        shape = ce.quantized_mixed_group_launch_shape(out_dtype, index_dtype, widths, batch, hot, weighted, bits=4)
        assert shape["staged"] == staged and shape["codes_per_lane"] == CODES[name]
        assert shape["max_bags_per_block"] == most and shape["embedding_dim"] == D
    d_ids = torch.from_numpy(ids).to(index_dtype).cuda()
    d_off = None if hot else torch.from_numpy(offsets).to(offset_dtype).cuda()
    d_w = weights.cuda() if weighted else None
    kw = dict(num_hots=hot, mode=mode, out_dtype=out_dtype)
    got = ce.embedding_forward_quantized_mixed_group(group, d_ids, d_off, d_w, **kw)
    assert got.shape == (batch, D) and got.dtype == out_dtype and got.is_contiguous()
    singles = []
    for t in range(T):
        lo, hi = int(all_offsets[t * batch]), int(all_offsets[(t + 1) * batch])
        i, o, w = ids[lo:hi], all_offsets[t * batch:(t + 1) * batch + 1] - lo, weights[lo:hi]
        singles.append(ce.embedding_forward_quantized(
            group.tables[t], torch.from_numpy(i).to(index_dtype).cuda(),
            None if hot else torch.from_numpy(o).to(offset_dtype).cuda(), w.cuda() if weighted else None,
            batch_size=batch, bits=4, **kw))
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


def test_torch_op_graph_replay_and_repairing_module(ce):
    from cuembed_amd import cuembed_pyt as P
    data, _, group = group_of(ce, "A")
    widths, batch, T = GROUPS["A"], 67, len(GROUPS["A"])
    ids, offsets, weights, _ = draw_batch(widths, batch, 0, F16, 3, "mean")
    idx, off, d_w = torch.from_numpy(ids).cuda(), torch.from_numpy(offsets).cuda(), weights.cuda()
    want = ce.embedding_forward_quantized_mixed_group(group, idx, off, d_w, mode="mean")
    assert torch.equal(P.cuemb_embedding_quantized_mixed_group(group, idx, off, d_w, mode="mean"), want)
    torch.library.opcheck(torch.ops.cuembed_pyt.cuemb_embedding_quantized_mixed_group_4bit,
                          (list(group.tables), group.table_ptrs, group.descriptor(batch, 32), 32, idx, off, d_w, "mean",
                           F16, -1), test_utils=("test_schema", "test_faketensor"))
    # ---- one captured call replays to the eager bits after the ids changed in place
    out = torch.empty((batch, sum(widths)), dtype=F16, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ce.embedding_forward_quantized_mixed_group(group, idx, off, d_w, mode="mean", out=out)     # warm-up, descriptor
        torch.cuda.current_stream().synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            ce.embedding_forward_quantized_mixed_group(group, idx, off, d_w, mode="mean", out=out)
    torch.cuda.synchronize()
    for seed in (6, 7, 8):                   # the offsets stay; the ids are redrawn per table
        rng = np.random.default_rng(seed)
        fresh = np.concatenate([rng.integers(0, ROWS[t], int(offsets[(t + 1) * batch] - offsets[t * batch]))
                                for t in range(T)])
        idx.copy_(torch.from_numpy(fresh).cuda())
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, ce.embedding_forward_quantized_mixed_group(group, idx, off, d_w, mode="mean")), seed
    # ---- the module quantizes on the device and repairs an id at its table's row count to row 0
    fixed, _, _, _ = draw_batch(widths, batch, 5, F16, seed=4)
    bad = torch.from_numpy(fixed).view(T, batch, 5).cuda()
    bad[1, 2, 3] = ROWS[1]                                           # (valid for table 0)
    repaired = bad.clone()
    repaired[1, 2, 3] = 0
    bags = ce.QuantizedMixedEmbeddingBagGroup.from_float([torch.from_numpy(x).cuda() for x in data], bits=4,
                                                         out_dtype=F32, bounds_check="repair")
    assert bags.bits == 4 and all(torch.equal(a, b) for a, b in zip(bags.group.tables, group.tables))
    assert torch.equal(bags(bad), ce.embedding_forward_quantized_mixed_group(group, repaired, num_hots=5, out_dtype=F32))
