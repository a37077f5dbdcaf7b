"""embedding_weight_grad_grouped: the gradient of a group's weighted sum with respect to the per-lookup weights, in one
launch.

    bits        on arbitrary data the result equals num_tables calls of embedding_weight_grad on grad_y[:, t, :] made
                contiguous, concatenated in the group's layout: separate tables and a one-storage group, CSR and fixed
                hotness, int32 / int64 indices and offsets, the three lane widths and the three walks of the kernel;
    misaligned  one table 4 bytes into its storage narrows the whole group: exact data, where every order gives one result;
    fp64        |got - exact| <= exact_sums.weight_grad_bound, the bound the single-table kernel is held to;
    edges       an empty batch, all bags empty, 64 lookups of one row, out=;
    addressing  three 9 GiB tables as views of an untouched arena, rows past 2^31 elements and 2^32 bytes, every narrowed
                address poisoned (far_rows): a narrowing bug reads a wrong value and never faults.
"""
import numpy as np
import pytest
import torch

import exact_sums as X
import far_rows as F
import grouped_backward_cases as G
import grouped_cases as C
import grouped_train_reference as R

pytestmark = pytest.mark.gpu

T = len(C.ROWS)
INT32 = 1 << 31
MEMORY_CAP = 40 << 30
POISON = 0x3B


@pytest.fixture(scope="module")
def ce():
    import cuembed_amd
    assert torch.cuda.is_available()
    return cuembed_amd


@pytest.fixture(autouse=True)
def _no_error_left(ce):
    yield
    torch.cuda.synchronize()
    assert ce._lib.lib().cuembed_peek_last_error() == 0


def ibits(t):
    t = t.contiguous()
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()]).view(-1)


def values(kind, width):
    return [torch.from_numpy(C.table_values(t, rows, width)).cuda().to(G.DTYPES[kind]) for t, rows in enumerate(C.ROWS)]


def make_group(ce, tables, storage):
    if storage == "one":
        group = ce.TableGroup.from_flat(torch.cat(tables), C.ROWS)
        assert group.flat is not None
        return group
    return ce.TableGroup(tables)


def arbitrary_grad_y(kind, batch, width, seed):
    g = np.random.default_rng(seed).uniform(-1.0, 1.0, (batch, T, width)).astype(np.float32)
    return G.dev(g).to(G.DTYPES[kind])


def per_table(ce, tables, grad_y, batch, ids, offsets, hot):
    """num_tables calls of embedding_weight_grad on grad_y[:, t, :].contiguous(), concatenated in the group's layout."""
    parts = []
    for t in range(T):
        i_t, o_t, _ = G.table_problem(t, batch, ids, offsets, hot)
        g_t = grad_y[:, t, :].contiguous()
        if i_t.numel() == 0:
            parts.append(torch.zeros(0, dtype=grad_y.dtype, device="cuda"))
            continue
        parts.append(ce.embedding_weight_grad(tables[t], i_t, g_t, offsets=o_t, num_hots=hot).view(-1))
    return torch.cat(parts)


def lanes_of(group, grad_y, width):
    """(lane bytes, packs per row, lanes of a group) as EmbeddingWeightGradGrouped derives them from SplitRow."""
    lane = group.lane_bytes(grad_y.data_ptr())
    chunks = width * grad_y.element_size() // lane
    lanes = 1
    while lanes < chunks and lanes < 64:
        lanes *= 2
    return lane, chunks, lanes


def grouped_calls(ce, group, grad_y, batch, ids, offsets, hot):
    """The grouped result for every combination of index and offset dtype."""
    for idt in (np.int32, np.int64):
        if offsets is None:
            idx = G.dev(ids.astype(idt)).view(T, batch, hot)
            yield (idt.__name__,), ce.embedding_weight_grad_grouped(group, grad_y, idx, num_hots=hot), idx
            continue
        for odt in (np.int32, np.int64):
            idx = G.dev(ids.astype(idt))
            yield (idt.__name__, odt.__name__), ce.embedding_weight_grad_grouped(group, grad_y, idx,
                                                                                 G.dev(offsets.astype(odt))), idx


# (kind, width, lane bytes of aligned tables, walk): W = 64: 8 (fp16 / bf16) or 16 (fp32) lanes, the pipelined batches;
# W = 6 fp16: 12-byte rows, 3 lanes of 4 bytes, a lane group of 4 -- below 8, the fallback walk; W = 36 bf16: 72-byte
# rows, 9 lanes of 8 bytes in a group of 16 (masked lanes); W = 260 fp32: 65 lanes of 16 bytes -- more than 64, the strided walk
SHAPES = [("f32", 64, 16, "batches"), ("f16", 64, 16, "batches"), ("bf16", 64, 16, "batches"),
          ("f16", 6, 4, "fallback"), ("bf16", 36, 8, "batches"), ("f32", 260, 16, "strided")]


@pytest.mark.parametrize("storage", ["separate", "one"])
@pytest.mark.parametrize("kind,width,lane,walk", SHAPES, ids=["%s-W%d" % s[:2] for s in SHAPES])
def test_bits_of_num_tables_single_table_calls(ce, kind, width, lane, walk, storage):
    tables = values(kind, width)
    group = make_group(ce, tables, storage)
    for batch in C.BATCHES:
        grad_y = arbitrary_grad_y(kind, batch, width, 7 * batch + width)
        got_lane, chunks, lanes = lanes_of(group, grad_y, width)
        assert got_lane == lane, (got_lane, lane)          # a base a whole number of rows into an aligned storage never narrows
        assert {"batches": chunks <= lanes and lanes >= 8, "fallback": lanes < 8, "strided": chunks > lanes}[walk]
        for name, ids, offsets, hot, _ in C.layouts(batch):
            want = per_table(ce, tables, grad_y, batch, ids, offsets, hot)
            for dtypes, got, idx in grouped_calls(ce, group, grad_y, batch, ids, offsets, hot):
                assert got.shape == idx.shape and got.dtype == grad_y.dtype
                assert torch.equal(ibits(got), ibits(want)), (name, batch, dtypes)


@pytest.mark.parametrize("kind", ["f32", "f16", "bf16"])
def test_one_misaligned_table_narrows_the_whole_group(ce, kind):
    """Table 1 is a view 4 bytes into its storage: lanes of 4 bytes for the group, 16 for the single-table calls on the
    aligned copies.  Integer tables in [-2, 2] and exact_grad_y: every partial sum is an integer below 2^9 (bf16: one
    gradient in 16 is non-zero), exact in any order."""
    width, dtype = 64, G.DTYPES[kind]
    rng = np.random.default_rng(5)
    host = [rng.integers(-2, 3, (rows, width)).astype(np.float32) for rows in C.ROWS]
    tables = [G.dev(h).to(dtype) for h in host]
    shift = 4 // tables[1].element_size()
    storage = torch.zeros(C.ROWS[1] * width + shift, dtype=dtype, device="cuda")
    moved = storage[shift:].view(C.ROWS[1], width)
    moved.copy_(tables[1])
    assert moved.data_ptr() % 16 == 4 and moved.is_contiguous()
    group = ce.TableGroup([tables[0], moved, tables[2]])
    for batch in (5, 1023):
        gy = G.exact_grad_y(rng, batch, T, width, kind)
        grad_y = G.dev(gy).to(dtype)
        assert lanes_of(group, grad_y, width)[0] == 4
        for name, ids, offsets, hot, _ in C.layouts(batch):
            exact, _ = R.weight_grad64([h.astype(np.float64) for h in host], batch, ids, offsets, hot, gy)
            assert G.representable(kind, False, exact)
            want = per_table(ce, tables, grad_y, batch, ids, offsets, hot)
            assert np.array_equal(want.double().cpu().numpy(), exact), name
            for dtypes, got, _ in grouped_calls(ce, group, grad_y, batch, ids, offsets, hot):
                assert torch.equal(ibits(got), ibits(want)), (name, batch, dtypes)


@pytest.mark.parametrize("kind", ["f32", "f16", "bf16"])
def test_within_the_single_table_bound_of_fp64(ce, kind):
    width, batch = 64, 1023
    tables = values(kind, width)
    group = ce.TableGroup(tables)
    grad_y = arbitrary_grad_y(kind, batch, width, 99)
    tables64 = [t.double().cpu().numpy() for t in tables]
    for name, ids, offsets, hot, _ in C.layouts(batch):
        exact, scale = R.weight_grad64(tables64, batch, ids, offsets, hot, grad_y.double().cpu().numpy())
        bound = X.weight_grad_bound(kind, width, exact, scale)
        idx = G.dev(ids) if offsets is not None else G.dev(ids).view(T, batch, hot)
        got = ce.embedding_weight_grad_grouped(group, grad_y, idx, G.dev(offsets), num_hots=hot)
        err = np.abs(got.double().cpu().numpy().reshape(-1) - exact)
        worst = int(np.argmax(err - bound))
        assert np.all(err <= bound), (name, worst, err[worst], bound[worst])


def test_edges(ce):
    kind, width = "f16", 64
    tables = values(kind, width)
    group = ce.TableGroup(tables)
    # an empty batch
    empty = torch.zeros(0, dtype=torch.int64, device="cuda")
    got = ce.embedding_weight_grad_grouped(group, torch.zeros((0, T, width), dtype=torch.float16, device="cuda"), empty,
                                           torch.zeros(1, dtype=torch.int64, device="cuda"))
    assert got.shape == (0,) and got.dtype == torch.float16
    # all bags empty
    batch = 5
    grad_y = arbitrary_grad_y(kind, batch, width, 1)
    got = ce.embedding_weight_grad_grouped(group, grad_y, empty, torch.zeros(T * batch + 1, dtype=torch.int64, device="cuda"))
    assert got.shape == (0,)
    # a bag of 64 lookups of one row, between empty bags: 64 times the same dot product
    lengths = np.zeros((T, batch), dtype=np.int64)
    lengths[1, 2] = 64
    lengths[2, 4] = 3
    offsets = np.concatenate([[0], np.cumsum(lengths.reshape(-1))])
    ids = np.concatenate([np.full(64, 11), [0, 299, 7]])
    got = ce.embedding_weight_grad_grouped(group, grad_y, G.dev(ids), G.dev(offsets))
    want = per_table(ce, tables, grad_y, batch, ids, offsets, 0)
    assert torch.equal(ibits(got), ibits(want))
    assert bool((ibits(got)[:64] == ibits(got)[0]).all()) and float(got[0]) != 0.0
    one = (tables[1][11].float() * grad_y[2, 1].float()).double().sum()
    assert abs(float(got[0]) - float(one)) <= 2.0 ** -10 * abs(float(one)) + 1e-3
    # out=
    out = torch.full((ids.size,), -7.0, dtype=torch.float16, device="cuda")
    back = ce.embedding_weight_grad_grouped(group, grad_y, G.dev(ids), G.dev(offsets), out=out)
    assert back is out and torch.equal(ibits(out), ibits(want))


# ---- addressing: three tables far apart in one untouched arena -------------------------------------------------------------
@pytest.fixture(scope="module")
def arena():
    free, _ = torch.cuda.mem_get_info()
    if free < MEMORY_CAP:
        pytest.skip("the far-row test needs %d GiB of free device memory, %d GiB are free" % (MEMORY_CAP >> 30, free >> 30))
    a = torch.empty((F.ARENA_BYTES,), dtype=torch.uint8, device="cuda")       # never touched as a whole
    assert a.data_ptr() % 256 == 0
    yield a
    del a
    torch.cuda.empty_cache()


def tensor_of(arena, view, dtype):
    assert view.end <= arena.numel() and dtype.itemsize == view.elem_size
    t = arena[view.base:view.end].view(dtype).view(view.rows, view.width)
    assert t.data_ptr() == arena.data_ptr() + view.base and t.is_contiguous()
    return t


@pytest.mark.parametrize("kind,width", F.GROUPED_TABLES, ids=["%s-W%d" % c for c in F.GROUPED_TABLES])
def test_reads_far_rows_of_three_tables(ce, arena, kind, width):
    """Rows whose element offset passes 2^31 and 2^32 and whose byte offset passes 2^32 and 2^33, in three 9 GiB tables:
    the compact copies' single-table results, bit for bit.  The compact rows differ row by row and from the poison, so a
    narrowed address gives another dot product."""
    dtype = G.DTYPES[kind]
    views = F.grouped_views(F.ELEM_SIZE[kind], width)
    tables = [tensor_of(arena, v, dtype) for v in views]
    group = ce.TableGroup(tables)
    B = 5
    for idt in (np.int64, np.int32):
        layout, rows = F.pick(views, seed=41 + width, below=INT32 if idt == np.int32 else None)
        assert all(max(r) * width >= INT32 and max(r) * width * 2 >= (1 << 32) for r in rows)
        assert idt == np.int32 or all(max(r) * width >= (1 << 32) for r in rows)
        rng = np.random.default_rng(width)
        compacts = [G.dev(rng.uniform(-1, 1, (len(r), width)).astype(np.float32)).to(dtype) for r in rows]
        for a, n in layout.aliases:
            arena[a:a + n].fill_(POISON)
        for c in compacts:
            assert not bool((c.contiguous().view(torch.uint8).view(c.shape[0], -1) == POISON).all(dim=1).any())
        for t in range(T):
            for k, r in enumerate(rows[t]):
                tables[t][r].copy_(compacts[t][k])
        grad_y = G.dev(rng.uniform(-1, 1, (B, T, width)).astype(np.float32)).to(dtype)
        fixed = np.stack([F.fixed_bags(r, B, 3, width + t, idt).reshape(B, 3) for t, r in enumerate(rows)])
        got = ce.embedding_weight_grad_grouped(group, grad_y, G.dev(fixed), num_hots=3)
        want = torch.stack([ce.embedding_weight_grad(compacts[t], G.dev(F.compact(fixed[t].reshape(-1), rows[t])),
                                                     grad_y[:, t, :].contiguous(), num_hots=3).view(B, 3) for t in range(T)])
        assert torch.equal(ibits(got), ibits(want)), (idt.__name__, "fixed")
        lens = rng.integers(0, 9, T * B)
        lens[[0, 6, T * B - 1]] = 0
        lens[7] = 70
        off = np.concatenate([[0], np.cumsum(lens)])
        ids = np.concatenate([np.asarray(r, dtype=np.int64)[rng.integers(0, len(r), int(lens[t * B:(t + 1) * B].sum()))]
                              for t, r in enumerate(rows)]).astype(idt)
        for odt in (np.int64, np.int32):
            got = ce.embedding_weight_grad_grouped(group, grad_y, G.dev(ids), G.dev(off.astype(odt)))
            per = []
            for t in range(T):
                lo, hi = int(off[t * B]), int(off[(t + 1) * B])
                per.append(ce.embedding_weight_grad(compacts[t], G.dev(F.compact(ids[lo:hi], rows[t])),
                                                    grad_y[:, t, :].contiguous(),
                                                    offsets=G.dev((off[t * B:(t + 1) * B + 1] - lo).astype(odt))))
            assert torch.equal(ibits(got), ibits(torch.cat(per))), (idt.__name__, "csr", odt.__name__)
