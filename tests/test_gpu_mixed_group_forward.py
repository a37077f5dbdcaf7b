"""GPU parity of the mixed-width grouped forward (one launch for a group of tables of DIFFERENT widths): torch.equal on
integer views against torch.cat of T single-table calls of embedding_forward, and against the CPU oracle called once per
table.

What is new in the kernel is the table of a workgroup, the lanes of a bag as a run-time value, the column base of the
store and rows wider than a workgroup; the groups below are the smallest at which each can go wrong (tables of 5,000, 17,
300 and 64 rows, B in {1, 5, 1,023}: 1,023 leaves a partial last workgroup in every table)."""
import numpy as np
import pytest
import torch

import grouped_cases as C

pytestmark = pytest.mark.gpu

ROWS = (5000, 17, 300, 64)
KINDS = ("f32", "f16", "bf16")
DTYPE = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
INT = {"i32": (np.int32, torch.int32), "i64": (np.int64, torch.int64)}
SENTINEL = 0x5A
# widths -> lane bytes per kind (what the group's widths alone allow on aligned buffers)
GROUPS = {
    (128, 16, 64, 32): {"f32": 16, "f16": 16, "bf16": 16},   # bag groups of 16, 2, 8 and 4 lanes next to each other (16-bit)
    (36, 4, 128): {"f32": 16, "f16": 8, "bf16": 8},          # 16-bit: a 9-lane group (broadcast walk), 1 lane, 32 lanes
    (6, 2, 10): {"f32": 8, "f16": 4, "bf16": 4},
    (512, 8): {"f32": 16, "f16": 16, "bf16": 16},            # a whole wavefront per bag beside one-lane bags (16-bit)
    (36, 36, 36): {"f32": 16, "f16": 8, "bf16": 8},
    (128,): {"f32": 16, "f16": 16, "bf16": 16},
}


@pytest.fixture(scope="module")
def ce():
    import cuembed_amd
    assert torch.cuda.is_available()
    return cuembed_amd


def to_kind(oracle, kind, a):
    """fp32 values -> (the oracle's array of `kind`, the same elements on the device)."""
    a32 = np.ascontiguousarray(a, dtype=np.float32)
    if kind == "f32":
        return a32, torch.from_numpy(a32).cuda()
    if kind == "f16":
        h = a32.astype(np.float16)
        return h, torch.from_numpy(h).cuda()
    b = oracle.to_bf16_bits(a32)
    return b, torch.from_numpy(b.view(np.int16)).cuda().view(torch.bfloat16)


def ibits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


def host_bits(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view({2: np.int16, 4: np.int32}[a.dtype.itemsize]))


_TABLES = {}


def tables_of(oracle, kind, widths):
    """(oracle arrays, device tensors) of a group, made once per (kind, widths) and never changed."""
    key = (kind, widths)
    if key not in _TABLES:
        _TABLES[key] = tuple(zip(*[to_kind(oracle, kind, C.table_values(t, ROWS[t], w)) for t, w in enumerate(widths)]))
    return _TABLES[key]


def oracle_cat(oracle, host_tables, batch, ids, offsets, hot, weights, mode):
    """[B, D]: oracle.embedding_forward once per table, concatenated on dim 1 (numpy in, numpy out)."""
    per_table = []
    for t, table in enumerate(host_tables):
        i, o, w = C.table_slice(t, batch, ids, offsets, hot, ids if weights is None else weights)
        per_table.append(oracle.embedding_forward(table, i.astype(np.int32), None if o is None else o.astype(np.int32),
                                                  None if weights is None else w, batch_size=batch, num_hots=hot,
                                                  mode=mode))
    return np.concatenate(per_table, axis=1)


def single_table_cat(ce, dev_tables, batch, ids, offsets, hot, d_weights, mode):
    """[B, D]: torch.cat of T calls of ce.embedding_forward (numpy ids / offsets, device tables and weights)."""
    per_table = []
    for t, table in enumerate(dev_tables):
        i, o, _ = C.table_slice(t, batch, ids, offsets, hot, ids)
        lo = t * batch * hot if offsets is None else int(offsets[t * batch])
        w = None if d_weights is None else d_weights[lo:lo + i.size].contiguous()
        per_table.append(ce.embedding_forward(table, torch.from_numpy(np.ascontiguousarray(i)).cuda(),
                                              None if o is None else torch.from_numpy(np.ascontiguousarray(o)).cuda(), w,
                                              batch_size=batch, num_hots=hot, mode=mode))
    return torch.cat(per_table, dim=1)


def run_all_layouts(ce, oracle, kind, widths, batch, lane=None):
    host_tables, dev_tables = tables_of(oracle, kind, widths)
    group = ce.MixedTableGroup(dev_tables)
    T, D = len(widths), sum(widths)
    assert group.embedding_dim == D and group.widths == tuple(widths)
    checked = 0
    for name, ids, offsets, hot, w32 in C.layouts(batch, ROWS[:T]):
        w_host, w_dev = to_kind(oracle, kind, w32)
        types = [(i, o) for i in INT for o in INT] if offsets is not None else [(i, "i32") for i in INT]
        for mode, weighted in C.MODES:
            want = host_bits(oracle_cat(oracle, host_tables, batch, ids, offsets, hot, w_host if weighted else None, mode))
            assert tuple(want.shape) == (batch, D)
            cat = single_table_cat(ce, dev_tables, batch, ids, offsets, hot, w_dev if weighted else None, mode)
            for it, ot in types:
                d_ids = torch.from_numpy(ids.astype(INT[it][0])).cuda()
                d_off = None if offsets is None else torch.from_numpy(offsets.astype(INT[ot][0])).cuda()
                got = ce.embedding_forward_mixed_group(group, d_ids, d_off, w_dev if weighted else None, batch_size=batch,
                                                       num_hots=hot, mode=mode)
                assert got.shape == (batch, D) and got.is_contiguous() and got.dtype == DTYPE[kind]
                if lane is not None:
                    assert group.lane_bytes(got.data_ptr()) == lane
                assert torch.equal(ibits(got), ibits(cat)), (name, mode, weighted, it, ot, "vs single-table calls")
                assert torch.equal(ibits(got).cpu(), want), (name, mode, weighted, it, ot, "vs the oracle")
                checked += 1
    return checked


@pytest.mark.parametrize("batch", C.BATCHES, ids=lambda b: "b%d" % b)
@pytest.mark.parametrize("widths", list(GROUPS), ids=lambda w: "w" + "_".join(map(str, w)))
@pytest.mark.parametrize("kind", KINDS)
def test_mixed_group_forward_has_the_bits_of_single_table_calls(ce, oracle, kind, widths, batch):
    """fixed hotness 1 / 7 / 26 and ragged CSR bags (an all-empty table; empty bags on both sides of each table
    boundary), sum and mean, weighted and not, int32 / int64 indices and offsets."""
    assert run_all_layouts(ce, oracle, kind, widths, batch, lane=GROUPS[widths][kind]) == 4 * (3 * 2 + 2 * 4)


@pytest.mark.parametrize("batch", C.BATCHES, ids=lambda b: "b%d" % b)
def test_rows_wider_than_a_workgroup(ce, oracle, batch):
    """(514, 4) in fp32: 2,056-byte rows, 257 lanes of 8 bytes -- one more than a 256-thread workgroup has (the column
    loop's second pass) -- beside two-lane bags."""
    shape = ce.mixed_group_launch_shape(torch.float32, torch.int32, (514, 4), batch)
    assert shape["elems_per_lane"] == 2 and shape["block_threads"] == 256
    assert run_all_layouts(ce, oracle, "f32", (514, 4), batch, lane=8) == 4 * (3 * 2 + 2 * 4)


@pytest.mark.parametrize("kind", KINDS)
def test_same_width_group_equals_the_existing_grouped_forward(ce, oracle, kind):
    """(36, 36, 36): the [B, 3 * 36] result is the existing embedding_forward_grouped's [B, 3, 36]."""
    widths = (36, 36, 36)
    _, dev_tables = tables_of(oracle, kind, widths)
    mixed, same = ce.MixedTableGroup(dev_tables), ce.TableGroup(dev_tables)
    for batch in (5, 1023):
        for name, ids, offsets, hot, w32 in C.layouts(batch, ROWS[:3]):
            _, w_dev = to_kind(oracle, kind, w32)
            d_ids = torch.from_numpy(ids).cuda()
            d_off = None if offsets is None else torch.from_numpy(offsets).cuda()
            for mode, weighted in C.MODES:
                w = w_dev if weighted else None
                got = ce.embedding_forward_mixed_group(mixed, d_ids, d_off, w, num_hots=hot, mode=mode)
                old = ce.embedding_forward_grouped(same, d_ids, d_off, w, num_hots=hot, mode=mode)
                assert torch.equal(ibits(got), ibits(old).view(batch, 3 * 36)), (batch, name, mode, weighted)


def test_fixed_hotness_too_long_to_stage(ce, oracle):
    """(6, 2, 10) in fp16 has one-lane bags, 256 per workgroup: 26 int64 ids each exceed the 16 KiB staging budget, so the
    indices are read where they lie (offsets == nullptr in the unstaged kernel)."""
    widths, batch, hot = (6, 2, 10), 1023, 26
    assert not ce.mixed_group_launch_shape(torch.float16, torch.int64, widths, batch, hot)["staged"]
    assert ce.mixed_group_launch_shape(torch.float16, torch.int32, widths, batch, 7)["staged"]
    host_tables, dev_tables = tables_of(oracle, "f16", widths)
    rng = np.random.default_rng(5)
    ids = C.draw_ids(rng, ROWS[:3], np.full((3, batch), hot))
    w_host, w_dev = to_kind(oracle, "f16", C.weights_for(rng, ids.size))
    d_ids = torch.from_numpy(ids).cuda()
    for mode, weighted in C.MODES:
        want = host_bits(oracle_cat(oracle, host_tables, batch, ids, None, hot, w_host if weighted else None, mode))
        got = ce.embedding_forward_mixed_group(dev_tables, d_ids, None, w_dev if weighted else None, num_hots=hot, mode=mode)
        assert torch.equal(ibits(got).cpu(), want), (mode, weighted)


def shifted(t, nbytes):
    """A contiguous copy of t whose data pointer is `nbytes` past a 16-byte boundary (kept alive by the view)."""
    size = t.element_size()
    flat = torch.zeros((t.numel() + 32 // size,), dtype=t.dtype, device="cuda")
    first = ((nbytes - flat.data_ptr()) % 16) // size
    view = flat[first:first + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == nbytes and view.is_contiguous()
    return view


@pytest.mark.parametrize("batch", [5, 1023], ids=lambda b: "b%d" % b)
@pytest.mark.parametrize("kind", KINDS)
def test_misaligned_table_or_out_narrows_the_lanes_and_keeps_the_bits(ce, oracle, kind, batch):
    """One table viewed 8 bytes (then 4 bytes) past a 16-byte boundary, and `out` given so: the call narrows the lanes for
    the whole launch and the bits stay those of the aligned call."""
    widths = (128, 16, 64, 32)
    _, dev_tables = tables_of(oracle, kind, widths)
    D = sum(widths)
    aligned = ce.MixedTableGroup(dev_tables)
    by8 = ce.MixedTableGroup([dev_tables[0], shifted(dev_tables[1], 8), dev_tables[2], dev_tables[3]])
    by4 = ce.MixedTableGroup([dev_tables[0], dev_tables[1], shifted(dev_tables[2], 4), dev_tables[3]])
    assert (aligned.lane_bytes(), by8.lane_bytes(), by4.lane_bytes()) == (16, 8, 4)
    for name, ids, offsets, hot, w32 in C.layouts(batch, ROWS):
        _, w_dev = to_kind(oracle, kind, w32)
        d_ids = torch.from_numpy(ids.astype(np.int32)).cuda()
        d_off = None if offsets is None else torch.from_numpy(offsets.astype(np.int32)).cuda()
        for mode, weighted in C.MODES:
            w = w_dev if weighted else None
            want = ce.embedding_forward_mixed_group(aligned, d_ids, d_off, w, num_hots=hot, mode=mode)
            for group, lane in ((by8, 8), (by4, 4)):
                got = ce.embedding_forward_mixed_group(group, d_ids, d_off, w, num_hots=hot, mode=mode)
                assert group.lane_bytes(got.data_ptr()) == lane
                assert torch.equal(ibits(got), ibits(want)), (name, mode, weighted, lane, "table")
            for nbytes in (8, 4):
                out = shifted(torch.empty((batch, D), dtype=want.dtype, device="cuda"), nbytes)
                assert aligned.lane_bytes(out.data_ptr()) == nbytes
                back = ce.embedding_forward_mixed_group(aligned, d_ids, d_off, w, num_hots=hot, mode=mode, out=out)
                assert back.data_ptr() == out.data_ptr()
                assert torch.equal(ibits(out), ibits(want)), (name, mode, weighted, nbytes, "out")


@pytest.mark.parametrize("batch", [5, 1023], ids=lambda b: "b%d" % b)
@pytest.mark.parametrize("widths", [(128, 16, 64, 32), (36, 4, 128)], ids=lambda w: "w" + "_".join(map(str, w)))
@pytest.mark.parametrize("kind", KINDS)
def test_streaming_changes_no_bit_and_nothing_outside_out_is_written(ce, oracle, kind, widths, batch):
    """row_loads="streaming", and an out= region inside a larger buffer filled with a sentinel byte: nothing outside
    [B, D] changes."""
    _, dev_tables = tables_of(oracle, kind, widths)
    group = ce.MixedTableGroup(dev_tables)
    T, D, guard = len(widths), sum(widths), 4
    for name, ids, offsets, hot, w32 in C.layouts(batch, ROWS[:T]):
        _, w_dev = to_kind(oracle, kind, w32)
        d_ids = torch.from_numpy(ids.astype(np.int32)).cuda()
        d_off = None if offsets is None else torch.from_numpy(offsets).cuda()
        for mode, weighted in C.MODES:
            w = w_dev if weighted else None
            plain = ce.embedding_forward_mixed_group(group, d_ids, d_off, w, num_hots=hot, mode=mode)
            got = ce.embedding_forward_mixed_group(group, d_ids, d_off, w, num_hots=hot, mode=mode, row_loads="streaming")
            assert torch.equal(ibits(got), ibits(plain)), (name, mode, weighted, "streaming")
            buf = torch.empty((guard + batch + guard, D), dtype=plain.dtype, device="cuda")
            raw = buf.view(torch.uint8)
            raw.fill_(SENTINEL)
            region = buf[guard:guard + batch]
            back = ce.embedding_forward_mixed_group(group, d_ids, d_off, w, num_hots=hot, mode=mode, out=region)
            assert back.data_ptr() == region.data_ptr()
            assert torch.equal(ibits(region), ibits(plain)), (name, mode, weighted, "out=")
            assert bool((raw[:guard] == SENTINEL).all()) and bool((raw[guard + batch:] == SENTINEL).all()), \
                (name, mode, weighted, "a store left the [B, D] region")


def test_one_call_under_hip_graph_capture(ce):
    """One linear stream; the indices are rewritten in place between replays; the replayed result equals the eager one."""
    widths, batch = (128, 16, 64, 32), 64
    T = len(widths)
    tables = [torch.from_numpy(C.table_values(t, ROWS[t], w).astype(np.float16)).cuda() for t, w in enumerate(widths)]
    group = ce.MixedTableGroup(tables)
    lengths = np.full((T, batch), 9)
    offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(lengths.reshape(-1))])).cuda()
    idx = torch.from_numpy(C.draw_ids(np.random.default_rng(3), ROWS, lengths)).cuda()
    out = torch.empty((batch, sum(widths)), dtype=torch.float16, device="cuda")

    def step():
        ce.embedding_forward_mixed_group(group, idx, offsets, mode="sum", out=out)

    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        step()                               # warm-up outside capture (module loading, the descriptor's one copy)
        torch.cuda.current_stream().synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            step()
    for seed in (4, 5):
        idx.copy_(torch.from_numpy(C.draw_ids(np.random.default_rng(seed), ROWS, lengths)).cuda())
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        eager = ce.embedding_forward_mixed_group(group, idx, offsets, mode="sum")
        assert torch.equal(out, eager), seed


def test_bounds_check_repairs_or_raises(ce):
    widths, batch, hot = (36, 4, 128), 5, 7
    tables = [torch.from_numpy(C.table_values(t, ROWS[t], w)).cuda() for t, w in enumerate(widths)]
    rng = np.random.default_rng(9)
    ids = C.draw_ids(rng, ROWS[:3], np.full((3, batch), hot)).reshape(3, batch, hot)
    bad = ids.copy()
    bad[1, 2, 3] = ROWS[1]          # at table 1's row count (valid for table 0)
    bad[2, 0, 0] = -1
    repaired = bad.copy()
    repaired[1, 2, 3] = 0
    repaired[2, 0, 0] = 0
    d_bad, d_repaired = torch.from_numpy(bad).cuda(), torch.from_numpy(repaired).cuda()
    trusted = ce.MixedEmbeddingBagGroup(tables, mode="mean")
    assert trusted.num_tables == 3 and trusted.embedding_dim == sum(widths)
    want = trusted(d_repaired)
    assert torch.equal(want, ce.embedding_forward_mixed_group(trusted.group, d_repaired, num_hots=hot, mode="mean"))
    repairing = ce.MixedEmbeddingBagGroup(tables, mode="mean", bounds_check="repair")
    assert torch.equal(repairing(d_bad), want)
    assert repairing.last_check.words()[:2] == (2, 1 * batch * hot + 2 * hot + 3)
    with pytest.raises(IndexError):
        ce.MixedEmbeddingBagGroup(tables, mode="mean", bounds_check="raise")(d_bad)
    # CSR through the same door: offsets of the fixed-hotness batch
    off = torch.arange(0, 3 * batch * hot + 1, hot, device="cuda")
    assert torch.equal(repairing(d_bad.view(-1), off), want)
