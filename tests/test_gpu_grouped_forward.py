"""GPU parity of the grouped forward (one launch for a group of tables): bit-exact against the CPU oracle, called once
per table, and torch.equal to T single-table calls of embedding_forward stacked on dim 1.

What is new in the grouped kernel is the table choice, the output row and the table boundaries inside a wavefront and a
workgroup; the shapes (tests/grouped_cases.py) are the smallest at which those can go wrong: three tables of 5,000, 17
and 300 rows, B in {1, 5, 1,023}, every index source and access width (W = 4, 36, 128, 512; 514 in fp32)."""
import numpy as np
import pytest
import torch

import grouped_cases as C

pytestmark = pytest.mark.gpu

KINDS = ("f32", "f16", "bf16")
WIDTHS = (4, 36, 128, 512)
INT = {"i32": (np.int32, torch.int32), "i64": (np.int64, torch.int64)}
SENTINEL = 0x5A


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


def tables_of(oracle, kind, width, rows=C.ROWS):
    """(oracle arrays, device tensors) of the group, made once per (kind, width, rows) and never changed."""
    key = (kind, width, rows)
    if key not in _TABLES:
        _TABLES[key] = tuple(zip(*[to_kind(oracle, kind, C.table_values(t, r, width)) for t, r in enumerate(rows)]))
    return _TABLES[key]


def oracle_grouped(oracle, host_tables, batch, ids, offsets, hot, weights, mode):
    """[B, T, W]: oracle.embedding_forward once per table, stacked on dim 1 (numpy in, numpy out)."""
    per_table = []
    for t, table in enumerate(host_tables):
        i, o, w = C.table_slice(t, batch, ids, offsets, hot, ids if weights is None else weights)
        per_table.append(oracle.embedding_forward(table, i.astype(np.int32), None if o is None else o.astype(np.int32),
                                                  None if weights is None else w, batch_size=batch, num_hots=hot,
                                                  mode=mode))
    return np.stack(per_table, axis=1)


def single_table_stack(ce, dev_tables, batch, ids, offsets, hot, d_weights, mode):
    """[B, T, W]: torch.stack of T calls of ce.embedding_forward (numpy ids / offsets, device tables and weights)."""
    per_table = []
    for t, table in enumerate(dev_tables):
        i, o, _ = C.table_slice(t, batch, ids, offsets, hot, ids)
        lo = t * batch * hot if offsets is None else int(offsets[t * batch])
        w = None if d_weights is None else d_weights[lo:lo + i.size].contiguous()
        per_table.append(ce.embedding_forward(table, torch.from_numpy(np.ascontiguousarray(i)).cuda(),
                                              None if o is None else torch.from_numpy(np.ascontiguousarray(o)).cuda(), w,
                                              batch_size=batch, num_hots=hot, mode=mode))
    return torch.stack(per_table, dim=1)


def run_all_layouts(ce, oracle, kind, width, batch, rows=C.ROWS):
    host_tables, dev_tables = tables_of(oracle, kind, width, rows)
    group = ce.TableGroup(dev_tables)
    checked = 0
    for name, ids, offsets, hot, w32 in C.layouts(batch, rows):
        w_host, w_dev = to_kind(oracle, kind, w32)
        types = [(i, o) for i in INT for o in INT] if offsets is not None else [(i, "i32") for i in INT]
        for mode, weighted in C.MODES:
            want = host_bits(oracle_grouped(oracle, host_tables, batch, ids, offsets, hot,
                                            w_host if weighted else None, mode))
            assert tuple(want.shape) == (batch, len(rows), width)
            stacked = single_table_stack(ce, dev_tables, batch, ids, offsets, hot, w_dev if weighted else None, mode)
            for it, ot in types:
                d_ids = torch.from_numpy(ids.astype(INT[it][0])).cuda()
                d_off = None if offsets is None else torch.from_numpy(offsets.astype(INT[ot][0])).cuda()
                got = ce.embedding_forward_grouped(group, d_ids, d_off, w_dev if weighted else None, batch_size=batch,
                                                   num_hots=hot, mode=mode)
                assert got.shape == (batch, len(rows), width) and got.is_contiguous()
                assert torch.equal(ibits(got).cpu(), want), (name, mode, weighted, it, ot)
                assert torch.equal(ibits(got), ibits(stacked)), (name, mode, weighted, it, ot, "vs single-table calls")
                checked += 1
    return checked


@pytest.mark.parametrize("batch", C.BATCHES, ids=lambda b: "b%d" % b)
@pytest.mark.parametrize("width", WIDTHS, ids=lambda w: "w%d" % w)
@pytest.mark.parametrize("kind", KINDS)
def test_grouped_forward_matches_the_oracle_bit_for_bit(ce, oracle, kind, width, batch):
    """fixed hotness 1 / 7 / 26 and ragged CSR bags (an all-empty table; empty bags on both sides of each table
    boundary), sum and mean, weighted and not, int32 / int64 indices and offsets."""
    assert run_all_layouts(ce, oracle, kind, width, batch) == 4 * (3 * 2 + 2 * 4)


@pytest.mark.parametrize("batch", C.BATCHES, ids=lambda b: "b%d" % b)
def test_grouped_forward_of_rows_that_take_8_byte_lanes(ce, oracle, batch):
    """W = 514 in fp32: 2,056-byte rows, 257 lanes of 8 bytes (indices read from global memory)."""
    assert ce.grouped_forward_launch_shape(torch.float32, torch.int32, 514, 3, batch, 0, is_csr=True)["elems_per_lane"] == 2
    run_all_layouts(ce, oracle, "f32", 514, batch)


@pytest.mark.parametrize("kind,width", [("f32", 128), ("f16", 128), ("bf16", 36)], ids=["f32_w128", "f16_w128", "bf16_w36"])
def test_fixed_hotness_too_long_to_stage(ce, oracle, kind, width):
    """One sample's indices exceed the staging budget (4,100 int32 ids > 16 KiB): B = 5, the indices come through the
    cross-lane / global path with offsets == nullptr."""
    batch, hot = 5, 4100
    shape = ce.grouped_forward_launch_shape({"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}[kind],
                                            torch.int32, width, 3, batch, hot)
    assert not shape["staged"] and shape["index_source"] == ("global" if width == 36 else "wave_shuffle")
    host_tables, dev_tables = tables_of(oracle, kind, width)
    rng = np.random.default_rng(5)
    ids = C.draw_ids(rng, C.ROWS, np.full((3, batch), hot))
    w_host, w_dev = to_kind(oracle, kind, C.weights_for(rng, ids.size))
    d_ids = torch.from_numpy(ids.astype(np.int32)).cuda()
    for mode, weighted in C.MODES:
        want = host_bits(oracle_grouped(oracle, host_tables, batch, ids, None, hot, w_host if weighted else None, mode))
        got = ce.embedding_forward_grouped(dev_tables, d_ids, None, w_dev if weighted else None, num_hots=hot, mode=mode)
        assert torch.equal(ibits(got).cpu(), want), (mode, weighted)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("width", [36, 128])
def test_one_table_equals_the_single_table_call(ce, oracle, kind, width):
    host_tables, dev_tables = tables_of(oracle, kind, width)
    for batch in (5, 1023):
        for name, ids, offsets, hot, w32 in C.layouts(batch, rows=(C.ROWS[2],)):
            _, w_dev = to_kind(oracle, kind, w32)
            d_ids = torch.from_numpy(ids).cuda()
            d_off = None if offsets is None else torch.from_numpy(offsets).cuda()
            for mode, weighted in C.MODES:
                w = w_dev if weighted else None
                got = ce.embedding_forward_grouped([dev_tables[2]], d_ids, d_off, w, num_hots=hot, mode=mode)
                one = ce.embedding_forward(dev_tables[2], d_ids, d_off, w, batch_size=batch, num_hots=hot, mode=mode)
                assert got.shape == (batch, 1, width)
                assert torch.equal(ibits(got).view(batch, width), ibits(one)), (batch, name, mode, weighted)


@pytest.mark.parametrize("batch", [5, 1023], ids=lambda b: "b%d" % b)
@pytest.mark.parametrize("width", [36, 128])
@pytest.mark.parametrize("kind", KINDS)
def test_hints_change_no_bit_and_guard_rows_stay_untouched(ce, oracle, kind, width, batch):
    """row_loads="streaming", a sample_order over the combined bags (bag_order_by_length), and an out= buffer with
    guard rows on both sides of the [B, T, W] region."""
    _, dev_tables = tables_of(oracle, kind, width)
    group = ce.TableGroup(dev_tables)
    T, guard = len(dev_tables), 4
    for name, ids, offsets, hot, w32 in C.layouts(batch):
        _, w_dev = to_kind(oracle, kind, w32)
        d_ids = torch.from_numpy(ids.astype(np.int32)).cuda()
        d_off = None if offsets is None else torch.from_numpy(offsets).cuda()
        for mode, weighted in C.MODES:
            w = w_dev if weighted else None
            plain = ce.embedding_forward_grouped(group, d_ids, d_off, w, num_hots=hot, mode=mode)
            stacked = single_table_stack(ce, dev_tables, batch, ids, offsets, hot, w, mode)
            assert torch.equal(ibits(plain), ibits(stacked)), (name, mode, weighted, "vs single-table calls")
            got = ce.embedding_forward_grouped(group, d_ids, d_off, w, num_hots=hot, mode=mode, row_loads="streaming")
            assert torch.equal(ibits(got), ibits(plain)), (name, mode, weighted, "streaming")
            if d_off is not None:
                order = ce.bag_order_by_length(d_off)
                assert order.numel() == T * batch
                got = ce.embedding_forward_grouped(group, d_ids, d_off, w, mode=mode, sample_order=order)
                assert torch.equal(ibits(got), ibits(plain)), (name, mode, weighted, "sample_order")
                got = ce.embedding_forward_grouped(group, d_ids, d_off, w, mode=mode, sample_order=order,
                                                   row_loads="streaming")
                assert torch.equal(ibits(got), ibits(plain)), (name, mode, weighted, "sample_order + streaming")
            buf = torch.empty((guard + batch * T + guard, width), dtype=plain.dtype, device="cuda")
            raw = buf.view(torch.uint8)
            raw.fill_(SENTINEL)
            region = buf[guard:guard + batch * T].view(batch, T, width)
            back = ce.embedding_forward_grouped(group, d_ids, d_off, w, num_hots=hot, mode=mode, out=region)
            assert back.data_ptr() == region.data_ptr()
            assert torch.equal(ibits(region), ibits(plain)), (name, mode, weighted, "out=")
            assert bool((raw[:guard] == SENTINEL).all()) and bool((raw[guard + batch * T:] == SENTINEL).all()), \
                (name, mode, weighted, "a store left the [B, T, W] region")


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
def test_one_misaligned_table_narrows_the_group_and_stays_bit_exact(ce, oracle, kind, batch):
    """One table viewed 8 bytes past a 16-byte boundary: 8-byte lanes for the whole group; another one 4 bytes past: 4-byte
    lanes.  Same bits as the aligned group."""
    width = 128
    host_tables, dev_tables = tables_of(oracle, kind, width)
    aligned = ce.TableGroup(dev_tables)
    by8 = ce.TableGroup([dev_tables[0], shifted(dev_tables[1], 8), dev_tables[2]])
    by4 = ce.TableGroup([dev_tables[0], shifted(dev_tables[1], 8), shifted(dev_tables[2], 4)])
    for name, ids, offsets, hot, w32 in C.layouts(batch):
        w_host, w_dev = to_kind(oracle, kind, w32)
        d_ids = torch.from_numpy(ids.astype(np.int32)).cuda()
        d_off = None if offsets is None else torch.from_numpy(offsets.astype(np.int32)).cuda()
        for mode, weighted in C.MODES:
            want = host_bits(oracle_grouped(oracle, host_tables, batch, ids, offsets, hot, w_host if weighted else None,
                                            mode))
            for group, lane in ((aligned, 16), (by8, 8), (by4, 4)):
                got = ce.embedding_forward_grouped(group, d_ids, d_off, w_dev if weighted else None, num_hots=hot, mode=mode)
                assert group.lane_bytes(got.data_ptr()) == lane
                assert torch.equal(ibits(got).cpu(), want), (name, mode, weighted, lane)
