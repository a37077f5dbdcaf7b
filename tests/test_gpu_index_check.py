"""cuembed_amd.check_indices on the GPU against the numpy model (tests/index_check_reference.py), exactly: the four
report words and both repaired arrays, for int32 / int64 indices x int32 / int64 offsets, report-only, in place and out
of place, on one table and on the three-table group of the grouped tests (5,000 / 17 / 300 rows).

Bad data only ever goes into check_indices, which dereferences nothing with it: no test here (or anywhere) hands an
unrepaired bad array to a kernel that addresses table rows.

Sizes: nnz in {0, 1, 63, 64, 65, 1,023, 4,097} crosses wavefront (64) and workgroup (256 lanes of 1, 2 or 4 ids)
boundaries of the index pass; B in {1, 5, 1,023}; B = 1,023 with three tables gives 3,070 offsets = three tiles of the
offsets scan, one chunk each; B = 700,001 gives 2,100,004 offsets = 684 tiles of three chunks each, the one size at which
a workgroup of the scan carries its state from chunk to chunk.  Every CSR call gets a report pre-filled with garbage and a workspace of exactly the queried size filled
with 0xFF.
"""
import numpy as np
import pytest
import torch

import index_check_reference as M
from grouped_cases import ROWS

pytestmark = pytest.mark.gpu

SHAPES = [(0, 1), (1, 1), (63, 5), (64, 5), (65, 1), (1023, 5), (4097, 1023)]       # (nnz, B)
GROUPS = {"single": (300,), "group": ROWS}
TORCH = {np.int32: torch.int32, np.int64: torch.int64}
GARBAGE = 0x7A7A7A7A7A7A7A7A


@pytest.fixture(scope="module")
def ce():
    import cuembed_amd
    assert torch.cuda.is_available()
    return cuembed_amd


@pytest.fixture(scope="module")
def table_groups(ce):
    """The groups whose row counts are checked against (the check never reads a table: width 4 is enough)."""
    return {name: ce.TableGroup([torch.zeros((r, 4), device="cuda") for r in rows]) for name, rows in GROUPS.items()}


def clean_csr(rng, rows, batch, nnz, boundary_empties=False):
    """(ids int64 [nnz], offsets int64 [T * B + 1]) of a valid batch: random bag lengths that sum to nnz."""
    T = len(rows)
    n = T * batch
    inner = np.sort(rng.integers(0, nnz + 1, n - 1)) if n > 1 else np.zeros(0, dtype=np.int64)
    offsets = np.concatenate([[0], inner, [nnz]]).astype(np.int64)
    if boundary_empties and batch >= 3:
        for t in range(1, T):       # the last bag of table t - 1 and the first of table t are empty
            offsets[t * batch - 1] = offsets[t * batch]
            offsets[t * batch + 1] = offsets[t * batch]
        offsets = np.maximum.accumulate(offsets)
    table, _ = M.table_of_positions(nnz, rows, batch, 0, offsets)
    ids = (rng.integers(0, 1 << 40, nnz) % np.asarray(rows, dtype=np.int64)[table]) if nnz else np.zeros(0, dtype=np.int64)
    return ids.astype(np.int64), offsets


def csr_cases(rng, rows, batch, nnz, idx_np, off_np):
    """[(name, ids, offsets)]: the clean batch and every corruption of the issue's list that this shape can hold."""
    T, n = len(rows), len(rows) * batch
    ii, oi = np.iinfo(idx_np), np.iinfo(off_np)
    ids, offsets = clean_csr(rng, rows, batch, nnz)
    table, _ = M.table_of_positions(nnz, rows, batch, 0, offsets)
    own_rows = np.asarray(rows, dtype=np.int64)[table] if nnz else np.zeros(0, dtype=np.int64)
    out = [("clean", ids, offsets)]
    if nnz:
        edges = sorted({p for p in (0, nnz - 1, 63, 64, 255, 256, 511, 512, 1023, 1024, 2047, 2048, 4095, 4096) if p < nnz})
        bad = ids.copy()
        for k, p in enumerate(edges):     # -1 and exactly rows_t, in turn, at the first, the last and every boundary position
            bad[p] = -1 if k % 2 else own_rows[p]
        out.append(("edges", bad, offsets))
        out.append(("all_bad", np.where(np.arange(nnz) % 2 == 0, own_rows, -1 - np.arange(nnz)), offsets))
        extreme = ids.copy()
        extreme[rng.integers(0, nnz, min(nnz, 4))] = ii.min
        extreme[rng.integers(0, nnz, min(nnz, 4))] = ii.max
        out.append(("extreme_ids", extreme, offsets))
    mid = n // 2
    if n >= 2:
        o = offsets.copy()
        o[mid] = offsets[mid - 1] - 1 if offsets[mid - 1] > 0 else -1
        out.append(("one_decrease", ids, o))
        o = offsets.copy()
        o[mid] = oi.max
        out.append(("spike", ids, o))
        o = offsets.copy()
        o[:mid] = -1 - np.arange(mid)
        o[0] = oi.min
        out.append(("negative_offsets", ids, o))
    o = offsets.copy()
    o[n] = nnz + 7
    out.append(("end_past_nnz", ids, o))
    if nnz >= 2:        # o[0] > 0: the ids in front of it belong to no bag -- a bad one there is not counted
        o = np.maximum(offsets, 1)
        bad = ids.copy()
        bad[0] = -1
        out.append(("skipped_head", bad, o))
    out.append(("garbage_offsets", ids, rng.integers(oi.min, oi.max, n + 1, dtype=np.int64, endpoint=True)))
    if nnz:
        out.append(("garbage_both", rng.integers(ii.min, ii.max, nnz, dtype=np.int64, endpoint=True),
                    rng.integers(-nnz, 2 * nnz + 1, n + 1, dtype=np.int64)))
    return out


def neighbour_case(rng):
    """The three-table group at B = 5 with empty bags on both sides of each table boundary: ids that are valid for the
    larger neighbouring table but not for their own, at the first and last position of table 1 (17 rows) and of table 2."""
    rows, batch, nnz = ROWS, 5, 1023
    ids, offsets = clean_csr(rng, rows, batch, nnz, boundary_empties=True)
    cuts = offsets[::batch]
    assert cuts[1] + 2 <= cuts[2] < cuts[3] and offsets[batch - 1] == offsets[batch] == offsets[batch + 1]
    ids[cuts[1]] = 17          # first of table 1: a row of table 0 (5,000 rows) and of table 2 (300), not of table 1
    ids[cuts[2] - 1] = 299     # last of table 1: the last row of table 2
    ids[cuts[1] - 1] = 4999    # last of table 0: valid there
    ids[cuts[2]] = 300         # first of table 2: one past its rows, valid for table 0 only
    return ids, offsets


def run(ce, name, ids, offsets, rows, batch, hot, idx_np, off_np, mode, source, misaligned=False):
    idx_np_arr = ids.astype(idx_np)
    off_np_arr = None if offsets is None else offsets.astype(off_np)
    want_report, want_ids, want_offsets = M.check(idx_np_arr, off_np_arr, rows, batch, hot)

    def device(a):
        if not misaligned:
            return torch.from_numpy(a).cuda()
        # `misaligned` elements past a 16-byte boundary: 4 bytes (int32 [1:]) and 8 bytes (int64 [1:]) leave one id per
        # lane, 8 bytes of int32 ([2:]) two
        buf = torch.empty((a.size + misaligned,), dtype=TORCH[a.dtype.type], device="cuda")
        view = buf[misaligned:].view(a.shape)
        view.copy_(torch.from_numpy(a))
        assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == misaligned * a.itemsize != 0
        return view

    idx = device(idx_np_arr)
    off = None if off_np_arr is None else torch.from_numpy(off_np_arr).cuda()
    report = torch.full((4,), GARBAGE, dtype=torch.int64, device="cuda")
    need = ce.check_indices_workspace_bytes(len(rows), batch, hot, ids.size)
    workspace = torch.full((need,), 0xFF, dtype=torch.uint8, device="cuda") if need else None
    kwargs = dict(batch_size=batch, num_hots=hot, report=report, workspace=workspace)
    kwargs.update(source)
    if mode == "in_place":
        kwargs.update(repair=True, out_indices=idx, out_offsets=off)
    elif mode == "out_of_place":
        kwargs.update(repair=True)
    got = ce.check_indices(idx, off, **kwargs)
    what = (name, mode, idx_np.__name__, off_np.__name__)
    assert got.report is report
    assert np.array_equal(report.cpu().numpy(), want_report), (what, report.tolist(), want_report.tolist())
    if mode == "report":
        assert got.indices is idx and got.offsets is off
    else:
        assert np.array_equal(got.indices.cpu().numpy(), want_ids), what
        if off is not None:
            assert np.array_equal(got.offsets.cpu().numpy(), want_offsets), what
        if want_report[0] == 0 and want_report[2] == 0:       # a clean batch: bit-identical copies
            assert np.array_equal(want_ids, idx_np_arr) and (off is None or np.array_equal(want_offsets, off_np_arr))
    if mode != "in_place":                                    # the inputs are never written
        assert np.array_equal(idx.cpu().numpy(), idx_np_arr), what
        assert off is None or np.array_equal(off.cpu().numpy(), off_np_arr), what
    return got


MODES = ("report", "in_place", "out_of_place")
TYPES = [(np.int32, np.int32), (np.int32, np.int64), (np.int64, np.int32), (np.int64, np.int64)]
TYPE_IDS = ["i32_o32", "i32_o64", "i64_o32", "i64_o64"]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("idx_np,off_np", TYPES, ids=TYPE_IDS)
def test_csr_report_and_repair_match_the_model(ce, table_groups, idx_np, off_np, mode):
    rng = np.random.default_rng(11)
    for gname, rows in GROUPS.items():
        source = dict(num_rows=rows[0]) if gname == "single" else dict(group=table_groups[gname])
        for nnz, batch in SHAPES:
            for name, ids, offsets in csr_cases(rng, rows, batch, nnz, idx_np, off_np):
                run(ce, "%s/%s/nnz%d/B%d" % (gname, name, nnz, batch), ids, offsets, rows, batch, 0, idx_np, off_np, mode,
                    source)
    ids, offsets = neighbour_case(rng)
    got = run(ce, "neighbours", ids, offsets, ROWS, 5, 0, idx_np, off_np, mode, dict(group=table_groups["group"]))
    assert got.words()[0] == 3       # (4999 in table 0 is the one valid id of the four)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("idx_np", [np.int32, np.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("hot", [1, 3, 64])
def test_fixed_hotness_matches_the_model(ce, table_groups, idx_np, hot, mode):
    rng = np.random.default_rng(13 + hot)
    ii = np.iinfo(idx_np)
    for gname, rows in GROUPS.items():
        source = dict(num_rows=rows[0]) if gname == "single" else dict(group=table_groups[gname])
        for batch in (1, 5, 1023):
            per_table = batch * hot
            nnz = len(rows) * per_table
            table = np.arange(nnz) // per_table
            own_rows = np.asarray(rows, dtype=np.int64)[table]
            clean = rng.integers(0, 1 << 40, nnz) % own_rows
            some = clean.copy()
            for k, p in enumerate(sorted({0, nnz - 1, per_table - 1, per_table % nnz, (2 * per_table - 1) % nnz})):
                some[p] = -1 if k % 2 else own_rows[p]          # the first, the last and both sides of a table boundary
            some[rng.integers(0, nnz, max(1, nnz // 100))] = ii.min
            some[rng.integers(0, nnz, max(1, nnz // 100))] = ii.max
            for name, ids in (("clean", clean), ("some", some), ("all_bad", own_rows + np.arange(nnz) % 3)):
                shaped = ids.reshape(len(rows), batch, hot)
                run(ce, "%s/%s/B%d/H%d" % (gname, name, batch, hot), shaped, None, rows, batch, hot, idx_np, np.int64, mode,
                    source)


@pytest.mark.parametrize("mode", MODES)
def test_rows_past_2_to_the_31_are_compared_in_64_bits(ce, mode):
    rows = 1 << 40          # (no table exists: the check reads none)
    ids = np.array([0, rows - 1, rows, rows + 5, -1, np.iinfo(np.int64).max, 1 << 31, (1 << 32) + 1], dtype=np.int64)
    offsets = np.array([0, 3, 3, 8], dtype=np.int64)
    got = run(ce, "2^40 rows", ids, offsets, (rows,), 3, 0, np.int64, np.int64, mode, dict(num_rows=rows))
    assert got.words() == (4, 2, 0, -1)
    run(ce, "2^40 rows, fixed", ids, None, (rows,), 4, 2, np.int64, np.int64, mode, dict(num_rows=rows))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("idx_np,shift", [(np.int32, 1), (np.int32, 2), (np.int64, 1)], ids=["i32_4B", "i32_8B", "i64_8B"])
def test_a_misaligned_view_of_the_indices(ce, table_groups, idx_np, shift, mode):
    """indices[1:] and indices[2:] of a 16-byte aligned buffer: the narrower pieces (one id per lane; two for int32 ids
    that are 8-byte aligned), CSR and fixed hotness, in place and (with an aligned output: the less aligned of the two
    decides) out of place."""
    rng = np.random.default_rng(17)
    source = dict(group=table_groups["group"])
    for nnz, batch in ((65, 1), (1023, 5), (4097, 1023)):
        for name, ids, offsets in csr_cases(rng, ROWS, batch, nnz, idx_np, np.int32)[:4]:
            run(ce, "misaligned/%s/nnz%d" % (name, nnz), ids, offsets, ROWS, batch, 0, idx_np, np.int32, mode, source,
                misaligned=shift)
    rows = np.asarray(ROWS, dtype=np.int64)
    for batch, hot in ((1, 1), (5, 3), (1023, 3)):
        per_table = batch * hot
        nnz = len(ROWS) * per_table
        own_rows = rows[np.arange(nnz) // per_table]
        clean = rng.integers(0, 1 << 40, nnz) % own_rows
        some = clean.copy()
        for k, p in enumerate(sorted({0, nnz - 1, per_table - 1, per_table, 2 * per_table - 1, 2 * per_table})):
            some[p % nnz] = -1 if k % 2 else own_rows[p % nnz]      # the first, the last, both sides of both table boundaries
        for name, ids in (("clean", clean), ("some", some), ("all_bad", own_rows + np.arange(nnz) % 3)):
            run(ce, "misaligned/fixed/%s/B%d/H%d" % (name, batch, hot), ids.reshape(len(ROWS), batch, hot), None, ROWS,
                batch, hot, idx_np, np.int64, mode, source, misaligned=shift)


def long_offsets_case(rng, off_np, clean):
    """The three-table group with B = 700,001: 2,100,004 offsets are 684 tiles of THREE 1,024-offset chunks each, so a
    workgroup of the offsets scan carries its running maximum and its last raw offset from chunk to chunk.  The table cuts
    (offsets 700,001 and 1,400,002) lie in a tile's third chunk.  Unless `clean`: on both sides of inner chunk
    boundaries (positions 1,023 / 1,024 and 2,047 / 2,048 of a tile) and of tile boundaries (3,071 / 3,072), in three
    tiles, a decrease, a negative value and a spike that the running maximum must carry across the boundary -- one of
    them in front of each cut, so that the cuts themselves depend on the carry -- and, late, one spike far above nnz;
    and bad ids everywhere, whose verdicts depend on the cuts."""
    rows, batch, nnz = ROWS, 700001, 3000000
    n = len(rows) * batch
    tile = 3 * 1024
    offsets = np.sort(rng.integers(0, nnz + 1, n + 1)).astype(np.int64)
    offsets[0], offsets[n] = 0, nnz
    table, _ = M.table_of_positions(nnz, rows, batch, 0, offsets)
    own_rows = np.asarray(rows, dtype=np.int64)[table]
    ids = rng.integers(0, 1 << 40, nnz) % own_rows
    if clean:
        return ids, offsets, rows, batch
    kinds = ("decrease", "negative", "carry")
    k = 0
    for t in (5, 300, 683):
        for rel in (1024, 2048, 3072):
            for p in (t * tile + rel - 1, t * tile + rel):
                if p > n:
                    continue
                kind = kinds[k % 3]
                k += 1
                if kind == "decrease":
                    offsets[p] = offsets[p - 1] - 1
                elif kind == "negative":
                    offsets[p] = -5 - k
                else:
                    offsets[p] += 4000          # above the next 2,800 offsets or so: the next chunk starts below the carry
    for cut in (batch, 2 * batch):              # in the chunk in front of the cut's own
        offsets[cut - 700] += 4000
    offsets[600 * tile + 1023] = np.iinfo(off_np).max
    bad = rng.integers(0, nnz, nnz // 100)
    ids[bad] = np.where(bad % 2 == 0, own_rows[bad], -1 - bad)
    return ids, offsets, rows, batch


@pytest.mark.parametrize("mode", ("in_place", "out_of_place"))
@pytest.mark.parametrize("off_np", [np.int32, np.int64], ids=["o32", "o64"])
def test_offsets_scan_carries_across_the_chunks_of_a_tile(ce, table_groups, off_np, mode):
    rng = np.random.default_rng(29)
    source = dict(group=table_groups["group"])
    for clean in (True, False):
        ids, offsets, rows, batch = long_offsets_case(rng, off_np, clean)
        got = run(ce, "long offsets, clean=%s" % clean, ids, offsets, rows, batch, 0, np.int32, off_np, mode, source)
        words = got.words()
        if clean:
            assert words == (0, -1, 0, -1)
        else:
            # the carries mattered: the cuts are not the raw offsets, and bad ids were found in every table
            repaired = M.repair_offsets(offsets, ids.size)
            assert repaired[batch] != offsets[batch] and repaired[2 * batch] != offsets[2 * batch]
            assert words[2] >= 12 and words[3] == 5 * 3072 + 1023 and words[0] > 20000


def test_the_same_call_twice_on_one_report_agrees(ce, table_groups):
    rng = np.random.default_rng(19)
    _, ids, offsets = csr_cases(rng, ROWS, 1023, 4097, np.int64, np.int64)[-1]       # garbage in both arrays
    idx, off = torch.from_numpy(ids).cuda(), torch.from_numpy(offsets).cuda()
    report = ce.new_index_report("cuda")
    first = ce.check_indices(idx, off, group=table_groups["group"], repair=True, report=report)
    words = first.words()
    second = ce.check_indices(idx, off, group=table_groups["group"], repair=True, report=report)
    assert second.words() == words and words[0] > 0 and words[2] > 0
    assert torch.equal(first.indices, second.indices) and torch.equal(first.offsets, second.offsets)
    # ... and the repaired batch is clean, and repairing it changes nothing
    again = ce.check_indices(first.indices, first.offsets, group=table_groups["group"], repair=True, report=report)
    assert again.words() == (0, -1, 0, -1)
    assert torch.equal(again.indices, first.indices) and torch.equal(again.offsets, first.offsets)
    assert again.raise_if_bad() is again


def test_raise_if_bad_names_counts_positions_table_and_values(ce, table_groups):
    rng = np.random.default_rng(23)
    ids, offsets = neighbour_case(rng)
    cuts = offsets[::5]
    idx, off = torch.from_numpy(ids).cuda(), torch.from_numpy(offsets).cuda()
    with pytest.raises(IndexError) as err:
        ce.check_indices(idx, off, group=table_groups["group"]).raise_if_bad()
    text = str(err.value)
    assert "3 bad indices" in text and "first at position %d (table 1 of 17 rows)" % cuts[1] in text
    assert "indices[%d] = 17" % cuts[1] in text and "bad offsets" not in text
    bad_off = off.clone()
    bad_off[7] = -3
    with pytest.raises(IndexError) as err:
        ce.check_indices(idx, bad_off, group=table_groups["group"], repair=True).raise_if_bad()
    text = str(err.value)
    assert "1 bad offsets, first at position 7 (table 1): offsets[7] = -3 after" in text
    in_place = ce.check_indices(idx, bad_off, group=table_groups["group"], repair=True, out_indices=idx,
                                out_offsets=bad_off)
    with pytest.raises(IndexError) as err:
        in_place.raise_if_bad()
    assert "offsets[7]" not in str(err.value) and "indices[" not in str(err.value) and "table 1" in str(err.value)
