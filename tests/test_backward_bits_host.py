"""The conditions under which the backward's fingerprints (test_gpu_backward_bits.py) do not depend on the order in
which workgroups arrive, asserted on the CPU for every case: the run structure comes from the generators of
backward_bits_cases.py, the launch shape from backward_launch_shape(..., compute_units=256, xcds=8) under the case's
forced tuning (host arithmetic, no device).

Rows that several workgroups contribute to receive hardware float atomics.  Two contributions onto zero commute; three,
or two onto a value that an earlier sample block stored, round differently by arrival order.  So
  * a case on arbitrary data has no run longer than one workgroup's lookups (it touches two workgroups at most), and
  * in sample blocks after the first, none of its runs of a row that an earlier block stored crosses a workgroup
    boundary;
  * everything else is exact data: every sum of consecutive lookups of a run is representable in the case's type, so
    no order of additions can round.
No case is exempt.  The case list must also hold every shape the suite is there for."""
import functools

import numpy as np
import pytest
import torch

import backward_bits_cases as C
import test_gpu_backward_bits as P

#: |x| up to which every multiple of 0.25 (weighted) or 1 (unweighted) is representable: 11 / 8 / 24 significant bits
EXACT_BELOW = {"f16": {True: 512, False: 2048}, "bf16": {True: 64, False: 256}, "f32": {True: 1 << 22, False: 1 << 24}}


@pytest.fixture(scope="module")
def ce():
    import cuembed_amd
    return cuembed_amd


@functools.lru_cache(maxsize=None)
def structure(case_name):
    """(the case's inputs, its launch shape, and per run: block, lookups, workgroups touched, segments touched inside
    one workgroup, shared with an earlier block, ends at a segment end, ends at a workgroup end)."""
    import cuembed_amd as ce
    case = C.CASES[case_name]
    shape = P.pinned_shape(ce, case, compute_units=256, xcds=8)
    seg, per_block = shape["segment_len"], shape["segments_per_block"]
    d = C.build(case, seg, per_block)
    block = seg * per_block
    rows = []
    for p, start, lens, key, shared in d["runs"]:
        last = start + lens - 1
        groups = last // block - start // block + 1
        segments = np.where(groups == 1, last // seg - start // seg + 1, 0)
        rows.append(np.stack([np.full_like(lens, p), lens, groups, segments, shared.astype(np.int64),
                              ((last + 1) % seg == 0).astype(np.int64), ((last + 1) % block == 0).astype(np.int64)], axis=1))
    return d, shape, np.concatenate(rows)


@pytest.mark.parametrize("case_name", sorted(C.CASES))
def test_the_case_cannot_depend_on_arrival_order(ce, case_name):
    case = C.CASES[case_name]
    d, shape, runs = structure(case_name)
    block = shape["segment_len"] * shape["segments_per_block"]
    assert shape["column_slices"] == case.slices and shape["segment_len"] % 8 == 0
    assert d["keys"].shape[0] == d["nnz"] == int(runs[:, 1].sum())
    for p, start, lens, key, _ in d["runs"]:                                   # every block is sorted, its runs distinct rows
        assert np.all(np.diff(key) > 0)
    assert d["sids"].min() >= 0 and d["sids"].max() < C.BATCH
    if case.data == "arb":
        assert runs[:, 1].max() <= block, "a run longer than one workgroup's lookups"
        assert runs[:, 2].max() <= 2
        later_shared = runs[(runs[:, 0] > 0) & (runs[:, 4] == 1)]
        assert later_shared.shape[0] > 0 or case.blocks == 1
        assert np.all(later_shared[:, 2] == 1), "a run of a stored row crosses a workgroup boundary in a later block"
    else:
        # every sum of consecutive lookups of a run is the difference of two prefix sums of the COO
        values = d["grad_y"][d["sids"]].astype(np.float64)
        if case.weighted:
            values *= d["weights"].astype(np.float64)[:, None]
        assert np.all(values * 4 == np.round(values * 4))
        prefix = np.cumsum(values, axis=0)
        first = np.concatenate([np.repeat(start + p * d["block_len"], lens) for p, start, lens, _, _ in d["runs"]])
        prefix -= np.where(first[:, None] > 0, prefix[np.maximum(first - 1, 0)], 0.0)
        assert 2 * np.abs(prefix).max() < EXACT_BELOW[case.kind][case.weighted]
        # ... and so is what a row holds after each of its blocks (one row may have a run in every block)
        assert 2 * case.blocks * np.abs(prefix).max() < EXACT_BELOW[case.kind][case.weighted]


def test_the_cases_hold_every_shape_the_suite_is_for(ce):
    assert len(C.CASES) <= 150
    cases = list(C.CASES.values())
    shapes = {name: structure(name)[1] for name in C.CASES}
    for kind in ("f32", "f16", "bf16"):
        mine = [c for c in cases if c.kind == kind]
        assert {c.index for c in mine} == {"i32", "i64"} and {c.weighted for c in mine} == {True, False}
        assert {c.data for c in mine} == {"arb", "exact"} and {c.blocks for c in mine} == {1, 2, 3}
        lanes = {(C.lanes_of(kind, c.width), c.width * C.ELEM_BYTES[kind] // C.lanes_of(kind, c.width)) for c in mine}
        assert lanes >= {(1, 4), (3, 4), (3, 8), (8, 16), (32, 16), (257, 16)}, lanes
        assert any(shapes[C.case_id(c)]["segments_per_block"] == 1 for c in mine)
    assert {s["segment_len"] for s in shapes.values()} >= {8, 24, 32, 128}
    assert {c.slices for c in cases} == {1, 2, 4, 8}
    assert {c.out for c in cases} == {"dense", "known", "fit", "over", "small", "pad", "skip"}
    assert {c.nnz for c in cases} >= {1, 3, 7}
    for data in ("arb", "exact"):
        seen = np.zeros(8, dtype=bool)
        for name, c in C.CASES.items():
            if c.data != data or c.nnz is not None:
                continue
            _, shape, runs = structure(name)
            seg, block = shape["segment_len"], shape["segment_len"] * shape["segments_per_block"]
            lens = set(runs[:, 1].tolist())
            assert {1, 2, seg - 1, seg} <= lens and (seg + 1 in lens or seg + 1 > block)
            assert d_ragged(runs, seg, block)
            seen |= [bool(np.any(runs[:, 3] >= 3)), bool(np.any(runs[:, 3] >= 4)), bool(np.any(runs[:, 5] == 1)),
                     bool(np.any(runs[:, 6] == 1)), bool(np.any(runs[:, 2] == 2)), bool(np.any(runs[:, 2] >= 3)),
                     bool(np.any((runs[:, 0] > 0) & (runs[:, 4] == 1) & (runs[:, 2] >= 2))),
                     bool(np.any((runs[:, 0] > 0) & (runs[:, 4] == 1) & (runs[:, 3] >= 2)))]
        # through three, and four, segments of one workgroup; to a segment end; to a workgroup end; over one workgroup
        # boundary; through three workgroups; a stored row over a boundary in a later block; ... chained inside one
        want = [True, True, True, True, True, data == "exact", data == "exact", True]
        assert seen.tolist() == want, (data, seen.tolist())


def d_ragged(runs, seg, block):
    nnz = int(runs[runs[:, 0] == runs[:, 0].max(), 1].sum())
    return nnz % seg != 0 and nnz % block != 0
