"""The conditions that keep tests/test_gpu_far_rows.py honest, checked where no GPU is needed: for every view the GPU file
looks up, the picked rows straddle every 2^31 / 2^32 threshold that fits, every address a narrowing kernel would form
lies inside the arena, and poison, true rows and the tensors sharing the arena do not overlap (tests/far_rows.py)."""
import numpy as np
import pytest

import far_rows as F

INT32 = 1 << 31
FORWARD_IDS = ["%s-W%d+%d" % c[:3] for c in F.FORWARD_TABLES]


def _views():
    for kind, width, shift, _, int32_too in F.FORWARD_TABLES:
        yield "forward %s W=%d +%d" % (kind, width, shift), F.table_view(kind, width, shift), int32_too
    for kind, width, shift in F.WEIGHT_GRAD_TABLES[-2:]:                # (the others are forward tables)
        yield "weight gradient %s W=%d" % (kind, width), F.table_view(kind, width, shift), True
    for width, shift, _ in F.QUANTIZED_TABLES:
        yield "quantized W=%d +%d" % (width, shift), F.quantized_view(width, shift), True
    for kind, width in F.BACKWARD_TABLES:
        yield "backward %s W=%d" % (kind, width), F.backward_view(kind, width), True


VIEWS = list(_views())


def _straddled(view, rows, below=None):
    """Every threshold that fits (and, with `below`, whose rows are below it) has its two rows among `rows`, and they lie
    on either side of it."""
    unit = {"elements": view.width, "bytes": view.row_bytes, "rows": 1}
    count = 0
    for what, t, lo, hi in F.thresholds(view):
        assert lo * unit[what] < t <= hi * unit[what] and hi == lo + 1
        if below is None or hi < below:
            assert lo in rows and hi in rows, (view, what, t)
            count += 1
    return count


@pytest.mark.parametrize("name,view,int32_too", VIEWS, ids=[v[0] for v in VIEWS])
def test_picked_rows_straddle_every_threshold_and_aliases_stay_inside(name, view, int32_too):
    assert view.base >= F.GUARD and view.end <= F.ARENA_BYTES
    assert (view.rows - 1) * view.row_bytes >= F.GUARD or view.rows == F.BACKWARD_MAX_ROWS     # 16 GiB past the base
    layout, (rows,) = F.pick([view], seed=1)
    assert rows == sorted(set(rows)) and rows[-1] == view.rows - 1 and rows[0] in range(16) and rows[1] == rows[0] + 1
    # what fits: bytes to 2^34 always (the view is that long); elements to 2^32 unless the elements are single bytes ...
    fits = {(what, t) for what, t, _, _ in F.thresholds(view)}
    if view.rows != F.BACKWARD_MAX_ROWS:
        assert {("bytes", t) for t in F.BYTE_THRESHOLDS} <= fits
        assert {("elements", t) for t in F.ELEM_THRESHOLDS} <= fits
    assert (("rows", 1 << 31) in fits) == (view.rows > (1 << 31)) and (("rows", 1 << 32) in fits) == (view.rows > (1 << 32))
    if view.row_bytes == 4:
        assert ("rows", 1 << 32) in fits
    if view.row_bytes <= 8 and view.rows != F.BACKWARD_MAX_ROWS:
        assert ("rows", 1 << 31) in fits
    assert _straddled(view, rows) == len(fits)
    # the aliases: inside the arena, clear of every touched row, and there ARE some (the case can tell a narrowing)
    assert layout.aliases and all(0 <= a and a + n <= F.ARENA_BYTES for a, n in layout.aliases)
    touched = sorted(layout.touched)
    for a, n in layout.aliases:
        assert all(a + n <= b or b + m <= a for b, m in touched)
    assert len(touched) == len(rows) and all(b + m <= c for (b, m), (c, _) in zip(touched, touched[1:]))
    # signed wraps reach back at most 16 GiB (row ids of 4- and 8-byte rows), 8 GiB (element offsets), 2 GiB (bytes)
    for r in rows:
        for a in F.aliases(view, r):
            assert view.base - F.GUARD <= a < view.base + F.GUARD + view.row_bytes
    if int32_too:
        layout32, (rows32,) = F.pick([view], seed=1, below=INT32)
        assert rows32 and max(rows32) < INT32 and max(rows32) * view.width >= INT32          # still past 2^31 elements
        assert _straddled(view, rows32, below=INT32) >= 2
        assert layout32.aliases


def test_a_narrowed_row_is_another_address_for_every_far_row():
    """What makes a case bite: for every picked row past a threshold, the narrowed form of the quantity that passed it
    is a different address (so the kernel reads poison or another row), and below every threshold there is none."""
    for _, view, _ in VIEWS:
        _, (rows,) = F.pick([view], seed=1)
        for r in rows:
            far = r >= (1 << 31) or r * view.width >= (1 << 31) or r * view.row_bytes >= (1 << 31)
            assert bool(F.aliases(view, r)) == far, (view, r)
            unsigned = {view.base + (r & 0xFFFFFFFF) * view.row_bytes, view.base + ((r * view.width) & 0xFFFFFFFF) * view.elem_size}
            if r * view.width >= (1 << 32):
                assert unsigned - {view.addr(r)} and unsigned - {view.addr(r)} <= set(F.aliases(view, r))


def test_layout_refuses_what_it_must():
    view = F.table_view("f32", 4)
    assert F.Layout.problem([(view, [5, 5])]) and F.Layout.problem([(view, [view.rows])])
    assert "leaves the arena" in F.Layout.problem([(F.View("t", F.ARENA_BYTES - 64, 4, 4, 8), [0])])
    assert "alias" in F.Layout.problem([(F.View("t", 1 << 30, 4, 4), [1 << 29])])             # sign-wrapped: 8 GiB back
    a, b = F.View("a", F.GUARD, 4, 4, 100), F.View("b", F.GUARD + 1592, 4, 4, 100)
    assert "regions overlap" in F.Layout.problem([(a, [0]), (b, [0])])
    # a movable row under an alias is refused (pick re-draws it); the pinned row on the other side is met, not refused
    far = (1 << 30) + 7                                           # elements 2^32 + 28: narrows to row 7
    longer = F.table_view("f32", 4, rows=(1 << 30) + 16)
    assert "overlaps" in F.Layout.problem([(longer, [7, far])])
    assert F.Layout.problem([(view, [0, 1 << 30])]) is None and F.Layout([(view, [0, 1 << 30])]).met == 1


@pytest.mark.parametrize("case", F.optimizer_cases(), ids=lambda c: "%s-W%d-%s-%s" % c)
def test_optimizer_tensors_share_the_arena(case):
    kind, width, scheme, rule = case
    views = F.optimizer_views(*case)
    assert len(views) == 1 + len(F.STATE[rule]) and len({v.rows for v in views}) == 1
    table, rows = views[0], views[0].rows
    layout, picked = F.pick_shared(views, seed=5)
    for v in views:
        assert _straddled(v, picked) == len(F.thresholds(v))
    if scheme == "rows31":
        assert rows > (1 << 31) and (1 << 31) in picked and (1 << 31) - 1 in picked
    if scheme == "elems32":
        assert rows * width > (1 << 32) and max(picked) * width >= (1 << 32)
        assert any(v.width == width and v.elem_size == 4 for v in views[1:]) == ("e" in F.STATE[rule])
    if scheme == "elems31":
        assert rows * width > (1 << 31)
    assert layout.aliases and all(0 <= a and a + n <= F.ARENA_BYTES for a, n in layout.aliases)
    touched = sorted(layout.touched)
    assert len(touched) == len(picked) * len(views)
    for a, n in layout.aliases:
        assert all(a + n <= b or b + m <= a for b, m in touched)
    layout32, picked32 = F.pick_shared(views, seed=5, below=INT32)
    assert picked32 and max(picked32) < INT32


@pytest.mark.parametrize("elem_size,width", [(F.ELEM_SIZE[k], w) for k, w in F.GROUPED_TABLES] +
                         [(1, F.GROUPED_QUANTIZED_WIDTH + 8)])
def test_three_grouped_tables_share_the_arena(elem_size, width):
    views = F.grouped_views(elem_size, width)
    assert len(views) == 3 and all(b.base - a.end == F.GAP for a, b in zip(views, views[1:]))
    for below in (None, INT32):
        layout, rows = F.pick(views, seed=41, below=below)
        for v, picked in zip(views, rows):
            assert _straddled(v, picked) == len(F.thresholds(v)) >= 4          # bytes to 2^33, elements to 2^31 at least
            assert max(picked) * v.row_bytes >= (1 << 33) and max(picked) * v.width >= INT32
            assert below is not None or max(picked) * v.width >= (1 << 32)       # 4.8e9 16-bit elements, 9.6e9 bytes
        assert layout.aliases and all(0 <= a and a + n <= F.ARENA_BYTES for a, n in layout.aliases)
        touched = sorted(layout.touched)
        assert len(touched) == sum(len(r) for r in rows)
        for a, n in layout.aliases:
            assert all(a + n <= b or b + m <= a for b, m in touched)


def test_one_storage_group_and_slot_table_views():
    flat = F.flat_view()
    assert flat.row_bytes == 8 and flat.rows == sum(F.FLAT_ROW_COUNTS) and F.FLAT_ROW_COUNTS[0] > INT32
    assert flat.end <= F.ARENA_BYTES
    layout, (rows,) = F.pick([flat], seed=61)
    assert INT32 in rows and flat.rows - 1 in rows and layout.aliases
    # the rows of the second and third table narrow (as element or byte offsets) to rows 5 .. 63 of the first
    second = F.FLAT_ROW_COUNTS[0]
    assert flat.addr(5) in F.aliases(flat, second) and F.Layout.problem([(flat, rows + [second, second + 17])]) is None
    slots = F.View("slot_of_row", F.GUARD, 4, 1, rows=INT32 + 8)
    layout, (rows,) = F.pick([slots], seed=111)
    assert INT32 in rows and INT32 + 7 in rows and INT32 - 1 in rows and layout.aliases


def test_every_rule_meets_every_threshold_its_state_allows():
    cases = F.optimizer_cases()
    for rule in F.RULES:
        schemes = {s for _, _, s, r in cases if r == rule}
        assert "rows31" in schemes and "elems31" in schemes
        # two 16 GiB moments do not fit 32 GiB: Adam's element offsets stop past 2^31
        assert ("elems32" in schemes) == (rule != "adam")
        widths = {w for _, w, _, r in cases if r == rule}
        assert {256, 1000, 2056} <= widths and widths & {1, 2}
        assert {k for k, _, _, r in cases if r == rule} == {"f32", "f16", "bf16"}


def test_bags_cover_the_rows_and_remap():
    rows = [0, 1, 7, (1 << 31) - 1, 1 << 31, (1 << 32) + 3]
    ids = F.fixed_bags(rows, 5, 4, seed=3)
    assert set(ids.tolist()) == set(rows) and ids[0] == ids[1] and ids.dtype == np.int64
    assert np.array_equal(np.asarray(rows)[F.compact(ids, rows)], ids)
    idx, off = F.csr_bags(rows, 20, seed=3, offset_dtype=np.int32)
    lens = np.diff(off)
    assert off.dtype == np.int32 and off[0] == 0 and off[-1] == idx.size and set(idx.tolist()) == set(rows)
    assert lens[0] == 0 and lens[-1] == 0 and lens[5] == 70 and lens[6] == 1 and (lens[1:-1] == 0).sum() >= 2
    with pytest.raises(AssertionError):
        F.fixed_bags(rows, 5, 4, seed=3, dtype=np.int32)
    with pytest.raises(AssertionError):
        F.compact(np.array([2]), rows)
    small = F.fixed_bags(rows[:4], 3, 2, seed=1, dtype=np.int32)
    assert small.dtype == np.int32 and F.compact(small, rows[:4]).dtype == np.int32
