"""Host arithmetic of the far-row tests (not a test module; integers only, no torch, no GPU).

One untouched byte arena holds every tensor of a case as a VIEW: a [rows, W] table of any element size whose base lies
GUARD = 16 GiB into the arena and whose last row starts 16 GiB past the base, optimizer states at offsets of their own.
A case touches a few dozen rows of a view -- the rows on either side of every 2^31 / 2^32 threshold of the row id, the
element offset and the byte offset -- and looks up only those.

A kernel that narrowed one of the three quantities to 32 bits would form another address for such a row: an ALIAS.  This
module computes every alias (signed and unsigned narrowing of the id, of id * W and of id * row bytes), asserts that all
of them lie inside the arena -- a narrowing bug must read or write a wrong VALUE, never fault -- and that true rows,
aliases and the regions of the views sharing the arena do not overlap: a low or random row under an alias is re-picked.
Only a threshold row cannot move, and some aliases ARE threshold rows (the row at offset 2^32 narrows to row 0, the last
row below 2^33 bytes of a 144-byte row into the first one past 2^32): those hold other data instead of poison, see
Layout.  The GPU file fills every alias with a poison row and checks it after a kernel that writes.

    View(name, base, elem_size, width, rows=None)    a [rows, width] tensor at byte `base` of the arena
    thresholds(view)                                 [(what, threshold, last row below, first row at or above)] that fit
    boundary_rows(view, seed, below=None)            the rows a case touches (ascending, distinct)
    aliases(view, row)                               byte offsets (in the arena) a narrowed address of `row` starts at
    Layout([(view, rows), ...])                      the asserts; .aliases = [(byte offset, length)] to poison
    pick(views, seed, below=None)                    boundary_rows for every view, random rows re-drawn until Layout holds
    fixed_bags / csr_bags / compact                  ids over the picked rows, and their remap to 0..k-1
"""
import numpy as np

GUARD = 1 << 34                       # bytes in front of a table's base, and from its base to its last row
SLACK = 1 << 20
GAP = 4096                            # between the tensors that share the arena
ARENA_BYTES = 2 * GUARD + SLACK
ELEM_THRESHOLDS = (1 << 31, 1 << 32)
BYTE_THRESHOLDS = (1 << 31, 1 << 32, 1 << 33, 1 << 34)
ROW_THRESHOLDS = (1 << 31, 1 << 32)
RANDOM_ROWS = 6


class View:
    """A contiguous [rows, width] tensor of `elem_size`-byte elements that starts `base` bytes into the arena.  Default
    rows: the first row at or above 16 GiB past the base is the last one."""

    def __init__(self, name, base, elem_size, width, rows=None):
        self.name, self.base, self.elem_size, self.width = name, int(base), int(elem_size), int(width)
        self.row_bytes = self.elem_size * self.width
        self.rows = -(-GUARD // self.row_bytes) + 1 if rows is None else int(rows)
        assert self.base % self.elem_size == 0 and self.rows > 0 and self.row_bytes > 0

    @property
    def end(self):
        return self.base + self.rows * self.row_bytes

    def addr(self, row):
        return self.base + int(row) * self.row_bytes

    def __repr__(self):
        return "View(%s @%d, %d x %d x %dB)" % (self.name, self.base, self.rows, self.width, self.elem_size)


def thresholds(view):
    """Every threshold that both of its rows fit under: (what, threshold, last row below, first row at or above)."""
    found = []
    for what, values, unit in (("elements", ELEM_THRESHOLDS, view.width), ("bytes", BYTE_THRESHOLDS, view.row_bytes),
                               ("rows", ROW_THRESHOLDS, 1)):
        for t in values:
            first = -(-t // unit)
            if 1 <= first < view.rows:
                found.append((what, t, first - 1, first))
    return found


def boundary_rows(view, seed, below=None, random_rows=RANDOM_ROWS, low=0):
    """Rows low and low + 1 (0 and 1 unless an alias of a threshold row overlaps them in part), the last row, both sides
    of every threshold that fits, and `random_rows` seeded random rows; below: keep only rows < below (int32 ids: 2^31)."""
    limit = view.rows if below is None else min(view.rows, int(below))
    rows = {low, low + 1, view.rows - 1}
    for _, _, lo, hi in thresholds(view):
        rows.update((lo, hi))
    rng = np.random.default_rng(seed)
    rows.update(int(r) for r in rng.integers(2, limit, random_rows))
    return sorted(r for r in rows if 0 <= r < limit)


def _u32(x):
    return x & 0xFFFFFFFF


def _s32(x):
    x &= 0xFFFFFFFF
    return x - (1 << 32) if x >= (1 << 31) else x


def aliases(view, row):
    """The arena byte offsets at which a kernel would find `row` after narrowing, to 32 bits signed or unsigned, the
    row id (then times the row bytes), the element offset row * width (then times the element size) or the byte offset
    row * row_bytes.  The true address is left out."""
    row = int(row)
    found = set()
    for narrow in (_u32, _s32):
        found.add(view.base + narrow(row) * view.row_bytes)
        found.add(view.base + narrow(row * view.width) * view.elem_size)
        found.add(view.base + narrow(row * view.row_bytes))
    found.discard(view.addr(row))
    return sorted(found)


def _overlaps(intervals):
    """The first pair of overlapping (begin, end, label) intervals, or None."""
    ordered = sorted(intervals)
    for a, b in zip(ordered, ordered[1:]):
        if b[0] < a[1]:
            return a, b
    return None


def pinned_rows(view):
    """The rows a case cannot move: both sides of every threshold that fits, and the last row."""
    rows = {view.rows - 1}
    for _, _, lo, hi in thresholds(view):
        rows.update((lo, hi))
    return rows


class Layout:
    """The tensors of one case and the rows it touches in each: [(View, rows)].  Asserts, on the host:
        every view lies inside the arena and the views' regions are pairwise disjoint;
        every alias of every touched row lies inside the arena (one row long);
        touched rows are pairwise disjoint;
        no alias overlaps a touched row that the case could have moved (a low or a random row).
    An alias may meet a PINNED row (pinned_rows): exactly -- the row at element or byte offset 2^32 narrows to row 0 of a
    power-of-two row, which is then pinned too -- or in part, between two threshold rows of a row size that divides no
    power of two (144-byte rows: the last row below 2^33 bytes narrows into the first row past 2^32).  The narrowed
    access then reads other data all the same; the poison covers the alias's bytes outside every touched row.
    .aliases: the distinct (byte offset, length) pieces to fill with poison; .touched: (byte offset, length) of the true
    rows; .met: how many aliases met a pinned row."""

    def __init__(self, parts, arena_bytes=ARENA_BYTES):
        self.parts = [(v, [int(r) for r in rows]) for v, rows in parts]
        self.arena_bytes = arena_bytes
        self.error = self._check()
        assert self.error is None, self.error

    @classmethod
    def problem(cls, parts, arena_bytes=ARENA_BYTES):
        """The message of the assert that would fail, or None (pick() re-draws on it)."""
        self = cls.__new__(cls)
        self.parts = [(v, [int(r) for r in rows]) for v, rows in parts]
        self.arena_bytes = arena_bytes
        return self._check()

    def _check(self):
        regions = []
        for v, rows in self.parts:
            if v.base < 0 or v.end > self.arena_bytes:
                return "%r leaves the arena" % v
            if any(r < 0 or r >= v.rows for r in rows) or len(set(rows)) != len(rows):
                return "%r: rows outside the view or repeated" % v
            regions.append((v.base, v.end, v.name))
        hit = _overlaps(regions)
        if hit:
            return "regions overlap: %r" % (hit,)
        touched, alias = [], {}
        for v, rows in self.parts:
            pinned = pinned_rows(v)
            exact = {v.addr(0), v.addr(1)} if v.row_bytes & (v.row_bytes - 1) == 0 else set()
            for r in rows:
                touched.append((v.addr(r), v.addr(r) + v.row_bytes, "%s[%d]" % (v.name, r), r in pinned, v.addr(r) in exact))
                for a in aliases(v, r):
                    if a < 0 or a + v.row_bytes > self.arena_bytes:
                        return "alias %d of %s[%d] leaves the arena" % (a, v.name, r)
                    alias[(a, v.row_bytes)] = "alias of %s[%d]" % (v.name, r)
        hit = _overlaps(touched)
        if hit:
            return "touched rows overlap: %r" % (hit,)
        begins = sorted(touched)
        starts = np.asarray([t[0] for t in begins], dtype=np.int64)
        poison, met = [], 0
        for (a, n), label in sorted(alias.items()):
            k = int(np.searchsorted(starts, a + n))               # the rows that begin before the alias ends
            pieces, at = [], a
            hits = []
            while k > 0 and begins[k - 1][1] > a:
                hits.append(begins[k - 1])
                k -= 1
            for b, e, name, is_pinned, is_exact in reversed(hits):
                if not (is_pinned or (is_exact and (b, e - b) == (a, n))):
                    return "%s at %d overlaps %s" % (label, a, name)
                if b > at:
                    pieces.append((at, b - at))
                at = max(at, e)
            if at < a + n:
                pieces.append((at, a + n - at))
            met += bool(hits)
            poison.extend(pieces)
        self.aliases = sorted(set(poison))
        self.touched = [(t[0], t[1] - t[0]) for t in begins]
        self.met = met
        return None


def pick(views, seed, below=None, random_rows=RANDOM_ROWS):
    """boundary_rows of every view (one seed each), the random rows re-drawn until Layout's asserts hold.  Returns
    (Layout, [rows of view 0, rows of view 1, ...])."""
    for attempt in range(64):                                     # (the low rows move first, then the random rows)
        rows = [boundary_rows(v, seed + 1000 * (attempt // 8) + 17 * k, below, random_rows, 2 * (attempt % 8))
                for k, v in enumerate(views)]
        parts = list(zip(views, rows))
        if Layout.problem(parts) is None:
            return Layout(parts), rows
    raise AssertionError("no disjoint pick for %r: %s" % (views, Layout.problem(parts)))


def pick_shared(views, seed, below=None, random_rows=RANDOM_ROWS):
    """pick() for tensors that are addressed with the SAME row ids (a table and its optimizer states): the rows are
    those of views[0], the views must have its row count, and Layout holds for all of them together."""
    assert all(v.rows == views[0].rows for v in views)
    for attempt in range(64):
        low = 2 * (attempt % 8)
        rows = boundary_rows(views[0], seed + 1000 * (attempt // 8), below, random_rows, low)
        for v in views[1:]:
            rows = sorted(set(rows) | set(boundary_rows(v, seed, below, 0, low)))
        parts = [(v, rows) for v in views]
        if Layout.problem(parts) is None:
            return Layout(parts), rows
    raise AssertionError("no disjoint pick for %r: %s" % (views, Layout.problem(parts)))


# ---- ids over the picked rows ------------------------------------------------------------------------------------------
def fixed_bags(rows, batch, hot, seed, dtype=np.int64):
    """batch * hot ids drawn from `rows`: every row at least once (when batch * hot allows), the rest seeded random
    draws -- so rows repeat, inside a bag too."""
    rng = np.random.default_rng(seed)
    rows = np.asarray(rows, dtype=np.int64)
    n = batch * hot
    ids = rows[rng.integers(0, rows.size, n)]
    if n >= rows.size:
        ids[rng.permutation(n)[:rows.size]] = rows
    if n >= 2 and hot >= 2:
        ids[1] = ids[0]                                           # a repeat inside the first bag
    assert dtype == np.int64 or ids.max() < (1 << 31)
    return ids.astype(dtype)


def csr_bags(rows, batch, seed, longest=70, dtype=np.int64, offset_dtype=np.int64):
    """Ragged bags over `rows`: lengths in [0, 14] with empty bags (first, last, two inside), one bag of one lookup and
    one of `longest` (more than a wavefront of lane groups).  Returns (ids, offsets); every row is looked up."""
    assert batch >= 16
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 15, batch)
    lens[[0, 7, 8, batch - 1]] = 0
    lens[5] = longest
    lens[6] = 1
    offsets = np.concatenate([[0], np.cumsum(lens)])
    rows = np.asarray(rows, dtype=np.int64)
    n = int(offsets[-1])
    assert n >= rows.size
    ids = rows[rng.integers(0, rows.size, n)]
    ids[rng.permutation(n)[:rows.size]] = rows
    assert dtype == np.int64 or ids.max() < (1 << 31)
    return ids.astype(dtype), offsets.astype(offset_dtype)


def compact(ids, rows):
    """ids over the ascending distinct `rows` -> their positions 0..k-1 (the ids of the compact copy)."""
    rows = np.asarray(rows, dtype=np.int64)
    ids = np.asarray(ids)
    pos = np.searchsorted(rows, ids.astype(np.int64))
    assert np.array_equal(rows[pos], ids.astype(np.int64)), "an id names a row that was not picked"
    return pos.astype(ids.dtype)


# ---- what the GPU file looks up: the host test checks exactly these ----------------------------------------------------
ELEM_SIZE = {"f32": 4, "f16": 2, "bf16": 2}
#: forward / weight-gradient tables: (kind, width, bytes the base is shifted past 16 GiB, lane bytes, int32 ids too).
#: Lanes of 4 / 8 / 16 bytes through the row size (4-, 8- and 16-byte rows: ids to 2^32 resp. 2^31) and through a shifted
#: base; W = 36 in fp32 is nine lanes -- they divide no wavefront: the global index source.  int32 ids need W >= 2 to
#: pass 2^31 elements.
FORWARD_TABLES = (
    ("f32", 1, 0, 4, False), ("f32", 2, 0, 8, True), ("f32", 4, 0, 16, True), ("f32", 36, 0, 16, True),
    ("f32", 64, 0, 16, True), ("f32", 64, 4, 4, True), ("f32", 64, 8, 8, True),
    ("f16", 2, 0, 4, True), ("f16", 4, 0, 8, True), ("f16", 8, 0, 16, True), ("f16", 64, 0, 16, True),
    ("f16", 64, 4, 4, True),
    ("bf16", 2, 0, 4, True), ("bf16", 8, 0, 16, True), ("bf16", 64, 8, 8, True),
)
#: the weight gradient's other lane groups: rows wider than a wavefront of lanes
WEIGHT_GRAD_TABLES = tuple(c[:3] for c in FORWARD_TABLES if c[1] in (2, 8, 36, 64)) + (("f16", 256, 0), ("f32", 1024, 0))
#: grouped forward: three 16-bit tables of 9 GiB in one arena (grouped_views): 4.8e9 elements each
GROUPED_TABLES = (("f16", 8), ("bf16", 64))
GROUPED_QUANTIZED_WIDTH = 64
GROUPED_BYTES = 9 << 30
#: fused 8-bit tables: (codes per row W, base shift, codes per lane of the forward); the row is W + 8 bytes
QUANTIZED_TABLES = ((64, 0, 16), (8, 0, 8), (12, 0, 4), (64, 4, 4))
#: the backward's dense gradient: at most 2^31 - 1 rows (the row count is a 32-bit int of the API)
BACKWARD_TABLES = (("f32", 2), ("f32", 64), ("f16", 4), ("f16", 64), ("bf16", 8), ("bf16", 128))
BACKWARD_MAX_ROWS = (1 << 31) - 1


def table_view(kind, width, shift=0, rows=None, name="table"):
    return View(name, GUARD + shift, ELEM_SIZE[kind], width, rows)


def quantized_view(width, shift=0, name="qtable"):
    return View(name, GUARD + shift, 1, width + 8)


def grouped_views(elem_size, width):
    """Three [rows, width] tables of 9 GiB each whose bases lie 9 GiB + 4 KiB apart, the first 4 GiB + 4 KiB in: a
    2-byte element's sign-wrapped offset reaches 4 GiB back, a byte offset 2 GiB."""
    rows = GROUPED_BYTES // (elem_size * width)
    return [View("table%d" % t, (1 << 32) + GAP + t * (GROUPED_BYTES + GAP), elem_size, width, rows) for t in range(3)]


#: one storage, three tables: the global row ids of the second and third start past 2^31
FLAT_ROW_COUNTS = ((1 << 31) + 5, 17, 42)


def flat_view():
    return table_view("f32", 2, rows=sum(FLAT_ROW_COUNTS), name="flat")


def backward_view(kind, width):
    v = table_view(kind, width, name="grad")
    return table_view(kind, width, rows=min(v.rows, BACKWARD_MAX_ROWS), name="grad")


# ---- optimizer: table and states in one arena -------------------------------------------------------------------------
RULES = ("sgd", "adagrad", "rowwise_adagrad", "adam", "rowwise_adam")
#: the state tensors of a rule: "e" = fp32 per element [rows, W], "r" = fp32 per row [rows]
STATE = {"sgd": "", "adagrad": "e", "rowwise_adagrad": "r", "adam": "ee", "rowwise_adam": "er"}
#: rows of a scheme: ids past 2^31; element offsets (per-element state: rows * W) past 2^32; past 2^31
SCHEMES = {"rows31": lambda w: (1 << 31) + 5, "elems32": lambda w: -(-(1 << 32) // w) + 5,
           "elems31": lambda w: -(-(1 << 31) // w) + 5}
#: (kind, width, scheme): W = 1 / 2 (4-byte rows) and 256 take one slice per lane, 1000 four, 2056 the any-width loop
OPTIMIZER_TABLES = (("f32", 1, "rows31"), ("f16", 2, "rows31"), ("bf16", 2, "rows31"),
                    ("f16", 256, "elems32"), ("bf16", 1000, "elems32"), ("f16", 2056, "elems32"),
                    ("f32", 256, "elems31"), ("bf16", 256, "elems31"), ("f16", 1000, "elems31"), ("f32", 2056, "elems31"))
STATE_BASE = 1 << 33                  # a per-element or per-row fp32 tensor's sign-wrapped offset reaches 8 GiB back
ROW_STATE_BASE = (1 << 32) + (1 << 24)   # a per-row tensor of less than 2^31 rows: 2 GiB back; off the powers of two


def optimizer_views(kind, width, scheme, rule):
    """[table, state...] (STATE[rule]'s order) of one optimizer case, or None when they, or the aliases of their pinned
    rows, do not fit the arena (two 16 GiB moments; a state of 8-byte rows and 2^31 of them: its id wraps 16 GiB back).
    The per-row tensor lies at 4 GiB when it is small, everything else from 8 GiB up, 4 KiB apart, the table last."""
    rows = SCHEMES[scheme](width)
    at, states = STATE_BASE, []
    for k, what in enumerate(STATE[rule]):
        if what == "r" and 4 * rows <= STATE_BASE - ROW_STATE_BASE - GAP:
            states.append(View("row_state", ROW_STATE_BASE, 4, 1, rows))
            continue
        v = View("state%d" % k, at, 4, width if what == "e" else 1, rows)
        states.append(v)
        at = v.end + GAP
    views = [View("table", at, ELEM_SIZE[kind], width, rows)] + states
    pinned = sorted(set().union(*(pinned_rows(v) for v in views)))
    return views if Layout.problem([(v, pinned) for v in views]) is None else None


def optimizer_cases():
    """[(kind, width, scheme, rule)] that fit."""
    return [(k, w, s, rule) for k, w, s in OPTIMIZER_TABLES for rule in RULES if optimizer_views(k, w, s, rule)]
