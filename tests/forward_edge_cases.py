"""Tables and bags that carry IEEE edge values through the GROUP forwards (not a test module): numpy only, no GPU.
test_forward_edges_host.py asserts the conditions on the data built here, test_gpu_forward_edges.py runs the kernels on it.

On finite data a walk can pool one lookup too many with a zero weight and nothing shows, because 0 * x adds 0: the
neighbouring bag's lookup, the next table's, a lane past a bag's `hot` that feeds in (index 0, weight 0), a column at or
past W_t.  With an infinity in the wrong row each of these becomes 0 * Inf = NaN in the output.  So:

Tables (tables): the first half of each table's rows are drawn element by element from the specials of edge_table (+-0,
+-Inf, NaN, subnormals, values near the type's maximum, the halves of an exact tie), the other half is U(-1, 1), and the
last six rows are dedicated: all -0.0, all +0, all 1, all ulp / 2, all `big`, all +Inf.  Row 0 of every table -- what a
lane that feeds in index 0 reads -- is +Inf in every column.

Bags (problem): a bag is CLEAN when every row it looks up is finite in every column, its weights are finite and their sum
is not 0.  The rest are placed on purpose:

    poison      the first and the last lookup are the +Inf row; three of them stand around a clean bag
                  inside a table             (a, 1) poison, (a, 2) clean, (a, 3) poison, a the narrowest table with lookups
                  across a table boundary    the last bag of table t and the first of table t + 1 are one the clean bag and
                                             one a poison, with a poison on the clean bag's other side
                  across a workgroup         (g - 2) poison, (g - 1) clean, (g) poison, g the first bag of a workgroup
                                             (from the launch-shape query, handed in by the caller)
                the first one weighs its +Inf lookups 0.0 and its weights sum to exactly 0 (a mean over rows that hold an
                Inf, and Inf * 0 = NaN), the second weighs its first lookup -0.0, the third (B = 1,023) +Inf;
    zero_sum    finite rows, weights that sum to exactly 0;
    inf_weight, nan_weight   finite rows, one weight +Inf / NaN: per table at B = 1,023;
    neg0, over, tie          clean bags: the -0.0 row alone (one lookup where the layout has bag lengths), big + big
                             (overflows the 16-bit store), 1 + ulp / 2 (a tie at the store), the rest the +0 row, weights 1;
    wild        (B = 1,023, one bag in eight) up to three lookups anywhere in the specials.

What a batch of five bags per table cannot hold: at least half of the bags with lookups must stay clean, so at B = 5 the
classes are placed in the order above while that budget lasts (required_classes says what every case must hold).  A
group of two tables has ONE table boundary: csr_ragged puts the sandwich there and csr_empty_table the empty bags.
Empty bags have no row and no weight; they are counted apart (their result is +0, compared by bits) and the clean share
is taken over the bags with lookups.
"""
import functools

import numpy as np

import backward_edge_model as M
import grouped_cases as GC

ROWS = (5000, 17, 300, 64)
BATCHES = (5, 1023)
LAYOUTS = ("h1", "h7", "h26", "csr_ragged", "csr_empty_table")
HOT = {"h1": 1, "h7": 7, "h26": 26}
KINDS = ("f32", "f16", "bf16")
MODES = GC.MODES
WEIGHT_SET = np.array([0.5, 1.0, 0.25, -1.0, 0.0, -0.0], dtype=np.float32)
SAME_WIDTHS = (4, 36, 128)                      # TableGroups of three tables
MIXED = ((128, 16, 64, 32), (36, 4, 128), (6, 2, 10), (512, 8))
#: kind -> (smallest subnormal, a value near the maximum, ulp at 1)
LIMITS = {"f16": (2.0 ** -24, 60000.0, 2.0 ** -10), "bf16": (2.0 ** -133, 3.0e38, 2.0 ** -7),
          "f32": (2.0 ** -149, 3.0e38, 2.0 ** -23)}
DEDICATED = ("neg0", "zero", "one", "tie", "big", "pinf")       # the last six rows of every table, in this order
NAN_CAP, CLEAN_SHARE = 0.25, 0.5


def edge_table(rng, kind, rows, W):
    """A table of edge values of `kind` (as fp32 values exactly representable in it) plus ordinary rows."""
    sub, big, step = LIMITS[kind]
    specials = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, sub, -sub, 3 * sub, 1000 * sub, big, -big,
                         1.0, step / 2, 1.0 + step, -1.0, 0.5], dtype=np.float64)
    t = rng.uniform(-1, 1, (rows, W))
    t[: rows // 2] = specials[rng.integers(0, specials.shape[0], (rows // 2, W))]
    return t.astype(np.float32)


def dedicated_row(rows, name):
    return rows - len(DEDICATED) + DEDICATED.index(name)


@functools.lru_cache(maxsize=None)
def tables(kind, widths):
    """((fp32 values, bit patterns of `kind`) per table), made once and never changed."""
    out = []
    sub, big, step = LIMITS[kind]
    for t, w in enumerate(widths):
        rows = ROWS[t]
        t32 = edge_table(np.random.default_rng(7000 + 31 * t + w), kind, rows, w)
        t32[0] = np.inf             # what a lane that feeds in (index 0, weight 0) reads: 0 * Inf = NaN in every column
        for name, value in zip(DEDICATED, (-0.0, 0.0, 1.0, step / 2, big, np.inf)):
            t32[dedicated_row(rows, name)] = value
        bits = M.round_to_kind(kind, t32)
        values = M.from_bits(kind, bits)
        values.setflags(write=False)
        bits.setflags(write=False)
        out.append((values, bits))
    return tuple(out)


def finite_rows(values):
    return np.isfinite(values).all(axis=1)


def _zero_sum(n):
    w = np.zeros(n, dtype=np.float32)
    if n >= 4:
        w[1:3] = (1.0, -1.0)
    elif n >= 2 and n != 3:
        w[:2] = (1.0, -1.0)
    w[n // 2 + 1:][w[n // 2 + 1:] == 0] = -0.0          # zeros of both signs
    return w


@functools.lru_cache(maxsize=None)
def problem(kind, widths, batch, layout, block_starts=()):
    """One group call.  block_starts: stream positions g = t * B + b at which a workgroup begins inside a table (the caller
    takes them from the launch-shape query); the first one with room carries the workgroup sandwich.
    dict(ids int64 [nnz], offsets int64 [T * B + 1] or None, hot, weights fp32 [nnz], lengths [T, B], placed = {class:
    [(t, b)]}, sandwiches = {"table" / "boundary" / "workgroup": (left, clean, right) bags}, forced_empty)."""
    T, hot = len(widths), HOT.get(layout, 0)
    rows = ROWS[:T]
    tabs = tables(kind, widths)
    rng = np.random.default_rng(1 + 17 * batch + 1000 * LAYOUTS.index(layout) + sum(widths))
    forced_empty = set()
    if hot:
        lengths = np.full((T, batch), hot)
    else:
        lengths = rng.choice(GC.BAG_LENGTHS[1:] if batch <= 5 else GC.BAG_LENGTHS, size=(T, batch))
        if layout == "csr_empty_table":          # a table without a lookup, and an empty bag on its boundary's other side
            e = 0 if T == 2 else 2
            forced_empty = {(e, b) for b in range(batch)} | {(1, 0) if e == 0 else (e - 1, batch - 1)}
        elif T >= 3:                             # empty bags on both sides of the last table boundary
            forced_empty = {(T - 2, batch - 1), (T - 1, 0)}
        for t, b in forced_empty:
            lengths[t, b] = 0
    live = [t for t in range(T) if any((t, b) not in forced_empty for b in range(batch))]
    placed, where = {}, {}

    def free(t, b):
        return 0 <= t < T and 0 <= b < batch and (t, b) not in forced_empty and (t, b) not in where

    def place(t, b, cls, min_len=1, exact_len=None):
        assert free(t, b), (t, b, cls)
        if not hot:
            if exact_len is not None:
                lengths[t, b] = exact_len
            elif lengths[t, b] < min_len:
                lengths[t, b] = 7
        where[t, b] = cls
        placed.setdefault(cls, []).append((t, b))

    # ---- the sandwiches
    a = min(live, key=lambda t: (widths[t], t))
    sandwiches = {"table": ((a, 1), (a, 2), (a, 3))}
    place(a, 1, "poison0")
    place(a, 2, "sandwiched")
    place(a, 3, "poison1")
    last = batch - 1
    if a - 1 in live and free(a - 1, last) and free(a, 0):
        sandwiches["boundary"] = ((a - 1, last), (a, 0), (a, 1))
        place(a - 1, last, "poison2")
        place(a, 0, "sandwiched")
    else:
        for t in [a] + live:
            left = (t, last - 1)
            if t + 1 in live and (free(*left) or left == (a, 3)) and free(t, last) and free(t + 1, 0):
                sandwiches["boundary"] = (left, (t, last), (t + 1, 0))
                if free(*left):
                    place(left[0], left[1], "poison")
                place(t, last, "sandwiched")
                place(t + 1, 0, "poison2")
                break
    # ---- the classes that need a bag of their own
    with_lookups = T * batch - len(forced_empty)
    budget = with_lookups // 2 - sum(len(placed.get(c, ())) for c in ("poison0", "poison1", "poison2", "poison"))
    if batch > 5:
        for t in live:
            for b, cls in ((5, "inf_weight"), (6, "nan_weight"), (7, "zero_sum")):
                place(t, b, cls)
            place(t, 8, "neg0", exact_len=1)
            place(t, 9, "over", min_len=2)
            place(t, 10, "tie", min_len=2)
        for g in block_starts:
            t, b = divmod(int(g), batch)
            if all(free(t, b - k) for k in range(3)) and b >= 2:
                sandwiches["workgroup"] = ((t, b - 2), (t, b - 1), (t, b))
                place(t, b - 2, "poison")
                place(t, b - 1, "sandwiched")
                place(t, b, "poison")
                break
    else:
        spare = [(t, b) for t in [a] + [t for t in live if t != a] for b in range(batch) if free(t, b)]
        for cls in ("nan_weight", "zero_sum"):         # (the NaN row in the narrowest table, while it has a bag to spare)
            if budget > 0 and spare:
                place(*spare.pop(0), cls)
                budget -= 1
        for cls, kw in (("neg0", dict(exact_len=1)), ("over", dict(min_len=2)), ("tie", dict(min_len=2))):
            if spare:
                place(*spare.pop(), cls, **kw)
    # ---- ids and weights, bag by bag
    ids, weights = [], []
    for t in range(T):
        values = tabs[t][0]
        r = rows[t]
        pool = np.flatnonzero(finite_rows(values)[:r - len(DEDICATED)])
        row = lambda name: dedicated_row(r, name)
        for b in range(batch):
            n = int(lengths[t, b])
            if n == 0:
                continue
            cls = where.get((t, b))
            if cls is None and batch > 5 and rng.integers(0, 8) == 0:
                cls = "wild"
                placed.setdefault(cls, []).append((t, b))
            i = pool[rng.integers(0, pool.size, n)]
            w = WEIGHT_SET[rng.integers(0, WEIGHT_SET.size, n)].copy()
            if cls is not None and cls.startswith("poison"):
                i[0] = i[-1] = row("pinf")
                if cls == "poison0":
                    w = _zero_sum(n)
                    w[0], w[-1] = 0.0, 0.0
                else:
                    w[0] = w[-1] = 1.0
                    if cls == "poison1":
                        w[0] = -0.0
                    elif cls == "poison2" and batch > 5:
                        w[0] = np.inf
            elif cls == "zero_sum":
                w = _zero_sum(n)
            elif cls in ("inf_weight", "nan_weight"):
                w[n // 2] = np.inf if cls == "inf_weight" else np.nan
            elif cls == "neg0":
                i[:], w[:] = row("neg0"), 1.0
            elif cls == "over" and n >= 2:
                i[:], w[:] = row("zero"), 1.0
                i[:2] = row("big")
            elif cls == "tie" and n >= 2:
                i[:], w[:] = row("zero"), 1.0
                i[:2] = row("one"), row("tie")
            elif cls == "wild":
                at = rng.choice(n, size=min(n, 3), replace=False)
                i[at] = rng.integers(0, r // 2, at.size)
            else:                                  # clean: a weight sum that is not 0
                for fix in (0.5, 0.25):
                    if w.astype(np.float64).sum() == 0:
                        w[0] = fix
            ids.append(i)
            weights.append(w)
    ids = np.concatenate(ids).astype(np.int64)
    weights = np.concatenate(weights).astype(np.float32)
    offsets = None if hot else np.concatenate([[0], np.cumsum(lengths.reshape(-1))]).astype(np.int64)
    assert ids.size == lengths.sum()
    for x in (ids, weights, lengths):
        x.setflags(write=False)
    return dict(ids=ids, offsets=offsets, hot=hot, weights=weights, lengths=lengths, placed=placed, sandwiches=sandwiches,
                forced_empty=forced_empty, widths=widths, batch=batch, layout=layout, kind=kind)


def required_classes(widths, batch, layout):
    """What problem() must hold in every case (the module's docstring says why the rest cannot fit a small batch)."""
    T = len(widths)
    need = {"poison0", "poison1", "sandwiched", "table"}
    if not (T == 2 and layout == "csr_empty_table"):
        need |= {"poison2", "boundary"}
    if batch > 5:
        need |= {"inf_weight", "nan_weight", "zero_sum", "neg0", "over", "tie", "wild", "workgroup"}
    elif not (T == 2 and layout == "csr_empty_table"):
        need |= {"neg0"}
        if T >= 3:                         # fifteen bags or more: the clean classes fit, and one more bag of its own
            need |= {"over", "tie", "nan_weight"}
            if layout != "csr_empty_table":
                need |= {"zero_sum"}
    return need


def bag_table(p):
    """Per bag with lookups, in stream order: dict of arrays t, b, first, length, clean, has_inf_row, weight_sum."""
    T, batch = p["lengths"].shape
    tabs = tables(p["kind"], p["widths"])
    flat = p["lengths"].reshape(-1)
    first = np.concatenate([[0], np.cumsum(flat)])[:-1]
    out = {k: [] for k in ("t", "b", "first", "length", "clean", "has_inf_row", "weight_sum", "finite_rows")}
    for g in np.flatnonzero(flat):
        t, b = divmod(int(g), batch)
        lo, n = int(first[g]), int(flat[g])
        v = tabs[t][0][p["ids"][lo:lo + n]]
        w = p["weights"][lo:lo + n]
        with np.errstate(all="ignore"):
            s = float(w.astype(np.float64).sum())
        rows_finite = bool(np.isfinite(v).all())
        out["t"].append(t)
        out["b"].append(b)
        out["first"].append(lo)
        out["length"].append(n)
        out["finite_rows"].append(rows_finite)
        out["has_inf_row"].append(bool(np.isinf(v).any()))
        out["weight_sum"].append(s)
        out["clean"].append(rows_finite and bool(np.isfinite(w).all()) and s != 0)
    return {k: np.array(v) for k, v in out.items()}


ORACLE_VIEW = {"f32": np.float32, "f16": np.float16, "bf16": np.uint16}       # what the oracle takes for a kind
_EXPECTED = {}


def expected(oracle, p):
    """{(mode, weighted): bit patterns [B, D]}: oracle.embedding_forward once per table, concatenated; computed once per
    problem and never changed."""
    key = (p["kind"], p["widths"], p["batch"], p["layout"])
    if key not in _EXPECTED:
        kind, batch, hot = p["kind"], p["batch"], p["hot"]
        view = ORACLE_VIEW[kind]
        w_o = M.to_bits(kind, p["weights"]).view(view)
        out = {}
        for mode, weighted in MODES:
            per_table = []
            for t, (_, bits) in enumerate(tables(kind, p["widths"])):
                i, o, w = GC.table_slice(t, batch, p["ids"], p["offsets"], hot, w_o)
                per_table.append(oracle.embedding_forward(bits.view(view), i.astype(np.int32),
                                                          None if o is None else o.astype(np.int32),
                                                          np.ascontiguousarray(w) if weighted else None, batch_size=batch,
                                                          num_hots=hot, mode=mode))
            want = np.ascontiguousarray(np.concatenate(per_table, axis=1)).view(M.BITS[kind])
            want.setflags(write=False)
            out[mode, weighted] = want
        _EXPECTED[key] = out
    return _EXPECTED[key]


# ---- the quantized forwards: where a poisoned row reaches -------------------------------------------------------------------
# There is no fp32 model of the quantized walk in the suite, so nothing here predicts a VALUE.  What is predicted is the
# reach of a poisoned row -- one whose fp32 bias in the fused bytes is +Inf (-Inf in one row) or whose scale is NaN: it
# dequantizes to Inf or NaN in every column, and no later operation makes that finite -- from ids and offsets alone.
Q_ROWS = (1000, 7, 300, 64)
Q_GROUPS = {"A": (16, 128, 32, 64), "B": (8, 24, 136), "C": (4, 12, 1028, 36)}      # test_gpu_quantized_mixed_group.py
Q_SAME = (8, 36, 64)                      # the single-table and same-width calls: three tables of one width
Q_BATCHES = (5, 300)
Q_LAYOUTS = ("h9", "csr")
Q_LENGTHS = (0, 1, 3, 4, 5, 8, 9, 17, 70)
Q_REGIMES = ("normal", "offset", "constant", "uniform")       # sums of 70 weighted rows stay inside fp16's range
Q_WEIGHTS = np.array([0.5, 1.0, 0.25, -1.0], dtype=np.float32)


def poisoned_rows(rows):
    """{row: what}: +Inf bias in rows 0 (what index 0 reads) and rows - 2, and in row 1 of a table of 64 rows or more;
    -Inf bias in the last row; a NaN scale in the middle row."""
    out = {0: "+inf", rows - 2: "+inf", rows - 1: "-inf", rows // 2: "nan_scale"}
    if rows >= 64:
        out[1] = "+inf"
    return out


@functools.lru_cache(maxsize=None)
def quantized_tables(widths):
    """((fused bytes with finite rows, the same with the poisoned rows, the poisoned row ids) per table)."""
    import quantized_reference as Q
    out = []
    for t, w in enumerate(widths):
        data = Q.make_table(Q_REGIMES[t], Q_ROWS[t], w, seed=10 + t)
        if Q_REGIMES[t] == "offset":
            data = data - np.float32(1e4 - 30.0)
        clean = Q.quantize(data)
        bad = clean.copy()
        plan = poisoned_rows(Q_ROWS[t])
        for row, what in plan.items():
            if what == "nan_scale":
                bad[row, w:w + 4] = np.array([np.nan], dtype="<f4").view(np.uint8)
            else:
                bad[row, w + 4:] = np.array([np.inf if what == "+inf" else -np.inf], dtype="<f4").view(np.uint8)
        assert not np.isfinite(Q.dequant32(bad)[sorted(plan)]).any() and np.isfinite(Q.dequant32(clean)).all()
        clean.setflags(write=False)
        bad.setflags(write=False)
        out.append((clean, bad, np.array(sorted(plan), dtype=np.int64)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def quantized_problem(widths, batch, layout, block_starts=()):
    """One call on a group of len(widths) quantized tables.  Bags are clean (rows outside poisoned_rows, weights of either
    sign with a sum that is not 0) or poisoned: the first and the last lookup are rows with a +Inf bias, one more is the
    -Inf or the NaN-scale row where the bag is long enough; weights 0.0 and -0.0 on poisoned lookups of every other such
    bag.  Sandwiches (poisoned, clean, poisoned) as in problem(): inside every table, across every table boundary, and at
    the first of block_starts with room.  dict(ids, offsets or None, hot, weights fp32, lengths [T, B], poisoned [T, B],
    sandwiches = [(kind, left, clean, right)])."""
    T, hot = len(widths), 9 if layout == "h9" else 0
    rng = np.random.default_rng(5 + 13 * batch + sum(widths) + (0 if hot else 1000))
    lengths = np.full((T, batch), hot) if hot else rng.choice(Q_LENGTHS, size=(T, batch))
    role, sandwiches = {}, []

    def sandwich(kind, left, clean, right):
        if any(role.get(x, want) != want for x, want in ((left, "P"), (clean, "C"), (right, "P"))):
            return
        for x, want in ((left, "P"), (clean, "C"), (right, "P")):
            role[x] = want
            if not hot and lengths[x] == 0:
                lengths[x] = 4
        sandwiches.append((kind, left, clean, right))

    sandwich("table", (0, 1), (0, 2), (0, 3))
    for t in range(T - 1):
        sandwich("boundary", (t, batch - 2), (t, batch - 1), (t + 1, 0))
    if batch > 5:
        for t in range(1, T):
            sandwich("table", (t, 1), (t, 2), (t, 3))
        for g in block_starts:
            t, b = divmod(int(g), batch)
            if b >= 2 and b + 1 < batch - 2:
                before = len(sandwiches)
                sandwich("workgroup", (t, b - 2), (t, b - 1), (t, b))
                if len(sandwiches) > before:
                    break
    elif not hot:                          # (B = 5) an empty bag next to a poisoned one
        lengths[T - 1, 2] = 0
        role[T - 1, 2] = "C"
        role[T - 1, 1] = "P"
        lengths[T - 1, 1] = max(lengths[T - 1, 1], 3)
    if batch > 5:
        if not hot:                        # an empty bag next to a poisoned one
            lengths[T - 1, 5] = 0
            role[T - 1, 5] = "C"
            role[T - 1, 6] = "P"
            lengths[T - 1, 6] = max(lengths[T - 1, 6], 3)
    ids, weights = [], []
    poisoned = np.zeros((T, batch), dtype=bool)
    nth = 0
    for t in range(T):
        rows = Q_ROWS[t]
        plan = poisoned_rows(rows)
        pool = np.setdiff1d(np.arange(rows), sorted(plan))
        for b in range(batch):
            n = int(lengths[t, b])
            if n == 0:
                continue
            i = pool[rng.integers(0, pool.size, n)]
            w = Q_WEIGHTS[rng.integers(0, Q_WEIGHTS.size, n)].copy()
            what = role.get((t, b))
            if what == "P" or (what is None and batch > 5 and rng.integers(0, 8) == 0):
                poisoned[t, b] = True
                i[0], i[-1] = 0, rows - 2
                if n >= 3:
                    i[n // 2] = (rows - 1, rows // 2)[nth % 2]
                if nth % 2:
                    w[0], w[-1] = 0.0, -0.0
                nth += 1
            else:
                for fix in (0.5, 0.25):
                    if w.astype(np.float64).sum() == 0:
                        w[0] = fix
            ids.append(i)
            weights.append(w)
    ids = np.concatenate(ids).astype(np.int64)
    weights = np.concatenate(weights).astype(np.float32)
    offsets = None if hot else np.concatenate([[0], np.cumsum(lengths.reshape(-1))]).astype(np.int64)
    for x in (ids, weights, lengths, poisoned):
        x.setflags(write=False)
    return dict(ids=ids, offsets=offsets, hot=hot, weights=weights, lengths=lengths, poisoned=poisoned,
                sandwiches=sandwiches, widths=widths, batch=batch, layout=layout)


def quantized_block_starts(family, widths, batch, layout):
    """Stream positions at which a workgroup begins inside a table, whatever the output type, the index type and the
    weights: the same-width group's from grouped_forward_launch_shape, the mixed group's -- of its narrowest table --
    from quantized_mixed_group_launch_shape."""
    import torch
    import cuembed_amd as ce
    hot, T = (9 if layout == "h9" else 0), len(widths)
    found = []
    for out in (torch.float16, torch.float32):
        for index in (torch.int32, torch.int64):
            for weighted in (False, True):
                if family == "same":
                    per = ce.grouped_forward_launch_shape(out, index, widths[0], T, batch, hot, hot == 0, weighted,
                                                          quantized=True)["samples_per_block"]
                    found.append({g for g in range(per, T * batch, per)})
                else:
                    shape = ce.quantized_mixed_group_launch_shape(out, index, widths, batch, hot, weighted)
                    n = min(range(T), key=lambda t: (widths[t], t))
                    per = shape["block_threads"] // min(widths[n] // shape["codes_per_lane"], shape["block_threads"])
                    found.append({n * batch + b for b in range(per, batch, per)})
    return tuple(sorted(set.intersection(*found)))


Q_CASES = [("same", (w,) * 3) for w in Q_SAME] + [("mixed", w) for w in Q_GROUPS.values()]


def quantized_case(family, widths, batch, layout):
    return quantized_problem(widths, batch, layout, quantized_block_starts(family, widths, batch, layout))
