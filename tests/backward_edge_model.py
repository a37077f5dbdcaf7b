"""What the backward routes must compute on non-finite and signed-zero gradients (not a test module): numpy only, no GPU,
no oracle.  test_backward_edges_host.py asserts the conditions on the data built here, test_gpu_backward_edges.py runs
the kernels on it.

The operations, on float32 arrays that hold values of the element type:

    scatter_add     out[row, c] = sum over the row's lookups of f32(grad_y[sid, c]) [* f32(w)]
    weight_grad     grad_w[p]   = sum over c of table[row_p, c] * grad_y[sample_p, c]
    (the mean's scale is grouped_train_reference.mean_factor / mean_scale as they are)

Class rule (classify): a sum with a NaN term, or with terms of both infinities, is NaN; otherwise +Inf or -Inf if one
is among the terms; otherwise it is finite, and on the data of these tests -- small multiples of a power of two that
cancel -- the finite value is the EXACT sum, and a zero sum is +0 (every sum starts at +0, and +0 + -0 = +0).  None of
this depends on the order of the additions, so it judges fp32 partial sums, 16-bit atomics and read-modify-write alike.

Comparison rule (compare), that of test_gpu_optimizer_ieee_edges.py: where the model is NaN the device's value must be
NaN, payload and sign free; everywhere else the bits are identical -- the sign of zero, the sign of infinity and the
pattern of an untouched element included.

Inputs are bit patterns of the element type (special / to_bits), never pushed through a float conversion.
"""
import collections

import numpy as np

import backward_bits_cases as C

#: (exponent bits, mantissa bits) and the unsigned type of a kind's patterns
FORMAT = {"f32": (8, 23), "f16": (5, 10), "bf16": (8, 7)}
BITS = {"f32": np.uint32, "f16": np.uint16, "bf16": np.uint16}
#: the magnitude below which every multiple of `unit` is representable: 24 / 11 / 8 significant bits
SIGNIFICANT = {"f32": 24, "f16": 11, "bf16": 8}
WEIGHT_SET = np.array([0.5, 0.25, -0.5, 0.0], dtype=np.float32)
PLANTS = ("+inf", "-inf", "nan", "-0")


def special(kind, what):
    """The bit pattern of +inf / -inf / a quiet nan / -0 / +0 in `kind`."""
    ebits, mbits = FORMAT[kind]
    top = ((1 << ebits) - 1) << mbits
    sign = 1 << (ebits + mbits)
    return {"+inf": top, "-inf": top | sign, "nan": top | (1 << (mbits - 1)), "-0": sign, "+0": 0}[what]


def is_nan_bits(kind, bits):
    ebits, mbits = FORMAT[kind]
    return (np.asarray(bits).astype(np.int64) & ((1 << (ebits + mbits)) - 1)) > (((1 << ebits) - 1) << mbits)


def to_bits(kind, values):
    """float32 values that are REPRESENTABLE in `kind` (or non-finite) -> its bit patterns; a NaN becomes the quiet NaN."""
    v = np.ascontiguousarray(values, dtype=np.float32)
    if kind == "f32":
        out = v.view(np.uint32).copy()
    elif kind == "f16":
        with np.errstate(all="ignore"):
            h = v.astype(np.float16)
        assert np.array_equal(h.astype(np.float32)[~np.isnan(v)], v[~np.isnan(v)]), "a value is not representable in fp16"
        out = h.view(np.uint16).copy()
    else:
        x = v.view(np.uint32)
        assert np.all((x & 0xFFFF == 0) | np.isnan(v)), "a value is not representable in bf16"
        out = (x >> 16).astype(np.uint16)
    out[np.isnan(v)] = special(kind, "nan")
    return out


def from_bits(kind, bits):
    """Bit patterns of `kind` -> float32 values (exact)."""
    b = np.ascontiguousarray(bits, dtype=BITS[kind])
    if kind == "f32":
        return b.view(np.float32).copy()
    if kind == "f16":
        return b.view(np.float16).astype(np.float32)
    return (b.astype(np.uint32) << 16).view(np.float32)


def compare(kind, got_bits, want_bits, label):
    """The comparison rule.  Returns (elements compared by bits, elements compared by class)."""
    got, want = np.asarray(got_bits), np.asarray(want_bits)
    assert got.shape == want.shape, "%s: shape %r, the model has %r" % (label, got.shape, want.shape)
    by_class = is_nan_bits(kind, want)
    missing = by_class & ~is_nan_bits(kind, got)
    if missing.any():
        at = tuple(int(i) for i in np.argwhere(missing)[0])
        raise AssertionError("%s: %d elements are NaN in the model and not on the device, the first at %r: device %#x"
                             % (label, int(missing.sum()), at, int(got[at])))
    differs = (got != want) & ~by_class
    if differs.any():
        at = tuple(int(i) for i in np.argwhere(differs)[0])
        raise AssertionError("%s: %d elements differ, the first at %r: device %#x, model %#x"
                             % (label, int(differs.sum()), at, int(got[at]), int(want[at])))
    return int((~by_class).sum()), int(by_class.sum())


# ---- the class rule ----------------------------------------------------------------------------------------------------
Sums = collections.namedtuple("Sums", "value terms nan_in nan_product both_inf flipped_inf all_negative_zero scale")
# per output element: value float32 (NaN / +-Inf by the class rule, else the exact sum, +0 for a zero sum); terms = how
# many; nan_in = a term's gradient was NaN; nan_product = a term is NaN though neither factor is (Inf * 0);
# both_inf = terms of both infinities and no NaN term; flipped_inf = a term is -Inf from a +Inf gradient;
# all_negative_zero = at least one term and every term is -0.0; scale = the sum of the finite terms' magnitudes


def classify(terms64, group_starts, reasons=True):
    """terms64 [n, W] float64 (float32 products widened), n rows grouped into consecutive groups that start at
    group_starts.  Returns per group (the value of the class rule as float64, the sum of the finite terms' magnitudes,
    whether a term is NaN, whether both infinities and no NaN are among the terms; all but the value None without
    `reasons`).
    An IEEE sum in fp64 -- which cannot overflow or round on this data -- IS the class rule, in any order: NaN from a NaN
    or from both infinities, else the infinity, else the exact sum; with `reasons` that is checked against the rule
    spelled out."""
    red = lambda a: np.add.reduceat(a, group_starts, axis=0)
    with np.errstate(all="ignore"):
        value = red(terms64)
    value = np.where(value == 0, 0.0, value)                     # a zero sum is +0
    if not reasons:
        return value, None, None, None
    finite = np.isfinite(terms64)
    scale = red(np.where(finite, np.abs(terms64), 0.0))
    count = lambda mask: red(mask.astype(np.int32)) > 0
    any_nan, any_p, any_n = count(np.isnan(terms64)), count(terms64 == np.inf), count(terms64 == -np.inf)
    total = red(np.where(finite, terms64, 0.0))
    rule = np.where(any_nan | (any_p & any_n), np.nan, np.where(any_p, np.inf, np.where(any_n, -np.inf, np.where(total == 0, 0.0, total))))
    assert np.array_equal(rule.view(np.uint64) | (np.isnan(rule) * np.uint64(1 << 63)),
                          value.view(np.uint64) | (np.isnan(value) * np.uint64(1 << 63))), "the class rule and the IEEE sum differ"
    return value, scale, any_nan, any_p & any_n & ~any_nan


def scatter_add(rows_of_lookup, sids, grad_y, weights, num_rows, chunk=64, exact=True, reasons=True):
    """The scatter-add of lookups (rows_of_lookup[i], sids[i], weights[i]) -- in any order -- into num_rows rows.
    grad_y [samples, W] and weights [n] (or None) are float32 values of the element type.  exact=False: arbitrary finite
    data, of which only the classes are meant (the finite values are the fp64 sums rounded to fp32).  reasons=False
    leaves scale and the fields that say WHY an element is what it is (nan_in ... all_negative_zero) empty: value only."""
    rows_of_lookup = np.asarray(rows_of_lookup).astype(np.int64)
    order = np.argsort(rows_of_lookup, kind="stable")
    r, s = rows_of_lookup[order], np.asarray(sids).astype(np.int64)[order]
    w = None if weights is None else np.asarray(weights, dtype=np.float32)[order]
    n, W = r.shape[0], grad_y.shape[1]
    out = {k: np.zeros((num_rows, W), dtype=t) for k, t in (("value", np.float64), ("nan_in", bool), ("nan_product", bool),
                                                           ("both_inf", bool), ("flipped_inf", bool),
                                                           ("all_negative_zero", bool), ("scale", np.float64))}
    count = np.bincount(r, minlength=num_rows)
    if n:
        starts = np.flatnonzero(np.concatenate([[True], r[1:] != r[:-1]]))
        hit = r[starts]
        red = lambda a: np.add.reduceat(a.astype(np.int32), starts, axis=0) > 0
        for c0 in range(0, W, chunk):
            g = np.asarray(grad_y[:, c0:c0 + chunk], dtype=np.float32)[s]
            with np.errstate(all="ignore"):
                t = g if w is None else (g * w[:, None]).astype(np.float32)
            t64 = t.astype(np.float64)
            value, scale, any_nan, both = classify(t64, starts, reasons)
            cols = slice(c0, c0 + g.shape[1])
            out["value"][hit, cols] = value
            if not reasons:
                continue
            out["scale"][hit, cols] = scale
            out["both_inf"][hit, cols] = both
            out["nan_in"][hit, cols] = red(np.isnan(g))
            out["nan_product"][hit, cols] = red(np.isnan(t) & ~np.isnan(g)) & ~out["nan_in"][hit, cols]
            out["flipped_inf"][hit, cols] = red((t == -np.inf) & (g == np.inf))
            negative_zero = (t == 0) & np.signbit(t)
            out["all_negative_zero"][hit, cols] = ~red(~negative_zero)
    value32 = out["value"].astype(np.float32)
    finite = np.isfinite(out["value"])
    assert not exact or np.array_equal(value32.astype(np.float64)[finite], out["value"][finite]), "a finite sum is not an fp32 value"
    return Sums(value32, count, out["nan_in"], out["nan_product"], out["both_inf"], out["flipped_inf"],
                out["all_negative_zero"], out["scale"])


def every_order_is_exact(kind, scale, unit):
    """True if sums whose terms are multiples of `unit` with magnitudes adding up to `scale` (per element) are
    representable in `kind` after every addition, in any order: all partial sums are multiples of unit below
    2^significant * unit."""
    return float(np.max(scale, initial=0.0)) < unit * 2.0 ** SIGNIFICANT[kind]


def weight_grad(table, rows_of_lookup, grad_y, sample_of_lookup):
    """grad_w[p] by the class rule over the W fp32 products table[row_p, c] * grad_y[sample_p, c]; returns
    (value float32 [n], scale [n], nan_product [n]: a NaN from 0 * Inf or Inf * 0 alone)."""
    rows_of_lookup = np.asarray(rows_of_lookup).astype(np.int64)
    sample_of_lookup = np.asarray(sample_of_lookup).astype(np.int64)
    n = rows_of_lookup.shape[0]
    value, scale, zero_inf = np.zeros(n), np.zeros(n), np.zeros(n, dtype=bool)
    for lo in range(0, n, 1 << 14):
        hi = min(n, lo + (1 << 14))
        a = np.asarray(table, dtype=np.float32)[rows_of_lookup[lo:hi]]
        b = np.asarray(grad_y, dtype=np.float32)[sample_of_lookup[lo:hi]]
        with np.errstate(all="ignore"):
            t = (a * b).astype(np.float32)
        v, sc, _, _ = classify(t.astype(np.float64).reshape(-1, 1), np.arange(hi - lo) * t.shape[1])   # a group per lookup
        value[lo:hi], scale[lo:hi] = v[:, 0], sc[:, 0]
        zero_inf[lo:hi] = (np.isnan(t) & ~np.isnan(a) & ~np.isnan(b)).any(axis=1)
    value32 = value.astype(np.float32)
    finite = np.isfinite(value)
    assert np.array_equal(value32.astype(np.float64)[finite], value[finite])
    return value32, scale, zero_inf


# ---- the default backward: the exact cases of backward_bits_cases.py with planted elements -------------------------------
#: sample triple 0 is never looked up: sample 0, the stand-in of the positions past nnz, is NaN in every column.  The
#: triples 1 .. 96 have ONE poisoned member each -- member j of triple poisoned_triple(j, family, plant, weight) holds
#: PLANTS[plant] in the columns of the family (planted_columns) and the triple weighs WEIGHT_SET[weight]; its other two
#: members are clean.  The other triples are clean.
POISONED_TRIPLES = 1 + 3 * 2 * len(PLANTS) * len(WEIGHT_SET)
TRIPLES = C.BATCH // 3
RECIPES_LONG = ([(0, 0), (1, 0)], [(0, 0)], [(1, 1)], [(2, 0)], [(0, 3)], [(0, 2)], [(1, 2)], [(3, 0)])   # (plant, weight)
RECIPES_SINGLE = ([(0, 0)], [(3, 0)], [(1, 1)], [(2, 0)], [(0, 3)], [(0, 2)], [(2, 3)], [(3, 3)])
RUN_CLASSES = ("three_groups", "two_groups", "shared", "segments", "segment_end", "single")
PICKS = {"three_groups": 2, "two_groups": 2, "shared": 3, "segments": 2, "segment_end": 2, "single": 8}


def poisoned_triple(member, family, plant, weight):
    return 1 + ((weight * len(PLANTS) + plant) * 2 + family) * 3 + member


def planted_columns(family, width, slices):
    """Family 0: column 0 and the first column of every slice; family 1: column W - 1 and the last column of every slice
    (odd W >= 3: and column 1, so that the clean column 0 has a poisoned partner).  The families are disjoint from W = 2
    on, and a row poisoned by one family alone keeps a clean column c whose pair partner c ^ 1 is poisoned."""
    per = width // slices
    if family == 0:
        return sorted({s * per for s in range(slices)})
    cols = {(s + 1) * per - 1 for s in range(slices)}
    if width % 2 == 1 and width >= 3:
        cols.add(1)
    return sorted(cols)


def run_table(d, seg, per_block):
    """Per run of C.build's layout, in COO order: dict of arrays block, index (inside the block), first (global position),
    length, key, shared, groups, segments (inside one workgroup, else 0), segment_end."""
    block = seg * per_block
    cols = collections.defaultdict(list)
    for p, start, lens, key, shared in d["runs"]:
        last = start + lens - 1
        groups = last // block - start // block + 1
        cols["block"].append(np.full_like(lens, p))
        cols["index"].append(np.arange(lens.shape[0], dtype=np.int64))
        cols["first"].append(start + p * d["block_len"])
        cols["length"].append(lens)
        cols["key"].append(key)
        cols["shared"].append(shared & (p > 0))
        cols["groups"].append(groups)
        cols["segments"].append(np.where(groups == 1, last // seg - start // seg + 1, 0))
        cols["segment_end"].append((last + 1) % seg == 0)
    return {k: np.concatenate(v) for k, v in cols.items()}


def run_classes(runs):
    """name -> bool per run."""
    return {"single": runs["length"] == 1, "segment_end": runs["segment_end"], "segments": runs["segments"] >= 2,
            "two_groups": runs["groups"] == 2, "three_groups": runs["groups"] >= 3, "shared": runs["shared"]}


def edge_build(case, seg, per_block):
    """C.build's run layout for an exact case with the sample ids laid out anew: COO positions 3k, 3k + 1, 3k + 2 look up
    the members 0, 1, 2 of ONE sample triple t(k), so every aligned triple of lookups cancels as in C.build, and t(k) is
    a clean triple unless the plan below puts a poisoned one there.  Returns C.build's dict with sids, weights, grad_y
    replaced, plus grad_y_bits / weights_bits (patterns of the case's type), runs_table, planted = [(run, position,
    family, plant, weight)], sandwich = the clean run between two poisoned ones, and last_sample."""
    assert case.data == "exact"
    d = dict(C.build(case, seg, per_block))
    nnz, width = d["nnz"], case.width
    runs = run_table(d, seg, per_block)
    R = runs["length"].shape[0]
    classes = run_classes(runs)
    same_block = lambda a, b: 0 <= a < R and 0 <= b < R and runs["block"][a] == runs["block"][b]
    triple_at = {}                      # COO triple -> sample triple
    chosen, keep_clean = set(), set()   # run INDICES inside a block: a key has the same index in every block
    planted = []
    counters = {"runs": 0}
    queues = {"long": list(RECIPES_LONG), "single": list(RECIPES_SINGLE)}

    def plant(run, positions_and_recipes, family):
        taken = [p // 3 for p, _ in positions_and_recipes]
        if len(set(taken)) != len(taken) or any(k in triple_at for k in taken):
            return False
        for p, (what, weight) in positions_and_recipes:
            triple_at[p // 3] = poisoned_triple(p % 3, family, what, weight)
            planted.append((run, p, family, what, weight))
        return True

    def poison(run, non_finite=False, where="both"):
        first, length = int(runs["first"][run]), int(runs["length"][run])
        last = first + length - 1
        which = "single" if length == 1 else "long"
        recipes = queues[which]
        family = counters["runs"] % 2
        for recipe in list(recipes):            # the first recipe in the queue that fits the run goes to its end
            if non_finite and all(PLANTS[what] == "-0" for what, _ in recipe):
                continue
            if len(recipe) == 2:
                spots = [(first, recipe[0]), (last, recipe[1])]
            elif where == "first" or length == 1:
                spots = [(first, recipe[0])]
            elif where == "last":
                spots = [(last, recipe[0])]
            else:
                spots = [(first, recipe[0]), (last, recipe[0])] if last // 3 != first // 3 else [(first, recipe[0])]
            if plant(run, spots, family) or (len(spots) == 2 and len(recipe) == 1 and plant(run, spots[:1], family)):
                counters["runs"] += 1
                recipes.remove(recipe)
                recipes.append(recipe)
                chosen.add(int(runs["index"][run]))
                return True
        return False

    # the last lookup of the COO names a poisoned sample (NaN)
    last_run = R - 1
    assert plant(last_run, [(nnz - 1, (2, 0))], 0)
    chosen.add(int(runs["index"][last_run]))
    # one clean run of at least two lookups between two poisoned ones, poisoned where they touch it
    sandwich = None
    for r in range(2, R - 2):
        idx = {int(runs["index"][q]) for q in (r - 1, r, r + 1)}
        if runs["length"][r] >= 2 and same_block(r - 1, r + 1) and not (idx & (chosen | keep_clean)) and \
                runs["length"][r - 1] <= 3 and runs["length"][r + 1] <= 3:
            if not poison(r - 1, True, "last"):
                continue
            assert poison(r + 1, True, "first"), "the second half of the sandwich could not be planted"
            keep_clean.add(int(runs["index"][r]))
            sandwich = r
            break
    # per class: runs with a poisoned element whose neighbours on both sides stay clean
    for name in RUN_CLASSES:
        picked = 0
        for r in np.flatnonzero(classes[name]):
            r = int(r)
            if picked == PICKS[name]:
                break
            i = int(runs["index"][r])
            if r in (0, R - 1) or not same_block(r - 1, r + 1) or i in chosen or i in keep_clean or \
                    (i - 1) in chosen or (i + 1) in chosen:
                continue
            if poison(r, non_finite=picked == 0):
                keep_clean.update((i - 1, i + 1))
                picked += 1
    # sums of -0.0 alone: in runs that stay finite, so any run that is not poisoned will do
    zeros = 0
    for r in range(R - 1):
        if zeros < 4 and int(runs["index"][r]) not in chosen and runs["length"][r] == 1:
            zeros += plant(r, [(int(runs["first"][r]), (3, (0, 3)[zeros % 2]))], zeros % 2)
    # ---- the sample of every lookup
    k = np.arange(-(-nnz // 3), dtype=np.int64)
    clean = POISONED_TRIPLES + (C.mix(k, 0, 3) % np.uint64(TRIPLES - POISONED_TRIPLES)).astype(np.int64)
    triple = clean.copy()
    for at, t in triple_at.items():
        triple[at] = t
    i = np.arange(nnz, dtype=np.int64)
    sids = 3 * triple[i // 3] + i % 3
    # ---- grad_y: C.build's exact values, then the planted elements
    c = np.arange(width, dtype=np.int64)[None, :]
    s = np.arange(C.BATCH, dtype=np.int64)[:, None]
    grad_y = (((s + c) % 3 - 1) * (1 + (C.mix(s // 3, c, 5) % np.uint64(2)).astype(np.int64))).astype(np.float32)
    kind = case.kind
    bits = to_bits(kind, grad_y)
    bits[0, :] = special(kind, "nan")
    weight_of_triple = WEIGHT_SET[(C.mix(np.arange(TRIPLES), 0, 7) % np.uint64(len(WEIGHT_SET))).astype(np.int64)].copy()
    for member in range(3):
        for family in range(2):
            for what in range(len(PLANTS)):
                for weight in range(len(WEIGHT_SET)):
                    t = poisoned_triple(member, family, what, weight)
                    weight_of_triple[t] = WEIGHT_SET[weight]
                    sample = 3 * t + member
                    if PLANTS[what] == "-0":       # wherever the clean value is 0
                        bits[sample, grad_y[sample] == 0] = special(kind, "-0")
                    else:
                        bits[sample, planted_columns(family, width, case.slices)] = special(kind, PLANTS[what])
    weights = weight_of_triple[sids // 3] if case.weighted else None
    d.update(sids=sids, grad_y=from_bits(kind, bits), grad_y_bits=bits, weights=weights,
             weights_bits=None if weights is None else to_bits(kind, weights), runs_table=runs, planted=planted,
             sandwich=sandwich, last_sample=int(sids[-1]))
    return d


def default_backward_expected(case, d, extra_rows, pattern_bits, inverse_pattern):
    """(gradient bits, inverse_mapping or None, overflow word) that one embedding_backward call of the case must leave in
    buffers pre-filled with the patterns (test_gpu_backward_bits.run_case's call sequence)."""
    kind = case.kind
    dense_ids, order, unique = C.compressed_ids(d["keys"])
    if case.out == "dense":
        sums = scatter_add(d["keys"], d["sids"], d["grad_y"], d["weights"], d["rows"])
        return to_bits(kind, sums.value), None, False, sums
    target = np.empty_like(dense_ids)
    target[order] = dense_ids
    sums = scatter_add(target, d["sids"], d["grad_y"], d["weights"], unique)
    rows = unique + extra_rows.get(case.out, 0)
    grad = np.full((rows, case.width), pattern_bits, dtype=BITS[kind])
    inverse = np.full((rows,), inverse_pattern, dtype=np.int64)
    if case.out == "small":
        return grad, inverse, True, sums
    grad[:unique] = to_bits(kind, sums.value)
    inverse[:unique] = np.unique(d["keys"])
    if case.out == "pad":
        grad[unique:] = special(kind, "+0")
        inverse[unique:] = inverse[(np.arange(unique, rows) - unique) % unique]
    return grad, inverse, False, sums


# ---- reference_sums: arbitrary finite data, dedicated poisoned samples ------------------------------------------------------
REFERENCE_LENGTHS = [300, 1, 2, 255, 256, 257, 5, 64 * 5, 64 * 5 + 1, 64 * 6 - 1, 3, 3000, 1, 1, 9000, 7, 512, 513, 1, 700]
REFERENCE_SHAPES = [("f16", 256), ("f16", 64), ("bf16", 256), ("f32", 32), ("f16", 40), ("f32", 4)]
REFERENCE_BATCH = 5000
LONG_RUN = 257


def round_to_kind(kind, a32):
    """Finite fp32 values rounded to nearest even into `kind`, as its bit patterns."""
    a32 = np.ascontiguousarray(a32, dtype=np.float32)
    if kind == "f32":
        return a32.view(np.uint32).copy()
    if kind == "f16":
        return a32.astype(np.float16).view(np.uint16).copy()
    x = a32.view(np.uint32).astype(np.uint64)
    return ((x + 0x7fff + ((x >> 16) & 1)) >> 16).astype(np.uint16)


def reference_sums_problem(kind, width, weighted):
    """The run lengths of test_reference_sums_long_runs_through_the_workgroup_path on U(-1, 1) data; the samples
    REFERENCE_BATCH ... are poisoned and looked up only at the planted positions: the lookup just before and just after
    every long run, the last lookup of the COO, the middle of one long run (weight 0 there, when weighted) and of the
    short run between two long ones.  Returns dict(ti, ts, grad_y_bits, weights_bits, planted positions, ncat, lengths,
    row_ids, start = a buffer for skip_grad_init with rows of -0.0 and of infinities)."""
    rng = np.random.default_rng(1000 + width)
    lengths = np.array(REFERENCE_LENGTHS)
    row_ids = np.cumsum(rng.integers(1, 4, len(lengths)))
    ti = np.repeat(row_ids, lengths).astype(np.int32)
    nnz, ncat = ti.shape[0], int(row_ids[-1]) + 3
    ts = rng.integers(0, REFERENCE_BATCH, nnz).astype(np.int32)
    first = np.cumsum(lengths) - lengths
    positions = []
    for r in np.flatnonzero(lengths >= LONG_RUN):
        positions += [int(first[r]) - 1, int(first[r] + lengths[r])]
    long_middle = int(np.flatnonzero(lengths == 513)[0])
    between = int(np.flatnonzero(lengths == 7)[0])
    assert lengths[between - 1] >= LONG_RUN and lengths[between + 1] >= LONG_RUN
    positions += [nnz - 1, int(first[long_middle] + 256), int(first[between] + 3)]
    positions = sorted({p for p in positions if 0 <= p < nnz})
    gy = round_to_kind(kind, rng.uniform(-1.0, 1.0, (REFERENCE_BATCH + len(positions), width)).astype(np.float32))
    w = round_to_kind(kind, rng.uniform(0.0, 1.0, nnz).astype(np.float32))
    columns = sorted({0, width - 1, width // 2})
    for n, p in enumerate(positions):
        sample = REFERENCE_BATCH + n
        ts[p] = sample
        what = PLANTS[n % len(PLANTS)]
        if p == first[long_middle] + 256:
            what = "+inf"
            w[p] = special(kind, "+0")
        gy[sample, columns[n % len(columns)]] = special(kind, what)
        gy[sample, columns[(n + 1) % len(columns)]] = special(kind, PLANTS[(n + 2) % len(PLANTS)])
    start = round_to_kind(kind, rng.uniform(-1.0, 1.0, (ncat, width)).astype(np.float32))
    start[row_ids[::4]] = special(kind, "-0")
    start[row_ids[1::4], ::2] = special(kind, "+inf")
    start[row_ids[1::4], 1::2] = special(kind, "-inf")
    start[ncat - 1] = special(kind, "-0")                           # (a row without lookups)
    return dict(ti=ti, ts=ts, grad_y_bits=gy, weights_bits=w if weighted else None, positions=positions, ncat=ncat,
                lengths=lengths, row_ids=row_ids, first=first, start=start)


# ---- the group of grouped_cases.py: mean scale, grouped backward, weight gradient --------------------------------------------
GROUP_ROWS = (5000, 17, 300)
GROUP_BATCHES = (5, 1023)
GROUP_WIDTHS = (4, 36, 128)
GROUP_LAYOUTS = ("h4", "csr_ragged", "csr_empty_table", "csr_zero_sums")
POWER_LENGTHS = (0, 1, 2, 4, 8)
#: per bag length, weight patterns whose sum is a power of two, and (last) one whose sum is exactly 0
WEIGHT_PATTERNS = {1: ([0.5], [0.25], [0.0]), 2: ([0.25, 0.25], [0.5, 0.0], [0.5, -0.5]),
                   4: ([0.5, 0.25, 0.25, 0.0], [0.5, -0.5, 0.25, 0.25], [0.5, -0.5, 0.0, 0.0]),
                   8: ([0.5, 0.5, 0.25, 0.25, 0.25, 0.25, 0.0, 0.0], [0.5, -0.5, 0.5, 0.25, 0.25, 0.0, 0.5, -0.5],
                       [0.5, -0.5, 0.25, 0.25, -0.5, 0.0, 0.0, 0.0])}
#: (batch, layout) of the weight-gradient tests: a lookup is non-finite with its whole bag, so the small batch takes the
#: layout of many short bags
WEIGHT_GRAD_CASES = ((5, "h4"), (1023, "h4"), (1023, "csr_ragged"))
GROUP_DENSITY = 32     # one gradient element in 32 is non-zero: the 17-row table sums ~200 lookups per row at B = 1,023


def group_problem(kind, batch, width, layout):
    """One grouped call on exactly summable data: dict(ids, offsets or None, hot, weights (fp32 values) / weights_bits,
    grad_y_bits [B, T, W], grad_y (fp32 values), lengths [T * B], planted = [(b, t, column, plant)])."""
    T = len(GROUP_ROWS)
    rng = np.random.default_rng(7 * batch + width + 1000 * GROUP_LAYOUTS.index(layout))
    if layout == "h4":
        lengths, offsets, hot = np.full((T, batch), 4), None, 4
    else:
        lengths = rng.choice(POWER_LENGTHS, size=(T, batch))
        if layout == "csr_empty_table":
            lengths[1, :] = 0
        elif batch >= 3:                      # empty bags on both sides of every table boundary, next to full ones
            lengths[:, 0] = 0
            lengths[:, -1] = 0
            lengths[:, 1] = 8
        offsets, hot = np.concatenate([[0], np.cumsum(lengths.reshape(-1))]).astype(np.int64), 0
    flat = lengths.reshape(-1)
    ids = np.concatenate([rng.integers(0, GROUP_ROWS[t], int(lengths[t].sum())) for t in range(T)]).astype(np.int64)
    weights = np.zeros(ids.shape[0], dtype=np.float32)
    at = 0
    for g, n in enumerate(flat):
        if n:
            patterns = WEIGHT_PATTERNS[int(n)]
            pick = int(rng.integers(0, 2)) if layout != "csr_zero_sums" or g % 3 else 2
            weights[at:at + n] = rng.permutation(np.array(patterns[pick], dtype=np.float32))
            at += n
    values = rng.integers(-1, 2, (batch, T, width)).astype(np.float32) * rng.integers(1, 3, (batch, T, width))
    values *= rng.integers(0, GROUP_DENSITY, values.shape) == 0
    bits = to_bits(kind, values)
    planted = []
    bags = [(b, t) for t in range(T) for b in range(batch)]
    step = max(1, len(bags) // (3 if batch <= 5 else 24))
    columns = (0, width - 1, width // 2)
    # (a small batch has few bags: both infinities share one of them, in different columns)
    specs = (["+inf", "-inf"], ["nan"], ["-0"]) if batch <= 5 else (["+inf"], ["-inf"], ["nan"], ["-0"])
    for n, (b, t) in enumerate(bags[(2 if 2 < batch <= 5 else 1)::step]):    # (a small ragged batch: bag 1 is the long one)
        if n % len(specs) == 0 and lengths[t, b] == 0 and lengths[t].any():      # the infinities: a bag with lookups
            b = int(np.flatnonzero(np.roll(lengths[t], -b))[0] + b) % batch
        for k, what in enumerate(specs[n % len(specs)]):
            if what == "-0":
                bits[b, t, np.flatnonzero(values[b, t] == 0)] = special(kind, "-0")
                planted.append((b, t, -1, what))
            else:
                c = columns[(n + k) % len(columns)]
                bits[b, t, c] = special(kind, what)
                planted.append((b, t, c, what))
    return dict(ids=ids, offsets=offsets, hot=hot, weights=weights, weights_bits=to_bits(kind, weights), grad_y_bits=bits,
                grad_y=from_bits(kind, bits), lengths=flat, planted=planted)


def group_keys(batch, p):
    """(global row, row of grad_y viewed as [B * T, W], table, sample) of every lookup of a group problem."""
    T = len(GROUP_ROWS)
    base = np.concatenate([[0], np.cumsum(GROUP_ROWS)]).astype(np.int64)
    bag = np.repeat(np.arange(T * batch, dtype=np.int64), p["lengths"])
    t, b = bag // batch, bag % batch
    return base[t] + p["ids"], b * T + t, t, b


def group_tables(kind, width):
    """Tables of -1 / 0 / 1 (fp32 values and bit patterns per table); a few rows of each hold +Inf, -Inf or NaN elements."""
    out = []
    for t, rows in enumerate(GROUP_ROWS):
        rng = np.random.default_rng(500 + 10 * width + t)
        values = rng.integers(-1, 2, (rows, width)).astype(np.float32)
        bits = to_bits(kind, values)
        for n, row in enumerate((1, rows // 2, rows - 2)):
            bits[row, (0, width - 1, width // 2)[(n + t) % 3]] = special(kind, PLANTS[n])
        out.append((from_bits(kind, bits), bits))
    return out


# ---- the exchange: the owner's merge --------------------------------------------------------------------------------------
MERGE_CASES = [(6000, 1500, 700, 2000), (6000, 1500, 0, 1500), (5000, 1, 4000, 4), (64, 10, 64, 16),
               (200_000, 60_000, 30_000, 70_000), (3000, 900, 500, 900)]      # the last: count == capacity
MERGE_CATEGORIES = 500_000


def hashed_patterns(kind, shape, salt):
    """Bit patterns for rows that may hold anything: NaNs of any payload and sign, +-Inf, -0.0, huge finite values."""
    ebits, mbits = FORMAT[kind]
    n = int(np.prod(shape))
    h = C.mix(np.arange(n), salt, 41).astype(np.int64)
    top = ((1 << ebits) - 1) << mbits
    sign = (h >> 31) << (ebits + mbits)
    mantissa = (h >> 3) & ((1 << mbits) - 1)
    which = h % 5
    out = np.select([which == 0, which == 1, which == 2, which == 3],
                    [sign | top | mantissa | 1, top, top | (1 << (ebits + mbits)), 1 << (ebits + mbits)],
                    sign | (top - (1 << mbits)) | mantissa)           # the largest exponent of a finite value
    return out.astype(BITS[kind]).reshape(shape)


def merge_problem(kind, width, n, distinct, padding, capacity):
    """ids [n] (padding ids = MERGE_CATEGORIES) and rows as bit patterns: integers in the rows of real ids with a few
    planted elements, hashed patterns in the rows of padding ids.  Every id of the pool occurs when count == capacity."""
    rng = np.random.default_rng(23 + width + n)
    pool = rng.choice(MERGE_CATEGORIES, size=distinct, replace=False)
    real = n - padding if padding < n else 0
    draw = rng.integers(0, distinct, size=real)
    if real >= distinct:
        draw[:distinct] = np.arange(distinct)
    ids = np.concatenate([pool[draw], np.full((n - real,), MERGE_CATEGORIES, dtype=np.int64)]).astype(np.int64)
    rng.shuffle(ids)
    values = rng.integers(-3, 4, size=(n, width), dtype=np.int8).astype(np.float32)
    # (a row that sums a thousand lookups arrives in pieces, in any order: thinned until the magnitudes add up to < 2^8)
    values *= rng.integers(0, max(1, int(real / distinct * 1.7 / 48) + 1), size=values.shape, dtype=np.int8) == 0
    bits = to_bits(kind, values)
    is_real = np.flatnonzero(ids < MERGE_CATEGORIES)
    for k, i in enumerate(is_real[::max(1, is_real.size // 12)][:12]):
        what = PLANTS[k % len(PLANTS)]
        c = (0, width - 1, width // 2)[k % 3]
        if what == "-0":
            bits[i, values[i] == 0] = special(kind, "-0")
        else:
            bits[i, c] = special(kind, what)
    pad = np.flatnonzero(ids >= MERGE_CATEGORIES)
    bits[pad] = hashed_patterns(kind, (pad.size, width), n)
    return ids, bits
