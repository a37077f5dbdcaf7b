"""The conditions that keep test_gpu_backward_edges.py honest, asserted on the CPU from the model and the layout alone
(backward_edge_model.py), and the model itself against the CPU oracle's loop.

A test on planted non-finite values proves something only if the planted elements sit where a kernel could leak them
and if clean results stand right next to poisoned ones.  For every exact case of backward_bits_cases.py under its forced
launch shape (host arithmetic, compute_units=256, xcds=8):

  positions   sample 0 -- what a position past nnz gathers -- is poisoned and never looked up; the sample of the last
              lookup -- what a clamped position names -- is poisoned; nnz is no multiple of the workgroup's lookups;
  run classes a single lookup, a run that ends at a segment end, spans segments of one workgroup, crosses one workgroup
              boundary, spans three workgroups, and (blocked) a run whose row an earlier block stored: each has a
              run with a non-finite result between two runs whose rows are entirely finite; one entirely finite run
              lies between two poisoned ones;
  columns     column 0, column W - 1, the first and last column of a slice are planted; every poisoned row has a clean
              column whose pair partner is poisoned; an odd W has its last column both poisoned and clean next to poison;
  classes     +Inf, -Inf, NaN from a NaN, NaN from +Inf + -Inf, a sum of -0.0 alone, and weighted NaN from Inf * 0 and
              -Inf from +Inf * -0.5 all occur;
  cap         at most one output element in four is non-finite (NaN is compared by class only);
  exactness   with the planted elements taken out, every sum of consecutive lookups is representable in the type.
"""
import functools

import numpy as np
import pytest

import backward_bits_cases as C
import backward_edge_model as M
import grouped_train_reference as R
import test_gpu_backward_bits as P
from test_backward_bits_host import EXACT_BELOW

EXACT_CASES = sorted(name for name, c in C.CASES.items() if c.data == "exact")
NAN_CAP = 0.25
ORACLE_VIEW = {"f32": np.float32, "f16": np.float16, "bf16": np.uint16}       # what the oracle takes for a kind


@pytest.fixture(scope="module")
def ce():
    import cuembed_amd
    return cuembed_amd


@functools.lru_cache(maxsize=None)
def edge_case(name):
    """(case, launch shape, inputs, the model's sums over the output rows, output row of every run)."""
    import cuembed_amd as ce
    case = C.CASES[name]
    shape = P.pinned_shape(ce, case, compute_units=256, xcds=8)
    d = M.edge_build(case, shape["segment_len"], shape["segments_per_block"])
    _, _, _, sums = M.default_backward_expected(case, d, P.EXTRA_ROWS, 0, 0)
    keys = d["runs_table"]["key"]
    row_of_run = keys if case.out == "dense" else np.searchsorted(np.unique(d["keys"]), keys)
    return case, shape, d, sums, row_of_run


def test_to_bf16_bits_keeps_every_nan_a_nan(oracle):
    nans = np.array([0x7f800001, 0x7fffffff, 0xffffffff, 0x7fc00000, 0xff800001], dtype=np.uint32)
    got = oracle.to_bf16_bits(nans.view(np.float32))
    assert np.all((got & 0x7fff) > 0x7f80), [hex(int(b)) for b in got]
    assert np.array_equal(got >> 15, nans >> 31)                                   # (the sign is kept)
    same = np.array([np.inf, -np.inf, 65536.0, -65536.0, 1.0, -0.0, 0.0, 3.3895314e38, 2.0 ** -133], dtype=np.float32)
    assert np.array_equal(oracle.to_bf16_bits(same), (same.view(np.uint32) >> 16).astype(np.uint16))
    assert np.array_equal(oracle.from_bf16_bits(oracle.to_bf16_bits(same)).view(np.uint32), same.view(np.uint32))
    # everything that is no NaN converts as before: round to nearest even on the integer pattern (65504 -> 65536)
    rng = np.random.default_rng(3)
    x = np.concatenate([rng.integers(0, 1 << 32, 100_000, dtype=np.uint64).astype(np.uint32),
                        np.array([65504.0, -65504.0], dtype=np.float32).view(np.uint32)])
    x = x[(x & 0x7fffffff) <= 0x7f800000]
    wide = x.astype(np.uint64)
    assert np.array_equal(oracle.to_bf16_bits(x.view(np.float32)), ((wide + 0x7fff + ((wide >> 16) & 1)) >> 16).astype(np.uint16))
    assert [hex(int(b)) for b in oracle.to_bf16_bits(np.array([65504.0, -65504.0], dtype=np.float32))] == ["0x4780", "0xc780"]
    # rounding to nearest even is what it was: 1 + 2^-8 is a tie (down to even), 1 + 3 * 2^-8 a tie (up to even)
    ties = np.array([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 3.4e38], dtype=np.float32)
    assert [hex(int(b)) for b in oracle.to_bf16_bits(ties)] == ["0x3f80", "0x3f82", "0x7f80"]


def test_the_comparison_rule():
    for kind in ("f32", "f16", "bf16"):
        nan, other_nan = M.special(kind, "nan"), M.special(kind, "nan") | 1 | M.special(kind, "-0")
        want = np.array([nan, M.special(kind, "+0"), M.special(kind, "+inf"), 5], dtype=M.BITS[kind])
        assert M.compare(kind, np.array([other_nan, 0, want[2], 5], dtype=M.BITS[kind]), want, kind) == (3, 1)
        for wrong in ([M.special(kind, "+inf"), 0, want[2], 5], [nan, M.special(kind, "-0"), want[2], 5],
                      [nan, 0, M.special(kind, "-inf"), 5], [nan, 0, nan, 5], [nan, 0, want[2], 4]):
            with pytest.raises(AssertionError):
                M.compare(kind, np.array(wrong, dtype=M.BITS[kind]), want, kind)
        values = np.array([np.nan, -0.0, np.inf, -np.inf, 0.25, -96.0], dtype=np.float32)
        assert np.array_equal(M.from_bits(kind, M.to_bits(kind, values)).view(np.uint32)[1:], values.view(np.uint32)[1:])
        assert M.is_nan_bits(kind, M.to_bits(kind, values)).tolist() == [True] + [False] * 5


def test_the_class_rule_on_a_handful_of_terms():
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    gy = np.array([[1, inf, -inf, nan, -0.0, inf, inf, 2],
                   [-1, 1, 1, 1, -0.0, -inf, 1, 2]], dtype=np.float32)
    sums = M.scatter_add([3, 3], [0, 1], gy, None, 5)
    assert np.array_equal(M.to_bits("f32", sums.value[3]),        # (to_bits: every NaN is the quiet NaN)
                          M.to_bits("f32", np.array([0.0, inf, -inf, nan, 0.0, nan, inf, 4.0], dtype=np.float32)))
    assert sums.nan_in[3].tolist() == [False, False, False, True, False, False, False, False]
    assert sums.both_inf[3].tolist() == [False] * 5 + [True, False, False]
    assert sums.all_negative_zero[3].tolist() == [False] * 4 + [True] + [False] * 3
    assert not sums.value[[0, 1, 2, 4]].any() and not np.signbit(sums.value[[0, 1, 2, 4]]).any() and sums.terms.tolist() == [0, 0, 0, 2, 0]
    weighted = M.scatter_add([0, 0], [0, 1], gy, np.array([0.0, -0.5], dtype=np.float32), 1)
    assert np.isnan(weighted.value[0, [1, 2, 3, 5, 6]]).all() and weighted.nan_product[0].tolist() == \
        [False, True, True, False, False, True, True, False]
    assert weighted.value[0, [0, 4, 7]].tolist() == [0.5, 0.0, -1.0] and not np.signbit(weighted.value[0, 4])
    flipped = M.scatter_add([0], [0], gy, np.array([-0.5], dtype=np.float32), 1)
    assert flipped.value[0, 1] == -inf and flipped.flipped_inf[0].tolist() == [False, True] + [False] * 3 + [True, True, False]


@pytest.mark.parametrize("name", EXACT_CASES)
def test_poisoned_positions(ce, name):
    case, shape, d, sums, _ = edge_case(name)
    block = shape["segment_len"] * shape["segments_per_block"]
    assert M.is_nan_bits(case.kind, d["grad_y_bits"][0]).all(), "sample 0 must be poisoned"
    assert not np.any(d["sids"] < 3), "sample 0 and its triple are never looked up: a NaN from it is a leak"
    last = d["last_sample"]
    assert last == d["sids"][-1] and not np.isfinite(d["grad_y"][last]).all(), "the last lookup's sample must be poisoned"
    assert d["nnz"] % block != 0 and d["nnz"] % shape["segment_len"] != 0
    if case.blocks > 1:
        assert d["nnz"] == C.BLOCKED_NNZ and (d["nnz"] - (case.blocks - 1) * d["block_len"]) % block != 0
    assert d["sids"].min() >= 3 and d["sids"].max() < C.BATCH and d["keys"].shape[0] == d["nnz"] == d["sids"].shape[0]
    # the run layout is backward_bits_cases.build's
    plain = C.build(case, shape["segment_len"], shape["segments_per_block"])
    assert np.array_equal(plain["keys"], d["keys"]) and plain["block_len"] == d["block_len"]


@pytest.mark.parametrize("name", EXACT_CASES)
def test_the_cancellation_survives(ce, name):
    """Aligned triples of lookups are the three members of one sample triple under one weight; with the planted elements
    taken out every sum of consecutive lookups of a run -- and what a row holds after each of its blocks -- is
    representable, so no order of additions can round."""
    case, shape, d, sums, _ = edge_case(name)
    sids, nnz = d["sids"], d["nnz"]
    whole = nnz // 3 * 3
    triples = sids[:whole].reshape(-1, 3)
    assert np.array_equal(triples % 3, np.tile(np.arange(3), (whole // 3, 1))) and np.all(triples // 3 == triples[:, :1] // 3)
    values = d["grad_y"][sids].astype(np.float64)
    if case.weighted:
        assert set(np.unique(d["weights"]).tolist()) == set(M.WEIGHT_SET.tolist())
        assert np.all(d["weights"][:whole].reshape(-1, 3) == d["weights"][:whole:3, None])
        with np.errstate(all="ignore"):
            values = values * d["weights"].astype(np.float64)[:, None]
    values[~np.isfinite(values)] = 0.0
    assert np.all(values * 4 == np.round(values * 4))
    clean = np.isfinite(d["grad_y"][triples]).all(axis=(1, 2))            # (a poisoned triple is bounded by the prefix test)
    assert clean.mean() > 0.5 and np.abs(values[:whole].reshape(-1, 3, case.width)[clean].sum(axis=1)).max() == 0
    prefix = np.cumsum(values, axis=0)
    first = np.concatenate([np.repeat(start + p * d["block_len"], lens) for p, start, lens, _, _ in d["runs"]])
    prefix -= np.where(first[:, None] > 0, prefix[np.maximum(first - 1, 0)], 0.0)
    assert 2 * case.blocks * np.abs(prefix).max() < EXACT_BELOW[case.kind][case.weighted]
    assert M.every_order_is_exact(case.kind, np.where(np.isfinite(sums.value), np.abs(sums.value), 0), 0.25)


@pytest.mark.parametrize("name", EXACT_CASES)
def test_run_classes_with_clean_neighbours(ce, name):
    case, shape, d, sums, row_of_run = edge_case(name)
    runs = d["runs_table"]
    poisoned_row = ~np.isfinite(sums.value).all(axis=1)
    poisoned_run = poisoned_row[row_of_run]
    same_block = np.concatenate([[False], runs["block"][1:] == runs["block"][:-1]])
    left_clean = np.concatenate([[False], ~poisoned_run[:-1]]) & same_block
    right_clean = np.concatenate([~poisoned_run[1:], [False]]) & np.concatenate([same_block[1:], [False]])
    islands = poisoned_run & left_clean & right_clean
    classes = M.run_classes(runs)
    need = {"single", "segment_end", "segments", "two_groups", "three_groups"} | ({"shared"} if case.blocks > 1 else set())
    if shape["segments_per_block"] == 1:
        need.discard("segments")          # (one segment per workgroup: test_every_run_class_is_reached counts the others)
    for cls in sorted(need):
        assert classes[cls].any(), "%s: the layout has no such run" % cls
        assert (islands & classes[cls]).any(), "%s: no poisoned run of this class between two clean ones" % cls
    # the planted lookups are where the plan says, and a poisoned run holds one
    for run, position, family, what, weight in d["planted"]:
        assert runs["first"][run] <= position < runs["first"][run] + runs["length"][run]
        assert d["sids"][position] == 3 * M.poisoned_triple(position % 3, family, what, weight) + position % 3
    has_plant = np.zeros(runs["length"].shape[0], dtype=bool)
    has_plant[[run for run, _, _, what, _ in d["planted"] if M.PLANTS[what] != "-0"]] = True
    # (a row is poisoned exactly when one of its runs holds a non-finite plant)
    by_row = np.zeros(poisoned_row.shape[0], dtype=bool)
    by_row[row_of_run[has_plant]] = True
    assert np.array_equal(by_row, poisoned_row)
    # one fully clean run between two poisoned ones
    r = d["sandwich"]
    assert r is not None and not poisoned_run[r] and poisoned_run[r - 1] and poisoned_run[r + 1] and runs["length"][r] >= 2
    spots = {position for _, position, _, _, _ in d["planted"]}
    assert int(runs["first"][r]) - 1 in spots and int(runs["first"][r] + runs["length"][r]) in spots


def test_every_run_class_is_reached(ce):
    """Every kind has cases with several segments per workgroup (so the class left out above is reached), sliced cases,
    both index types, weighted and unweighted, odd widths, every output form and sample blocks 2 and 3."""
    cases = [edge_case(name) for name in EXACT_CASES]
    for kind in ("f32", "f16", "bf16"):
        mine = [(c, s) for c, s, _, _, _ in cases if c.kind == kind]
        assert sum(s["segments_per_block"] > 1 for _, s in mine) >= 3
        assert {c.index for c, _ in mine} == {"i32", "i64"} and {c.weighted for c, _ in mine} == {True, False}
        assert {c.blocks for c, _ in mine} == {1, 2, 3} and any(c.slices > 1 for c, _ in mine)
    assert {c.out for c, _, _, _, _ in cases} == {"dense", "known", "fit", "over", "small", "pad", "skip"}
    assert {c.width for c, _, _, _, _ in cases} >= {1, 3, 2, 6, 1028, 2056}


@pytest.mark.parametrize("name", EXACT_CASES)
def test_planted_columns(ce, name):
    case, shape, d, sums, _ = edge_case(name)
    W, per = case.width, case.width // case.slices
    bad = ~np.isfinite(sums.value)
    columns = bad.any(axis=0)
    assert columns[0] and columns[W - 1]
    for s in range(case.slices):
        assert columns[s * per] and columns[(s + 1) * per - 1], "slice %d" % s
    if W >= 2:
        assert not set(M.planted_columns(0, W, case.slices)) & set(M.planted_columns(1, W, case.slices))
    rows = np.flatnonzero(bad.any(axis=1))
    assert rows.size > 0
    if W == 1:
        return            # (one column: a poisoned row has no clean one; the clean neighbours are rows)
    partner = np.arange(W) ^ 1
    has_partner = partner < W
    next_to_poison = ~bad[:, has_partner] & bad[:, partner[has_partner]]
    assert next_to_poison[rows].any(axis=1).all(), "a poisoned row without a clean column next to a poisoned one"
    if W % 2 == 1:
        assert bad[rows, W - 1].any() and (~bad[rows, W - 1]).any()
    # every clean element of a poisoned row is the exact sum of clean values: nothing but the planted columns is lost
    assert np.array_equal(bad.any(axis=0), np.isin(np.arange(W), M.planted_columns(0, W, case.slices) +
                                                    M.planted_columns(1, W, case.slices)))


@pytest.mark.parametrize("name", EXACT_CASES)
def test_classes_present_and_capped(ce, name):
    case, shape, d, sums, _ = edge_case(name)
    v = sums.value
    found = {"+inf": np.any(v == np.inf), "-inf": np.any(v == -np.inf), "nan from nan": np.any(np.isnan(v) & sums.nan_in),
             "nan from both infinities": np.any(np.isnan(v) & sums.both_inf & ~sums.nan_in & ~sums.nan_product),
             "all -0.0": np.any(sums.all_negative_zero & (v == 0) & ~np.signbit(v))}
    if case.weighted:
        found["nan from inf * 0"] = np.any(np.isnan(v) & sums.nan_product & ~sums.nan_in)
        found["-inf from +inf * -0.5"] = np.any((v == -np.inf) & sums.flipped_inf)
    assert all(found.values()), [k for k, hit in found.items() if not hit]
    # ... one of them in the run a segment STARTS with: its sum is the one that starts from the walk's first zero
    runs, row_of_run = d["runs_table"], edge_case(name)[4]
    at_start = (runs["first"] - runs["block"] * d["block_len"]) % shape["segment_len"] == 0
    assert np.any(sums.all_negative_zero[row_of_run[at_start]]), "no sum of -0.0 alone at a segment start"
    assert not np.signbit(v[v == 0]).any()
    share = float((~np.isfinite(v)).mean())          # (over the rows the call sums: a dense gradient has more, all zero)
    assert 0 < share <= NAN_CAP, share


@pytest.mark.parametrize("name", EXACT_CASES)
def test_the_model_agrees_with_the_oracle(ce, oracle, name):
    case, shape, d, sums, _ = edge_case(name)
    kind = case.kind
    as_oracle = lambda bits: None if bits is None else bits.view(ORACLE_VIEW[kind])
    dense_ids, order, unique = C.compressed_ids(d["keys"])
    index = np.int32 if case.index == "i32" else np.int64
    gy = as_oracle(d["grad_y_bits"])
    w = None if d["weights_bits"] is None else np.ascontiguousarray(as_oracle(d["weights_bits"])[order])
    keys, sids = d["keys"][order].astype(index), d["sids"][order].astype(index)
    if case.out == "dense":
        want, _ = oracle.embedding_backward(gy, case.width, d["rows"], keys, sids, None, w)
    else:
        want, inverse = oracle.embedding_backward(gy, case.width, unique, keys, sids, dense_ids.astype(index), w)
        assert np.array_equal(inverse, np.unique(d["keys"]))
    M.compare(kind, np.ascontiguousarray(want).view(M.BITS[kind]), M.to_bits(kind, sums.value), name)


# ---- reference_sums --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("kind,width", M.REFERENCE_SHAPES)
def test_reference_sums_problem(oracle, kind, width, weighted):
    """Poisoned samples are looked up at the planted positions only; the long runs without one come out finite in the
    oracle, the planted ones non-finite in planted columns only -- and the oracle's classes are the model's."""
    p = M.reference_sums_problem(kind, width, weighted)
    lengths, first, ts = p["lengths"], p["first"], p["ts"]
    assert lengths.tolist() == M.REFERENCE_LENGTHS
    nnz = ts.shape[0]
    poisoned = ts >= M.REFERENCE_BATCH
    assert np.array_equal(np.flatnonzero(poisoned), p["positions"]) and np.unique(ts[poisoned]).size == len(p["positions"])
    assert np.isfinite(M.from_bits(kind, p["grad_y_bits"][:M.REFERENCE_BATCH])).all()
    planted = M.from_bits(kind, p["grad_y_bits"][M.REFERENCE_BATCH:])
    assert np.all((~np.isfinite(planted)).any(axis=1) | ((planted == 0) & np.signbit(planted)).any(axis=1))
    spots = set(p["positions"])
    long_runs = np.flatnonzero(lengths >= M.LONG_RUN)
    for r in long_runs:
        assert first[r] == 0 or first[r] - 1 in spots
        assert first[r] + lengths[r] == nnz or first[r] + lengths[r] in spots
    assert nnz - 1 in spots
    run_of = np.repeat(np.arange(lengths.size), lengths)
    planted_runs = set(run_of[p["positions"]].tolist())
    clean_long = [r for r in long_runs if r not in planted_runs]
    assert len(clean_long) >= 4 and {3000, 9000} <= set(lengths[clean_long].tolist())
    assert any(lengths[r] >= M.LONG_RUN and first[r] < q < first[r] + lengths[r] - 1 for q in spots for r in [run_of[q]])
    assert any(lengths[r] < M.LONG_RUN and lengths[r - 1] >= M.LONG_RUN and lengths[r + 1] >= M.LONG_RUN
               for r in planted_runs if 0 < r < lengths.size - 1)
    as_oracle = lambda bits: None if bits is None else bits.view(ORACLE_VIEW[kind])
    want, _ = oracle.embedding_backward(as_oracle(p["grad_y_bits"]), width, p["ncat"], p["ti"], ts, None,
                                        as_oracle(p["weights_bits"]))
    want = M.from_bits(kind, np.ascontiguousarray(want).view(M.BITS[kind]))
    assert np.isfinite(want[p["row_ids"][clean_long]]).all(), "a long run without a planted lookup must be finite"
    sums = M.scatter_add(p["ti"], ts, M.from_bits(kind, p["grad_y_bits"]),
                         None if not weighted else M.from_bits(kind, p["weights_bits"]), p["ncat"], exact=False)
    for test in (np.isnan, np.isposinf, np.isneginf):
        assert np.array_equal(test(want), test(sums.value)), test.__name__
    if weighted:      # Inf * 0 in the middle of a long run
        zero = [q for q in spots if p["weights_bits"][q] == 0]
        assert len(zero) == 1 and lengths[run_of[zero[0]]] >= M.LONG_RUN and \
            np.isposinf(M.from_bits(kind, p["grad_y_bits"][ts[zero[0]]])).any()
    assert 0 < (~np.isfinite(want)).mean() <= NAN_CAP


# ---- the group ---------------------------------------------------------------------------------------------------------------
GROUP_CASES = [(kind, batch, width, layout) for kind in ("f32", "f16", "bf16") for batch in M.GROUP_BATCHES
               for width in M.GROUP_WIDTHS for layout in M.GROUP_LAYOUTS]


@functools.lru_cache(maxsize=None)
def group_model(kind, batch, width, layout, mode, weighted):
    """(problem, scaled grad_y as fp32 values, the model's sums over the group's global rows)."""
    p = M.group_problem(kind, batch, width, layout)
    T = len(M.GROUP_ROWS)
    w = p["weights"] if weighted else None
    gy = p["grad_y"]
    if mode == "mean":
        with np.errstate(all="ignore"):
            gy = R.mean_scale(kind, gy, R.mean_factor(T, batch, p["offsets"], p["hot"], w))
    keys, samples, _, _ = M.group_keys(batch, p)
    return p, gy, M.scatter_add(keys, samples, gy.reshape(batch * T, width), w, sum(M.GROUP_ROWS))


@pytest.mark.parametrize("kind,batch,width,layout", GROUP_CASES)
def test_group_problems_are_exactly_summable(oracle, kind, batch, width, layout):
    T = len(M.GROUP_ROWS)
    p = M.group_problem(kind, batch, width, layout)
    lengths = p["lengths"]
    assert set(np.unique(lengths).tolist()) <= set(M.POWER_LENGTHS) and lengths.sum() == p["ids"].size
    assert set(np.unique(p["weights"]).tolist()) <= set(M.WEIGHT_SET.tolist())
    starts = np.concatenate([[0], np.cumsum(lengths)])[:-1]
    weight_sums = np.array([p["weights"][s:s + n].astype(np.float64).sum() for s, n in zip(starts, lengths)])
    power = lambda x: np.all((x == 0) | (np.log2(np.where(x == 0, 1, np.abs(x))) % 1 == 0))
    assert power(lengths.astype(np.float64)) and power(weight_sums) and np.all(weight_sums >= 0)
    if layout == "csr_zero_sums":
        assert np.any((weight_sums == 0) & (lengths > 0)), "no bag whose weights sum to exactly 0"
    if layout != "h4":
        assert np.any(lengths == 0)
    plants = {what for _, _, _, what in p["planted"]}
    assert plants == set(M.PLANTS)
    # the factor of the model is an exact reciprocal: a power of two or 0
    for weighted in (False, True):
        factor = R.mean_factor(T, batch, p["offsets"], p["hot"], p["weights"] if weighted else None)
        assert power(factor.astype(np.float64))
        for mode in ("sum", "mean"):
            _, gy, sums = group_model(kind, batch, width, layout, mode, weighted)
            finite = np.where(np.isfinite(gy), gy, 0).astype(np.float64)
            assert np.all(finite * 8 == np.round(finite * 8))
            assert M.every_order_is_exact(kind, sums.scale, 0.125), (mode, weighted, float(sums.scale.max()))
            looked_up = sums.terms > 0
            share = float((~np.isfinite(sums.value[looked_up])).mean())
            assert 0 < share <= NAN_CAP, (mode, weighted, share)
            assert not np.signbit(sums.value[sums.value == 0]).any()
            if mode == "mean":
                assert np.isnan(gy).any() and np.any((gy == 0) & np.signbit(gy))
    # the model against the oracle's loop, on the sum (the stable order by global row)
    keys, samples, _, _ = M.group_keys(batch, p)
    order = np.argsort(keys, kind="stable")
    as_oracle = lambda bits: bits.view(ORACLE_VIEW[kind])
    want, _ = oracle.embedding_backward(as_oracle(p["grad_y_bits"].reshape(batch * T, width)), width, sum(M.GROUP_ROWS),
                                        keys[order], samples[order], None, as_oracle(p["weights_bits"])[order])
    M.compare(kind, np.ascontiguousarray(want).view(M.BITS[kind]),
              M.to_bits(kind, group_model(kind, batch, width, layout, "sum", True)[2].value), "oracle")


@pytest.mark.parametrize("kind", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("width", M.GROUP_WIDTHS)
def test_weight_gradient_problems(kind, width):
    """Clean lookups stand next to poisoned ones, 0 * Inf occurs, and the dot products are exact in the type."""
    tables = M.group_tables(kind, width)
    flat = np.concatenate([values for values, _ in tables])
    base = np.concatenate([[0], np.cumsum(M.GROUP_ROWS)])
    assert (~np.isfinite(flat)).any(axis=1).sum() == 3 * len(M.GROUP_ROWS)
    for batch, layout in M.WEIGHT_GRAD_CASES:
        p = M.group_problem(kind, batch, width, layout)
        keys, samples, _, _ = M.group_keys(batch, p)
        value, scale, zero_inf = M.weight_grad(flat, keys, p["grad_y"].reshape(-1, width), samples)
        assert M.every_order_is_exact(kind, scale, 1.0)
        bad = ~np.isfinite(value)
        assert 0 < bad.mean() <= NAN_CAP
        if batch > 5:
            assert zero_inf.any() and np.any(value == np.inf) and np.any(value == -np.inf)
            assert np.any(bad[1:] & ~bad[:-1]) and np.any(~bad[1:] & bad[:-1])
        M.to_bits(kind, value)
        assert np.all(base[-1] > keys)


# ---- the exchange ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,width", [("f16", 256), ("f32", 33), ("bf16", 64)])
def test_merge_problems(kind, width):
    for n, distinct, padding, capacity in M.MERGE_CASES:
        ids, bits = M.merge_problem(kind, width, n, distinct, padding, capacity)
        real = ids < M.MERGE_CATEGORIES
        k = np.unique(ids[real]).size
        assert k <= capacity, "the merge cases here all fit"
        values = M.from_bits(kind, bits)
        if (~real).any():
            pad = bits[~real]
            assert M.is_nan_bits(kind, pad).any() and (pad == M.special(kind, "+inf")).any() and \
                (pad == M.special(kind, "-inf")).any() and (pad == M.special(kind, "-0")).any()
            assert np.abs(np.where(np.isfinite(values[~real]), values[~real], 0)).max() >= {"f16": 2.0 ** 15}.get(kind, 2.0 ** 126)
        if real.any():
            uniq, inverse = np.unique(ids[real], return_inverse=True)
            sums = M.scatter_add(inverse, np.flatnonzero(real), values, None, k)
            assert M.every_order_is_exact(kind, sums.scale, 1.0)
            if n >= 5000 and padding < n:
                assert (~np.isfinite(sums.value)).any() and 0 < (~np.isfinite(sums.value)).mean() <= NAN_CAP
    assert any(np.unique(ids[ids < M.MERGE_CATEGORIES]).size == capacity
               for ids, capacity in ((M.merge_problem(kind, width, *c)[0], c[3]) for c in M.MERGE_CASES[-1:]))
