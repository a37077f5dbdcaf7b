"""The bit contract of the sparse optimizer step, stated independently of the kernels and checked on the CPU.

optimizer_bits_reference.py is a numpy-float32 model of the five rules: one IEEE operation per line, the row sum in the
kernel's lane order, one rounding at the store.  Here it is tied to everything else that is known about the step:

  * it reproduces every fingerprint of tests/golden/optimizer_step_bits.json (recorded from the kernels on an MI355X),
    so that fixture is explained by a statement of the contract and not only by the kernels' own past;
  * on uniform random data it lies inside the fp64 bounds of optimizer_reference / adam_reference, the semantics that
    are checked against torch's optimizers;
  * a fully sequential row sum, and m' formed with a fused multiply-add, each miss fingerprints: the fixture tells those
    apart, so the model's agreement says something (Adagrad's s' = s + g * g is exact on the fixture's data, fused or
    not: only the edge data tells that apart);
  * the edge data of test_gpu_optimizer_ieee_edges.py really holds what that test is for -- asserted from the model
    alone (see edge_conditions there for what each rule and type can reach).
"""
import functools
import hashlib
import json

import numpy as np
import pytest

import adam_reference as AR
import optimizer_bits_reference as B
import optimizer_reference as OR
import test_gpu_optimizer_ieee_edges as E
import test_gpu_optimizer_step_bits as P

@pytest.fixture(scope="module")
def golden():
    with open(P.GOLDEN) as f:
        return json.load(f)


def bits_of(t, kind):
    """A CPU tensor's bit patterns as the model's array type."""
    return np.frombuffer(P.raw_bytes(t), dtype=B.BITS[kind]).reshape(tuple(t.shape)).copy()


@functools.lru_cache(maxsize=None)
def problem_bits(kind, ncat, n, tail, width):
    table, ids, rows = P.problem(kind, ncat, n, tail, width)
    return bits_of(table, kind), ids.numpy().copy(), [bits_of(g, kind) for g in rows]


def case_arguments(case):
    """(rule, kind, ncat, n, tail, width, rounding, valid) of a fingerprint case, from its id."""
    parts = case.split("-")
    group, rule = parts[0], parts[1]
    if group == "small":
        kind, width, rounding = parts[2], int(parts[3][1:]), parts[5]
        return rule, kind, P.SMALL_NCAT, P.SMALL_N, P.SMALL_TAIL, width, rounding, B.valid_entries(P.SMALL_N)
    if group == "grid":
        return rule, "f16", P.GRID_NCAT, P.GRID_N, 0, P.GRID_WIDTH, parts[2], B.valid_entries(P.GRID_N)
    assert group == "pieces"
    n = len(P.PIECE_COUNTS) * P.PIECE_ROWS
    return rule, "f16", P.SMALL_NCAT, n, 0, 64, "nearest", B.valid_entries(n, counts=P.PIECE_COUNTS,
                                                                            piece_rows=P.PIECE_ROWS)


def model_fingerprints(case, **variant):
    """test_gpu_optimizer_step_bits.fingerprints with the model in the kernels' place."""
    rule, kind, ncat, n, tail, width, rounding, valid = case_arguments(case)
    table, ids, rows = problem_bits(kind, ncat, n, tail, width)
    state = [np.zeros((ncat, width) if shape == "e" else (ncat,), dtype=np.uint32) for shape in B.STATE[rule]]
    out = []
    for t, g in zip(P.STEPS, rows):
        table, state, _ = B.step(rule, kind, table, state, ids, g, valid, lr=P.LR, eps=P.EPS,
                                 bias_factor=AR.bias_factor(t, P.BETAS), betas=P.BETAS, weight_decay=P.WEIGHT_DECAY,
                                 rounding=rounding, seed=P.SEED, step=t, **variant)
        h = hashlib.sha256(table.tobytes())
        for s in state:
            h.update(s.tobytes())
        out.append(h.hexdigest())
    return out


def test_the_bias_factor_is_the_package_s():
    """The fingerprints were recorded with cuembed_amd.adam_bias_factor; the model is given adam_reference's."""
    import cuembed_amd
    for t in P.STEPS:
        assert np.float32(AR.bias_factor(t, P.BETAS)) == np.float32(cuembed_amd.adam_bias_factor(t, P.BETAS))


def test_the_model_s_lanes_are_the_launcher_s():
    """lane_bytes / group_of against sparse_row_update_launch_shape (host arithmetic), at every width of both tests."""
    import cuembed_amd
    for kind in ("f32", "f16", "bf16"):
        for width in sorted(set(P.WIDTHS[kind]) | set(E.WIDTHS[kind]) | {36, 256, 4096}):
            shape = cuembed_amd.sparse_row_update_launch_shape(P.TORCH[kind], width, 1000)
            lane = B.lane_bytes(kind, width)
            assert shape["lane_bytes"] == lane
            assert shape["lanes_per_row"] == width * B.ELEM_SIZE[kind] // lane
            assert shape["lanes_per_entry"] == B.group_of(shape["lanes_per_row"])


@pytest.mark.parametrize("case", sorted(P.CASES))
def test_the_model_reproduces_the_recorded_fingerprint(golden, case):
    assert model_fingerprints(case) == golden["cases"][case]


def _misses(golden, rule, **variant):
    return [case for case in sorted(P.CASES) if case.split("-")[1] == rule and case.startswith("small")
            and model_fingerprints(case, **variant) != golden["cases"][case]]


@pytest.mark.parametrize("rule", ["rowwise_adagrad", "rowwise_adam"])
def test_a_sequential_row_sum_misses_fingerprints(golden, rule):
    """One accumulator over the row instead of lanes and a butterfly: the fixture notices."""
    assert _misses(golden, rule, row_sum="sequential")


@pytest.mark.parametrize("rule", ["adam", "rowwise_adam"])
def test_a_fused_multiply_add_misses_fingerprints(golden, rule):
    """m' = fma(1 - beta1, g, beta1 * m): the fixture notices."""
    assert _misses(golden, rule, fused=True)


def test_a_fused_adagrad_state_is_told_apart_by_the_edge_data_only(golden):
    """s' = fma(g, g, s): the fixture's gradients are multiples of 2^-10 below 1, so g * g and s + g * g are exact in fp32
    and the fused form leaves every fingerprint as it is -- the edge data's full mantissas tell it apart."""
    assert not _misses(golden, "adagrad", fused=True)
    p = E.edge_problem("f32", 64)
    runs = [B.step("adagrad", "f32", p["table"], E.start_state("adagrad", p), p["ids"], p["grads"][0],
                   B.valid_entries(E.N), lr=P.LR, fused=fused) for fused in (False, True)]
    assert not np.array_equal(runs[0][1][0], runs[1][1][0])


# ---- the model inside the fp64 bounds -------------------------------------------------------------------------------------
BOUND_ROWS, BOUND_N = 64, 40


def to_bits(values, kind):
    x = np.ascontiguousarray(values, dtype=np.float32)
    return x.view(np.uint32).copy() if kind == "f32" else B.S.nearest(x, B.S_KIND[kind]).astype(np.uint16)


@pytest.mark.parametrize("width", [64, 1000])
@pytest.mark.parametrize("kind", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("rule", B.RULES)
def test_the_model_lies_within_the_fp64_bounds(rule, kind, width):
    """Two steps on uniform data against optimizer_reference / adam_reference, whose formulas are the ones compared with
    torch's optimizers: worst error / bound <= 1 for the table and every state tensor, after each step."""
    rng = np.random.default_rng(width + len(rule))
    table = to_bits(rng.uniform(-1, 1, (BOUND_ROWS, width)), kind)
    ids = rng.permutation(BOUND_ROWS)[:BOUND_N].astype(np.int64)
    state = [np.zeros((BOUND_ROWS, width) if shape == "e" else (BOUND_ROWS,), dtype=np.uint32) for shape in B.STATE[rule]]
    lr, eps, wd = 0.05, 1e-8, 0.01
    k = OR.k_for(width)
    for t in (1, 2):
        g_bits = to_bits(rng.uniform(-1, 1, (BOUND_N, width)), kind)
        w64 = B.widen(table[ids], kind).astype(np.float64)
        g64 = B.widen(g_bits, kind).astype(np.float64)
        s64 = [B.f32(s[ids]).astype(np.float64) for s in state]
        c = AR.bias_factor(t)
        table, state, _ = B.step(rule, kind, table, state, ids, g_bits, B.valid_entries(BOUND_N), lr=lr, eps=eps,
                                 bias_factor=c, weight_decay=wd)
        got_w = B.widen(table[ids], kind).astype(np.float64)
        got_s = [B.f32(s[ids]).astype(np.float64) for s in state]
        if rule in OR.RULES:
            w_new, d, s_new = OR.step(rule, w64, g64, s64[0] if s64 else None, lr, eps)
            assert OR.worst_ratio(got_w, w_new, OR.weight_bound(kind, w_new, w64, d, k)) <= 1.0
            if s64:
                assert OR.worst_ratio(got_s[0], s_new, OR.state_bound(s_new, k)) <= 1.0
        else:
            r = AR.step(rule, w64, g64, s64[0], s64[1], AR.scalars(lr, c, (0.9, 0.999), eps, wd))
            assert AR.worst_ratio(got_w, r["w"], AR.weight_bound(kind, r, w64, k)) <= 1.0
            assert AR.worst_ratio(got_s[0], r["m"], AR.exp_avg_bound(r, k)) <= 1.0
            assert AR.worst_ratio(got_s[1], r["v"], AR.exp_avg_sq_bound(r, k)) <= 1.0


# ---- the edge data of test_gpu_optimizer_ieee_edges.py holds what that test is for -------------------------------------------
def share_of_nans(bits, kind):
    return float(E.nan_test(kind)(bits).mean())


@pytest.mark.parametrize("kind,width,index,rounding", [c for c in E.small_cases() if c[2] == "i32"])
@pytest.mark.parametrize("rule", B.RULES)
def test_the_edge_data_meets_its_conditions(rule, kind, width, index, rounding):
    """For every run of the GPU test's case (eps, weight_decay, lane width), from the model alone: at most 5 % of each
    compared tensor is NaN after either step; the named rows' results hold every condition of edge_conditions; rows that
    no valid entry names, and their state, keep the input's bits."""
    p = E.edge_problem(kind, width)
    named = np.sort(p["ids"][:E.N])
    unnamed = np.setdiff1d(np.arange(E.NCAT), named)
    assert named.size == E.N and np.all(p["ids"] < E.NCAT) and np.all(p["ids"] >= 0)
    start = E.start_state(rule, p)
    for eps, weight_decay, shift in E.variants(rule, kind, width):
        steps = E.model_steps(rule, kind, width, rounding, eps, weight_decay, B.lane_bytes(kind, width, shift))
        label = (eps, weight_decay, shift)
        for table, state, _ in steps:
            assert share_of_nans(table, kind) <= E.NAN_SHARE, label
            assert np.array_equal(table[unnamed], p["table"][unnamed]), label
            for s, s0 in zip(state, start):
                assert share_of_nans(s, "f32") <= E.NAN_SHARE, label
                assert np.array_equal(s[unnamed], s0[unnamed]), label
        missing = E.edge_conditions(rule, kind, eps, weight_decay, rounding) - E.edge_findings(kind, named, steps)
        assert not missing, (label, sorted(missing))


def test_the_edge_data_is_what_its_description_says():
    """The bulk is finite, every regime occurs, and inf / NaN inputs sit in the six designated rows only."""
    for kind, widths in E.WIDTHS.items():
        for width in widths:
            p = E.edge_problem(kind, width)
            k = p["classes"]
            assert set(p["regimes"][k["bulk"]]) == set(E.REGIME_OF)
            plain = np.concatenate([k[name] for name in k if name != "special"])
            rows = p["ids"][plain]
            for g in p["grads"]:
                assert np.isfinite(B.widen(g[plain], kind)).all()
                assert not np.isfinite(B.widen(g[k["special"]], kind)).all()
            assert np.isfinite(B.widen(p["table"][rows], kind)).all()
            for s in (p["e"], p["m"], p["r"]):
                assert np.isfinite(B.f32(s[rows])).all()
            assert (B.f32(p["e"]) >= 0).all() and (B.f32(p["r"]) >= 0).all()          # sqrt's argument starts non-negative
