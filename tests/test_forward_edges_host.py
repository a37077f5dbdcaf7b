"""The conditions that keep test_gpu_forward_edges.py honest, asserted on the CPU from forward_edge_cases.py and the CPU
oracle alone.  A NaN is compared by class only, so a flood of NaNs would hide errors; in every (group, kind, B, layout)
case and every one of its four calls (sum / mean, weighted or not):

    at most one quarter of the oracle's output elements are NaN;
    at least half of the bags with lookups are clean (finite rows, finite weights, a weight sum that is not 0);
    every class and sandwich placement that forward_edge_cases.required_classes lists is there -- checked on the drawn
    ids and weights, not on the plan -- and gives what it is there for in the oracle's result.
"""
import numpy as np
import pytest
import torch

import backward_edge_model as M
import forward_edge_cases as F

DTYPE = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
GROUPS = [("same", (w,) * 3) for w in F.SAME_WIDTHS] + [("mixed", w) for w in F.MIXED] + [("mixed", None)]
ident = lambda v: "w" + "_".join(map(str, v)) if isinstance(v, tuple) else str(v)


@pytest.fixture(scope="module")
def ce():
    import cuembed_amd
    return cuembed_amd


def column_loop_widths(ce, kind):
    """The group whose widest table needs the column loop: 257 lanes of 8 bytes, one more than a workgroup has, beside a
    narrow table."""
    widths = (514, 4) if kind == "f32" else (1028, 4)
    shape = ce.mixed_group_launch_shape(DTYPE[kind], torch.int32, widths, 5)
    lane_bytes = shape["elems_per_lane"] * DTYPE[kind].itemsize
    assert shape["block_threads"] == 256 and widths[0] * DTYPE[kind].itemsize // lane_bytes == 257
    return widths


def block_starts(ce, family, kind, widths, batch, layout):
    """Stream positions at which a workgroup begins inside a table, from the launch-shape queries, for both index
    types, weighted or not."""
    hot, T = F.HOT.get(layout, 0), len(widths)
    found = []
    for index in (torch.int32, torch.int64):
        for weighted in (False, True):
            if family == "same":
                shape = ce.grouped_forward_launch_shape(DTYPE[kind], index, widths[0], T, batch, hot, hot == 0, weighted)
                per = shape["samples_per_block"]
                starts = tuple(g for g in range(per, T * batch, per) if g % batch >= 2)
            else:
                shape = ce.mixed_group_launch_shape(DTYPE[kind], index, widths, batch, hot, weighted)
                n = min(range(T), key=lambda t: (widths[t], t))
                lanes = min(widths[n] // shape["elems_per_lane"], shape["block_threads"])
                per = shape["block_threads"] // lanes
                starts = tuple(n * batch + b for b in range(per, batch, per))
            found.append(set(starts))
    # (a same-width group's bags per workgroup depend on the index type and the weights: the positions at which EVERY
    # variant begins a workgroup)
    return tuple(sorted(set.intersection(*found)))


def case_problem(ce, family, kind, widths, batch, layout):
    widths = column_loop_widths(ce, kind) if widths is None else widths
    return F.problem(kind, widths, batch, layout, block_starts(ce, family, kind, widths, batch, layout))


def test_tables_hold_the_specials_and_the_dedicated_rows():
    for kind in F.KINDS:
        for widths in F.MIXED + ((4, 4, 4),):
            for t, (values, bits) in enumerate(F.tables(kind, widths)):
                rows = F.ROWS[t]
                assert values.shape == (rows, widths[t]) and np.isposinf(values[0]).all()
                special, plain = values[:rows // 2], values[rows // 2:rows - len(F.DEDICATED)]
                assert np.isfinite(plain).all() and np.abs(plain).max() <= 1 and plain.shape[0] >= 3
                sub, big, step = F.LIMITS[kind]
                assert not np.isfinite(special).all(axis=1).all()
                if t == 0:            # (5,000 rows: every special occurs)
                    assert np.isnan(special).any() and np.isneginf(special).any() and np.any((special == 0) & np.signbit(special))
                    in_kind = lambda x: M.from_bits(kind, M.round_to_kind(kind, np.array([x], dtype=np.float32)))[0]
                    assert np.any(special == in_kind(sub)) and np.any(special == in_kind(big))
                for name, value in zip(F.DEDICATED, (-0.0, 0.0, 1.0, step / 2, big, np.inf)):
                    row = values[F.dedicated_row(rows, name)]
                    assert np.all(row == M.from_bits(kind, M.round_to_kind(kind, np.array([value], dtype=np.float32)))[0]) and np.signbit(row).all() == (name == "neg0"), (kind, name)
                assert np.array_equal(M.from_bits(kind, bits).view(np.uint32), values.view(np.uint32))


@pytest.mark.parametrize("layout", F.LAYOUTS)
@pytest.mark.parametrize("batch", F.BATCHES, ids=lambda b: "b%d" % b)
@pytest.mark.parametrize("family,widths", GROUPS, ids=ident)
@pytest.mark.parametrize("kind", F.KINDS)
def test_every_case_holds_its_classes_and_stays_mostly_clean(ce, oracle, kind, family, widths, batch, layout):
    p = case_problem(ce, family, kind, widths, batch, layout)
    widths = p["widths"]
    T, hot = len(widths), p["hot"]
    tabs = F.tables(kind, widths)
    bags = F.bag_table(p)
    lengths = p["lengths"]
    at = {(int(t), int(b)): k for k, (t, b) in enumerate(zip(bags["t"], bags["b"]))}
    cols = np.concatenate([[0], np.cumsum(widths)])
    # ---- ids in range, the layout
    for t in range(T):
        i, _, _ = F.GC.table_slice(t, batch, p["ids"], p["offsets"], hot, p["ids"])
        assert i.size == lengths[t].sum() and (i.size == 0 or (i.min() >= 0 and i.max() < F.ROWS[t]))
    if hot:
        assert np.all(lengths == hot) and p["offsets"] is None
    else:
        assert set(np.unique(lengths).tolist()) <= set(F.GC.BAG_LENGTHS) and p["offsets"][-1] == p["ids"].size
        empty = lengths == 0
        assert any(empty[t, -1] and empty[t + 1, 0] for t in range(T - 1)) or (T == 2 and p["layout"] == "csr_ragged"), \
            "no empty bags on both sides of a table boundary"
        if p["layout"] == "csr_empty_table":
            assert any(empty[t].all() for t in range(T)), "no table whose bags are all empty"
    finite_weights = p["weights"][np.isfinite(p["weights"])]
    assert set(np.unique(finite_weights).tolist()) <= set(F.WEIGHT_SET.tolist())
    if batch > 5:
        assert any(np.any((finite_weights == v) & (np.signbit(finite_weights) == np.signbit(v))) for v in F.WEIGHT_SET[-1:])
        assert {float(v) for v in np.unique(finite_weights)} == {float(v) for v in np.unique(F.WEIGHT_SET)}
    # ---- fixed hotness goes through LDS, except where the workgroup's indices (+ weights) exceed the 16 KiB staging budget
    if hot:
        for index in (torch.int32, torch.int64):
            for weighted in (False, True):
                if family == "same":
                    shape = ce.grouped_forward_launch_shape(DTYPE[kind], index, widths[0], T, batch, hot, False, weighted)
                    per = shape["samples_per_block"]
                else:
                    shape = ce.mixed_group_launch_shape(DTYPE[kind], index, widths, batch, hot, weighted)
                    per = shape["max_bags_per_block"]
                need_bytes = per * hot * (index.itemsize + (DTYPE[kind].itemsize if weighted else 0))
                assert shape["staged"] or need_bytes > 16384, (index, weighted, per, need_bytes)
                assert shape["staged"] or hot > 1
    # ---- the share of clean bags
    assert bags["clean"].mean() >= F.CLEAN_SHARE, bags["clean"].mean()
    # ---- the classes, from the drawn data
    need = F.required_classes(widths, batch, p["layout"])
    have = set(p["placed"]) | set(p["sandwiches"])
    assert need <= have, sorted(need - have)

    def lookups(t, b):
        k = at[t, b]
        lo, n = int(bags["first"][k]), int(bags["length"][k])
        return tabs[t][0][p["ids"][lo:lo + n]], p["weights"][lo:lo + n], k

    for name, (left, clean, right) in p["sandwiches"].items():
        g = [t * batch + b for t, b in (left, clean, right)]
        assert g[1] == g[0] + 1 and g[2] == g[1] + 1, name
        assert bags["clean"][at[clean]] and np.isposinf(lookups(*left)[0][-1]).all() and np.isposinf(lookups(*right)[0][0]).all()
        if name == "table":
            assert left[0] == clean[0] == right[0]
        elif name == "boundary":
            assert left[0] != right[0] and {clean[1], (left if clean[0] == right[0] else right)[1]} == {0, batch - 1}
        else:
            assert left[0] == right[0] and g[2] in block_starts(ce, family, kind, widths, batch, p["layout"])
    want = F.expected(oracle, p)
    values = {k: M.from_bits(kind, v) for k, v in want.items()}
    out_of = lambda key, t, b: values[key][b, cols[t]:cols[t + 1]]
    for cls, spots in p["placed"].items():
        for t, b in spots:
            v, w, k = lookups(t, b)
            if cls.startswith("poison"):
                assert np.isposinf(v[0]).all() and np.isposinf(v[-1]).all() and not bags["clean"][k]
            if cls == "poison0":        # Inf * 0 = NaN; a mean whose weights sum to exactly 0 over rows that hold an Inf
                assert w[-1] == 0 and not np.signbit(w[-1]) and bags["weight_sum"][k] == 0
                assert np.isnan(out_of(("sum", True), t, b)).all() and np.isnan(out_of(("mean", True), t, b)).all()
                assert np.isposinf(out_of(("sum", False), t, b)).all()
            elif cls == "poison1":      # Inf * -0.0
                assert w[0] == 0 and np.signbit(w[0]) and np.isnan(out_of(("sum", True), t, b)).all()
            elif cls == "inf_weight" or (cls == "poison2" and batch > 5):
                assert np.isposinf(w).sum() == 1 and not np.isnan(w).any()
            elif cls == "nan_weight":
                assert np.isnan(w).sum() == 1 and bags["finite_rows"][k] and np.isnan(out_of(("sum", True), t, b)).all()
                assert not np.isnan(out_of(("sum", False), t, b)).any()
            elif cls == "zero_sum":     # a mean whose weights sum to exactly 0 over finite rows: sum * 0
                assert bags["finite_rows"][k] and bags["weight_sum"][k] == 0 and np.isfinite(w).all()
                assert not out_of(("mean", True), t, b).any()
            elif cls == "neg0":         # the oracle starts every sum at +0: -0.0 alone gives +0
                assert np.all(v == 0) and np.signbit(v).all() and (hot or v.shape[0] == 1) and bags["clean"][k]
                got = out_of(("sum", False), t, b)
                assert not got.any() and not np.signbit(got).any()
            elif cls == "over" and v.shape[0] >= 2:
                assert bags["clean"][k] and np.isfinite(v).all()
                assert np.isposinf(out_of(("sum", False), t, b)).all()          # (big + big overflows fp32 as well)
            elif cls == "tie" and v.shape[0] >= 2:      # 1 + ulp / 2 rounds to even at the 16-bit store
                got = out_of(("sum", False), t, b)
                assert bags["clean"][k] and np.all(got == (1.0 + F.LIMITS[kind][2] / 2 if kind == "f32" else 1.0))
    if batch > 5 and hot != 1:
        assert any(lookups(t, b)[0].shape[0] >= 2 for t, b in p["placed"]["over"] + p["placed"]["tie"])
    # ---- the oracle's result: the NaN share, and what clean and empty bags give
    for key, v in values.items():
        assert v.shape == (batch, cols[-1])
        share = float(np.isnan(v).mean())
        assert share <= F.NAN_CAP, (key, share)
        for k in np.flatnonzero(bags["clean"]):
            assert not np.isnan(out_of(key, int(bags["t"][k]), int(bags["b"][k]))).any(), (key, k)
        for t, b in zip(*np.nonzero(lengths == 0)):
            assert not want[key][b, cols[t]:cols[t + 1]].any(), "an empty bag is +0"
    assert np.isnan(values["sum", True]).any() and np.isinf(values["sum", False]).any()


# ---- the quantized forwards ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", F.Q_LAYOUTS)
@pytest.mark.parametrize("batch", F.Q_BATCHES, ids=lambda b: "b%d" % b)
@pytest.mark.parametrize("family,widths", F.Q_CASES, ids=ident)
def test_quantized_cases_stay_mostly_clean_and_hold_the_sandwiches(ce, family, widths, batch, layout):
    """From ids and offsets alone: at least half of ALL bags are clean, a bag is poisoned exactly when it looks up a
    poisoned row, poisoned lookups with weight 0.0 and -0.0 occur, and the sandwiches stand inside a table, across every
    table boundary and (B = 300) across a workgroup boundary taken from the launch-shape queries."""
    p = F.quantized_case(family, widths, batch, layout)
    T = len(widths)
    tabs = F.quantized_tables(widths)
    lengths, flat = p["lengths"], p["lengths"].reshape(-1)
    first = np.concatenate([[0], np.cumsum(flat)])
    looks_up_poison = np.zeros((T, batch), dtype=bool)
    zero_weights = set()
    for g in np.flatnonzero(flat):
        t, b = divmod(int(g), batch)
        i, w = p["ids"][first[g]:first[g + 1]], p["weights"][first[g]:first[g + 1]]
        assert i.min() >= 0 and i.max() < F.Q_ROWS[t]
        bad = np.isin(i, tabs[t][2])
        looks_up_poison[t, b] = bad.any()
        zero_weights |= {bool(np.signbit(x)) for x in w[bad & (w == 0)]}
        if not bad.any():
            assert np.all(w != 0) and w.astype(np.float64).sum() != 0
    assert np.array_equal(looks_up_poison, p["poisoned"])
    assert zero_weights == {False, True}, "no poisoned lookup with weight 0.0 and with weight -0.0"
    assert (~p["poisoned"]).mean() >= F.CLEAN_SHARE and (~p["poisoned"])[lengths > 0].mean() >= F.CLEAN_SHARE
    assert set(np.unique(p["weights"][p["weights"] != 0]).tolist()) == set(F.Q_WEIGHTS.tolist())
    kinds = {k for k, _, _, _ in p["sandwiches"]}
    assert {"table", "boundary"} <= kinds and ("workgroup" in kinds or batch == 5)
    assert sum(k == "boundary" for k, _, _, _ in p["sandwiches"]) == T - 1
    starts = F.quantized_block_starts(family, widths, batch, layout)
    for kind, left, clean, right in p["sandwiches"]:
        g = [t * batch + b for t, b in (left, clean, right)]
        assert g[1] == g[0] + 1 and g[2] == g[1] + 1 and lengths[clean] > 0
        assert p["poisoned"][left] and not p["poisoned"][clean] and p["poisoned"][right]
        assert p["ids"][first[g[1]] - 1] in tabs[left[0]][2] and p["ids"][first[g[2]]] in tabs[right[0]][2]
        if kind == "boundary":
            assert left[0] == clean[0] == right[0] - 1 and right[1] == 0
        elif kind == "workgroup":
            assert g[2] in starts
    if not p["hot"]:
        assert np.any(lengths == 0)
        if batch > 5:
            assert lengths[T - 1, 5] == 0 and p["poisoned"][T - 1, 6]
    # the poisoned rows: every kind of poison is looked up
    for t in range(T):
        plan = F.poisoned_rows(F.Q_ROWS[t])
        assert len(plan) <= F.Q_ROWS[t] - 3 and 0 in plan          # (the 7-row table keeps three finite rows)
    seen = {F.poisoned_rows(F.Q_ROWS[t])[int(r)] for t in range(T)
            for r in F.GC.table_slice(t, batch, p["ids"], p["offsets"], p["hot"], p["ids"])[0] if int(r) in F.poisoned_rows(F.Q_ROWS[t])}
    assert seen == {"+inf", "-inf", "nan_scale"}, seen
