"""The conditions that keep test_gpu_mixed_group_backward_edges.py honest, asserted on the CPU from
backward_edge_model.mixed_group_problem alone: the sums are exact in any order, every plant value is looked up, the edge
columns of every table's slice of grad_y hold a looked-up +Inf (column c_{t + 1} + 0 lies directly beside table t's last
column), and at most one expected element in four is NaN (a NaN is compared by class only).
"""
import functools

import numpy as np
import pytest

import backward_edge_model as M
import grouped_train_reference as R
import mixed_group_backward_reference as MR

NAN_CAP = 0.25
KINDS = ("f32", "f16", "bf16")
CASES = [(kind, batch, widths, layout) for kind in KINDS for batch in M.GROUP_BATCHES for widths in M.MIXED_WIDTHS
         for layout in M.GROUP_LAYOUTS]
ident = lambda v: "w" + "_".join(map(str, v)) if isinstance(v, tuple) else str(v)


def scaled_grad_y(kind, batch, p, weighted):
    """The mean's scale of grad_y [B, D] as fp32 values: grouped_train_reference's factor and rounding per table slice."""
    T, cols = len(p["widths"]), MR.column_base(p["widths"])
    factor = R.mean_factor(T, batch, p["offsets"], p["hot"], p["weights"] if weighted else None)
    with np.errstate(all="ignore"):
        return np.concatenate([R.mean_scale(kind, p["grad_y"][:, None, cols[t]:cols[t + 1]], factor[:, t:t + 1])[:, 0, :]
                               for t in range(T)], axis=1)


@functools.lru_cache(maxsize=None)
def mixed_model(kind, batch, widths, layout, mode, weighted):
    """(problem, grad_y as the scatter reads it (fp32 values, [B, D]), the model's sums per table over the table's rows)."""
    p = M.mixed_group_problem(kind, batch, widths, layout)
    gy = scaled_grad_y(kind, batch, p, weighted) if mode == "mean" else p["grad_y"]
    cols = MR.column_base(widths)
    _, sample, table = M.mixed_group_keys(batch, p)
    sums = []
    for t, rows in enumerate(p["rows"]):
        mine = table == t
        w = p["weights"][mine] if weighted else None
        sums.append(M.scatter_add(p["ids"][mine], sample[mine], gy[:, cols[t]:cols[t + 1]], w, rows))
    return p, gy, sums


@pytest.mark.parametrize("kind,batch,widths,layout", CASES, ids=ident)
def test_mixed_group_problems_are_exactly_summable_and_planted(kind, batch, widths, layout):
    p = M.mixed_group_problem(kind, batch, widths, layout)
    T, cols = len(widths), MR.column_base(widths)
    lengths = p["lengths"]
    assert p["grad_y_bits"].shape == (batch, sum(widths)) and p["rows"] == M.MIXED_ROWS[:T]
    assert set(np.unique(lengths).tolist()) <= set(M.POWER_LENGTHS) and lengths.sum() == p["ids"].size
    assert set(np.unique(p["weights"]).tolist()) <= set(M.WEIGHT_SET.tolist())
    starts = np.concatenate([[0], np.cumsum(lengths)])[:-1]
    weight_sums = np.array([p["weights"][s:s + n].astype(np.float64).sum() for s, n in zip(starts, lengths)])
    if layout == "csr_zero_sums":
        assert np.any((weight_sums == 0) & (lengths > 0)), "no bag whose weights sum to exactly 0"
    if layout != "h4":
        assert np.any(lengths == 0)
    # ---- the plants: every value occurs, and is looked up by at least one row
    per_bag = lengths.reshape(T, batch)
    assert {what for _, _, _, what in p["planted"]} == set(M.PLANTS)
    looked_up = {what for b, t, _, what in p["planted"] if per_bag[t, b] > 0}
    assert looked_up == set(M.PLANTS), looked_up
    for b, t, c, what in p["planted"]:
        if c >= 0:
            assert 0 <= c < widths[t] and p["grad_y_bits"][b, cols[t] + c] == M.special(kind, what)
    # ---- the edges of every slice whose table has lookups: a looked-up +Inf in column 0 and in column W_t - 1
    for t in range(T):
        if per_bag[t].sum() == 0:
            continue
        edge = {c for b, tt, c, what in p["planted"] if tt == t and what == "+inf" and per_bag[t, b] > 0}
        assert edge & {0, widths[t] - 1}, (t, edge)                  # at least one edge of the slice, in any batch
        assert {0, widths[t] - 1} <= edge or np.count_nonzero(per_bag[t]) < 4, (t, edge)     # both, from four such bags on
    for weighted in (False, True):
        for mode in ("sum", "mean"):
            _, gy, sums = mixed_model(kind, batch, widths, layout, mode, weighted)
            finite = np.where(np.isfinite(gy), gy, 0).astype(np.float64)
            assert np.all(finite * 8 == np.round(finite * 8))
            bad = total = 0
            for t, s in enumerate(sums):
                assert M.every_order_is_exact(kind, s.scale, 0.125), (mode, weighted, t, float(s.scale.max()))
                hit = s.terms > 0
                bad += int(np.isnan(s.value[hit]).sum())          # (an infinity is compared by bits)
                total += int(s.value[hit].size)
                assert not np.signbit(s.value[s.value == 0]).any()
                # a plant stays inside its table's columns: a row of table t is non-finite only in columns whose plants
                # its own lookups reach
                reach = np.zeros((p["rows"][t], widths[t]), dtype=bool)
                _, sample, table = M.mixed_group_keys(batch, p)
                mine = table == t
                np.logical_or.at(reach, p["ids"][mine], ~np.isfinite(gy[sample[mine], cols[t]:cols[t + 1]]))
                assert not (~np.isfinite(s.value) & ~reach).any()
            assert 0 < bad / total <= NAN_CAP, (mode, weighted, bad / total)
            if mode == "mean":
                assert np.isnan(gy).any() and np.any((gy == 0) & np.signbit(gy))
