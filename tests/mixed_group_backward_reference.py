"""A numpy model of the mixed-width group's padded gradient, and the data helpers of its tests (no GPU).

The group: T tables [rows_t, W_t], bag g = t * B + b, grad_y [B, D], D = sum W_t, table t at columns [c_t, c_t + W_t).
The gradient: ascending global row ids (row_base[t] + row), one entry per looked-up row, padded to W_max = max W_t;
entry k holds its row's sum in columns [0, W_t) of the table t its id falls in.  Columns >= W_t are unspecified, so the
model returns a mask of the valid ones and every comparison goes through it.
"""
import numpy as np

import grouped_backward_cases as G

ROWS = (5000, 17, 300, 64)
#: the widths of the GPU tests, with the lane bytes a 16-bit element type gives them on aligned buffers
GROUPS = {(128, 16, 64, 32): 16, (36, 4, 128): 8, (6, 2, 10): 4, (36, 36, 36): 8, (128,): 16}

# tests/test_gpu_backward_tolerance.py, bound (3): the same constants
EPS = {"f16": 2.0 ** -11, "bf16": 2.0 ** -8}
TINY = 2.0 ** -23


def column_base(widths):
    return np.concatenate([[0], np.cumsum(widths)]).astype(np.int64)


def row_base(rows):
    return np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)


def exact_grad_y(rng, batch, widths, kind):
    """grouped_backward_cases.exact_grad_y per table slice, laid side by side: [B, D] fp32 of small integers."""
    return np.concatenate([G.exact_grad_y(rng, batch, 1, w, kind)[:, 0, :] for w in widths], axis=1)


def fp64_sums(widths, rows, batch, ids, offsets, hot, weights, grad_y):
    """grouped_backward_cases.fp64_sums table by table on the table's own columns: (exact, scale, walk) as
    [total_rows, W_max] fp64 (zero in the padding), run_len [total_rows], valid [total_rows, W_max] bool."""
    T, w_max = len(widths), max(widths)
    base, cols = row_base(rows), column_base(widths)
    total = int(base[-1])
    keys, sids = G.global_problem(rows, batch, ids, offsets, hot)
    table = sids % T
    exact, scale, walk = (np.zeros((total, w_max)) for _ in range(3))
    valid = np.zeros((total, w_max), dtype=bool)
    for t, w in enumerate(widths):
        valid[base[t]:base[t + 1], :w] = True
        mine = table == t
        if not mine.any():
            continue
        grad_t = np.ascontiguousarray(grad_y[:, cols[t]:cols[t + 1]], dtype=np.float64)
        e, s, k, _ = G.fp64_sums(keys[mine], sids[mine] // T, grad_t, None if weights is None else weights[mine], total)
        exact[:, :w] += e
        scale[:, :w] += s
        walk[:, :w] += k       # (disjoint rows per table: a sum of one non-zero term)
    return exact, scale, walk, np.bincount(keys, minlength=total), valid


def padded_gradient(widths, rows, batch, ids, offsets, hot, weights, grad_y):
    """The model: (ids int64 [count] ascending global rows, count, rows fp64 [count, W_max], valid bool [count, W_max])."""
    exact, _, _, run_len, valid = fp64_sums(widths, rows, batch, ids, offsets, hot, weights, grad_y)
    looked_up = np.flatnonzero(run_len)
    return looked_up.astype(np.int64), int(looked_up.size), exact[looked_up], valid[looked_up]


def hip_error_bound(kind, exact, scale, walk, run_len, lookups_per_block):
    """tests/test_gpu_backward_tolerance.py::_hip_error_bound, with its `run_len // 256` -- a workgroup there covers at
    least 256 lookups -- replaced by run_len // the lookups a workgroup of THIS launch covers
    (mixed_group_backward_launch_shape(...)["lookups_per_block"]): a run that crosses workgroups is combined by one
    16-bit atomic per workgroup it touches."""
    flushes = 2 + run_len // lookups_per_block
    return (EPS[kind] * (np.abs(exact) + 4.0 * (np.sqrt(flushes)[:, None] + 1.0) * walk)
            + 1e-5 * scale + TINY)
