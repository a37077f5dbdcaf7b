"""The definitions of the index check (cuembed::CheckIndices) in plain numpy, and nothing else.

n = num_tables * batch bags, table-major: bag g = t * batch + b.  rows[t] >= 1 is table t's row count.

Offsets (CSR).  Position i in 0 .. n is BAD iff o[i] < 0, or o[i] > nnz, or i > 0 and o[i] < o[i - 1].  The REPAIRED
offsets are the running maximum clamped into [0, nnz]: r[i] = min(nnz, max(0, max_{k <= i} o[k])).

Indices.  The checked range is [r[0], r[n]) for CSR and [0, nnz) for fixed hotness (nnz = n * num_hots).  Position p belongs
to the table t with r[t * batch] <= p < r[(t + 1) * batch] (CSR) or to t = p // (batch * num_hots).  p is BAD iff indices[p]
< 0 or indices[p] >= rows[t]; the repaired index is 0 where bad, unchanged elsewhere and outside the checked range.

Report: [bad indices, first (smallest) bad index position or -1, bad offsets, first bad offset position or -1].
"""
import numpy as np


def offsets_valid(offsets, nnz):
    o = np.asarray(offsets, dtype=np.int64)
    return bool(o[0] >= 0 and o[-1] <= nnz and np.all(o[1:] >= o[:-1]))


def bad_offsets(offsets, nnz):
    """Boolean [n + 1]: the local violations."""
    o = np.asarray(offsets, dtype=np.int64)
    bad = (o < 0) | (o > nnz)
    bad[1:] |= o[1:] < o[:-1]
    return bad


def repair_offsets(offsets, nnz):
    """int64 [n + 1]: the running maximum clamped into [0, nnz]."""
    o = np.asarray(offsets, dtype=np.int64)
    return np.minimum(nnz, np.maximum(0, np.maximum.accumulate(o)))


def table_of_positions(nnz, rows, batch, num_hots=0, repaired_offsets=None):
    """(table [nnz] int64, checked [nnz] bool) of every position."""
    T = len(rows)
    p = np.arange(nnz, dtype=np.int64)
    if repaired_offsets is None:
        return p // max(batch * num_hots, 1), np.ones(nnz, dtype=bool)
    cuts = repaired_offsets[::batch] if batch > 0 else np.repeat(repaired_offsets[:1], T + 1)
    assert cuts.shape[0] == T + 1
    table = np.clip(np.searchsorted(cuts[1:], p, side="right"), 0, T - 1)
    return table, (p >= cuts[0]) & (p < cuts[T])


def check(indices, offsets, rows, batch, num_hots=0):
    """-> (report int64[4], repaired indices (dtype kept), repaired offsets (dtype kept) or None)."""
    idx = np.asarray(indices).reshape(-1)
    nnz = idx.shape[0]
    rows = np.asarray(rows, dtype=np.int64)
    assert np.all(rows >= 1)
    report = np.array([0, -1, 0, -1], dtype=np.int64)
    repaired = None
    if offsets is not None:
        assert num_hots == 0 and len(offsets) == len(rows) * batch + 1
        bad_o = bad_offsets(offsets, nnz)
        repaired = repair_offsets(offsets, nnz)
        if bad_o.any():
            report[2], report[3] = bad_o.sum(), np.flatnonzero(bad_o)[0]
    else:
        assert num_hots > 0 and nnz == len(rows) * batch * num_hots
    table, checked = table_of_positions(nnz, rows, batch, num_hots, repaired)
    wide = idx.astype(np.int64)
    bad_i = checked & ((wide < 0) | (wide >= rows[table])) if nnz else np.zeros(0, dtype=bool)
    if bad_i.any():
        report[0], report[1] = bad_i.sum(), np.flatnonzero(bad_i)[0]
    fixed = np.where(bad_i, 0, idx).astype(idx.dtype).reshape(np.asarray(indices).shape)
    return report, fixed, None if repaired is None else repaired.astype(np.asarray(offsets).dtype)
