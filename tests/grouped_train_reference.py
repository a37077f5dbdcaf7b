"""A numpy model of what trains a group beyond sum pooling with table gradients (not a test module): the mean's scale
of grad_y, bit for bit, and the fp64 weight gradient of a group with the single-table kernel's bound.

Bag g = t * B + b belongs to table t and sample b; grad_y is [B, T, W]; lookups lie bag after bag (CSR offsets of
T * B + 1 entries, or H per bag).

    bag_lengths(T, B, offsets, hot)              [T * B] lookups per bag
    mean_factor(T, B, offsets, hot, weights)     [B, T] np.float32: 1 / length, or 1 / the fp32 sum of the bag's weights
                                                 IN LOOKUP ORDER; 0 where the denominator is 0
    mean_scale(kind, grad_y, factor)             round_to(kind, fp32(grad_y) * factor): one fp32 multiply, one rounding
    mean_factor64 / mean_scale_bound             the same in fp64, and what the design may be off by
    weight_grad64(tables64, rows, ...)           (exact, scale, table of lookup, sample of lookup) of a group

The weighted factor of the model sums in lookup order; the kernel may sum in another order, so bits are compared on
weights whose partial sums are exact (grouped_backward_cases.exact_weights) and arbitrary weights against the bound.
"""
import numpy as np

import exact_sums as X


def bag_lengths(num_tables, batch, offsets, hot):
    if offsets is None:
        return np.full(num_tables * batch, hot, dtype=np.int64)
    return np.diff(np.asarray(offsets).astype(np.int64))


def _bag_starts(lengths):
    return np.concatenate([[0], np.cumsum(lengths)])[:-1]


def mean_factor(num_tables, batch, offsets, hot, weights=None):
    """[B, T] float32.  weights: fp32 values ALREADY rounded to the tables' type."""
    lengths = bag_lengths(num_tables, batch, offsets, hot)
    if weights is None:
        denom = lengths.astype(np.float32)
    else:
        w = np.asarray(weights, dtype=np.float32)
        denom = np.zeros(lengths.size, dtype=np.float32)
        for g, (lo, n) in enumerate(zip(_bag_starts(lengths), lengths)):
            s = np.float32(0.0)
            for j in range(int(n)):
                s = np.float32(s + w[lo + j])
            denom[g] = s
    with np.errstate(divide="ignore"):
        f = np.where(denom == 0, np.float32(0.0), np.float32(1.0) / np.where(denom == 0, np.float32(1.0), denom))
    return f.astype(np.float32).reshape(num_tables, batch).T.copy()


def mean_scale(kind, grad_y, factor):
    """grad_y: fp32 values representable in `kind`, [B, T, W]; factor [B, T] float32.  Returns fp32 values of `kind`."""
    g = np.asarray(grad_y, dtype=np.float32)
    return X.round_to(kind, (g * np.asarray(factor, dtype=np.float32)[:, :, None]).astype(np.float32))


def mean_factor64(num_tables, batch, offsets, hot, weights=None):
    """[B, T] float64, exact up to fp64 rounding."""
    lengths = bag_lengths(num_tables, batch, offsets, hot)
    if weights is None:
        denom = lengths.astype(np.float64)
    else:
        w = np.asarray(weights, dtype=np.float64)
        denom = np.zeros(lengths.size)
        full = lengths > 0
        if full.any():
            denom[full] = np.add.reduceat(w[:int(lengths.sum())], _bag_starts(lengths)[full])   # (empty bags hold nothing)
    f = np.where(denom == 0, 0.0, 1.0 / np.where(denom == 0, 1.0, denom))
    return f.reshape(num_tables, batch).T.copy()


def mean_scale_bound(kind, exact, lengths_bt):
    """|design - exact| for out = round(kind, fp32(g) * fp32(1 / S)), S an fp32 sum of `len` positive fp32 terms in any
    order: the sum costs at most (len - 1) * 2^-24 relative, the reciprocal and the product 2^-24 each (first order:
    len + 1 in all, one more for the second-order terms), the final rounding EPS; one subnormal spacing as the floor."""
    n = np.asarray(lengths_bt, dtype=np.float64)[:, :, None]
    return X.EPS[kind] * np.abs(exact) + (n + 2.0) * 2.0 ** -24 * np.abs(exact) + X.SPACING[kind]


def lookup_bags(num_tables, batch, offsets, hot):
    """(table, sample) of every lookup."""
    lengths = bag_lengths(num_tables, batch, offsets, hot)
    bag = np.repeat(np.arange(num_tables * batch, dtype=np.int64), lengths)
    return bag // batch, bag % batch


def weight_grad64(tables64, batch, ids, offsets, hot, grad_y64):
    """The fp64 weight gradient of a group: (exact [nnz], scale [nnz]) -- exact_sums.weight_grad table by table, on the
    tables laid end to end and grad_y viewed as [B * T, W]."""
    T = len(tables64)
    t, b = lookup_bags(T, batch, offsets, hot)
    base = np.concatenate([[0], np.cumsum([x.shape[0] for x in tables64])]).astype(np.int64)
    flat = np.concatenate(tables64)
    gy = np.asarray(grad_y64, dtype=np.float64).reshape(batch * T, -1)
    return X.weight_grad(flat, base[t] + np.asarray(ids).astype(np.int64), gy, b * T + t)
