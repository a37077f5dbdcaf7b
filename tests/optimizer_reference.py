"""fp64 reference of the sparse optimizer rules and the error bounds of the HIP kernel (not a test module).

`step` applies one rule to the STORED values (table rows, gradient rows and state widened exactly to fp64) and returns,
per element, the exact new weight w', the update term d (w' = w - d) and the exact new state s'.  lr and eps are the
fp32 values the kernel is given, widened.

The kernel computes in fp32 and rounds once to the table's type T at the store, so

    weights:  |got - w'| <= EPS[T] * |w'| + SPACING[T] + K * 2^-24 * (|w| + |d|)
    state:    |got - s'| <= K * 2^-24 * |s'| + 2^-149

The first weight term is the one rounding to T (SPACING: a subnormal result); the last is the fp32 arithmetic: at most
six rounded operations for the update term (square, state add, sqrt, + eps, lr * g, divide; the subtraction is the
seventh and is covered by |w| + |d|), and for the row-wise sum at most 7 sequential additions per lane (8 elements of
16 bytes), a tree of log2(lanes) <= 6 levels and the scaling by 1 / W.  K = 16 covers that for rows of up to 256
elements; wider rows (several slices per lane) use K = 8 + ceil(log2 W).
"""
import math

import numpy as np

from exact_sums import EPS, SPACING

RULES = ("sgd", "adagrad", "rowwise_adagrad")


def k_for(width):
    return 16 if width <= 256 else max(16, 8 + int(math.ceil(math.log2(width))))


def step(rule, w, g, s, lr, eps=1e-8):
    """One step on the named rows only.  w, g: float64 [n, W] (the stored values, widened); s: None (sgd),
    float64 [n, W] (adagrad) or float64 [n] (rowwise_adagrad).  Returns (w_new, d, s_new) in float64."""
    w = np.asarray(w, dtype=np.float64)
    g = np.asarray(g, dtype=np.float64)
    lr = float(np.float32(lr))
    eps = float(np.float32(eps))
    if rule == "sgd":
        d = lr * g
        return w - d, d, None
    s = np.asarray(s, dtype=np.float64)
    if rule == "adagrad":
        s_new = s + g * g
        d = lr * g / (np.sqrt(s_new) + eps)
        return w - d, d, s_new
    if rule == "rowwise_adagrad":
        s_new = s + (g * g).sum(axis=1) / g.shape[1]
        d = lr * g / (np.sqrt(s_new)[:, None] + eps)
        return w - d, d, s_new
    raise ValueError(rule)


def weight_bound(kind, w_new, w, d, k=16):
    return EPS[kind] * np.abs(w_new) + SPACING[kind] + k * 2.0 ** -24 * (np.abs(w) + np.abs(d))


def state_bound(s_new, k=16):
    return k * 2.0 ** -24 * np.abs(s_new) + 2.0 ** -149


def worst_ratio(got, exact, bound):
    """max over EVERY element of |got - exact| / bound (0 for an empty array); non-finite values count as inf."""
    got = np.asarray(got, dtype=np.float64)
    if got.size == 0:
        return 0.0
    err = np.abs(got - exact)
    err = np.where(np.isfinite(err), err, np.inf)
    return float(np.max(err / bound))
