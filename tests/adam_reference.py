"""fp64 reference of the sparse Adam rules and the error bounds of the HIP kernel (not a test module).

`step` applies one rule to the STORED values (table rows, gradient rows and moments widened exactly to fp64) of the
named rows and returns the exact new weights and moments with the magnitudes the bounds are made of.  The scalars are
the fp32 values the kernel is given, widened: `scalars(lr, bias_factor, betas, eps, weight_decay)` rounds lr, c, beta,
1 - beta (formed in double), eps and weight_decay each once to fp32, and forms lr * c and lr * weight_decay as the
kernel does, with one fp32 multiplication each.

    decay = (lr * weight_decay) * w        (0 if weight_decay == 0)
    m'    = beta1 * m + (1 - beta1) * g
    adam:          v'   = beta2 * v + (1 - beta2) * g^2                 w' = w - decay - (lr * c) * m' / (sqrt(v') + eps)
    rowwise_adam:  v_r' = beta2 * v_r + (1 - beta2) * mean_j(g_j^2)     w' = w - decay - (lr * c) * m' / (sqrt(v_r') + eps)

The kernel computes in fp32, one rounded operation per step, and rounds once to the table's type T at the store.  m'
can cancel (beta1 * m against (1 - beta1) * g), so nothing is bounded relative to m' or to the update term itself:
with u = 2^-24, T_m = |beta1 * m| + |(1 - beta1) * g| and D = lr * c * T_m / (sqrt(v') + eps),

    moments:  |got - m'| <= K * u * T_m + 2^-149
              |got - v'| <= K * u * |v'| + 2^-149
    weights:  |got - w'| <= EPS[T] * |w'| + SPACING[T] + K * u * (|w| + |decay| + D)

Counting the rounded operations (each costs at most u relative to its result, to first order):
  m':  two products and their sum: at most 2 u * T_m.
  v':  g * g, (1 - beta2) * (.), beta2 * v and the sum, all terms positive: at most 3 u * v'.  Row-wise: the row's sum
       is at most 8 squares (1 each) added one after the other in a lane (7 additions), a butterfly of log2(64) = 6
       levels, the division by W, then (1 - beta2) * (.), beta2 * v_r and the sum: at most 18 u * v_r' in the worst
       case.
  update term: sqrt halves the relative error of v' and adds its own rounding, + eps is one more (adam: 3.5 u,
       row-wise: 11 u on the denominator); lr * c, the product with m' and the division are 3 more, and the error of
       m' enters as 2 u * T_m * lr * c / denominator <= 2 u * D: at most 8.5 u * D (adam) and 16 u * D (row-wise,
       where the kernel divides lr * c by the denominator once per row and multiplies by m').
  decay: lr * weight_decay and its product with w are 2 u * |decay|; the two subtractions cost u * (|w| + |decay|) and
       u * (|w| + |decay| + D).
K = 16 therefore covers both rules for rows of up to 256 elements (the row-wise worst case needs every one of 18
roundings to fall the same way; on an MI355X the worst error / bound over tests/test_gpu_sparse_adam.py was 0.24 for
fp32 weights, 0.12 for exp_avg and 0.21 for exp_avg_sq -- 16-bit weights reach 0.997, which is the rounding to the
table's type itself).  Wider rows put several slices into a lane's
sequential sum: K = 8 + ceil(log2 W) as for the Adagrad rules (tests/optimizer_reference.py), never below 16.
"""
import math

import numpy as np

from exact_sums import EPS, SPACING

RULES = ("adam", "rowwise_adam")
U = 2.0 ** -24


def k_for(width):
    return 16 if width <= 256 else max(16, 8 + int(math.ceil(math.log2(width))))


def scalars(lr, bias_factor=1.0, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
    """The fp32 values the kernel works with, as Python floats (exact widenings)."""
    f = np.float32
    beta1, beta2 = float(betas[0]), float(betas[1])
    lr32, c32, wd32 = f(lr), f(bias_factor), f(weight_decay)
    return dict(beta1=float(f(beta1)), omb1=float(f(1.0 - beta1)), beta2=float(f(beta2)), omb2=float(f(1.0 - beta2)),
                eps=float(f(eps)), step=float(f(lr32 * c32)), decay=float(f(lr32 * wd32)) if wd32 != 0 else 0.0,
                lr=float(lr32), c=float(c32), weight_decay=float(wd32))


def bias_factor(step, betas=(0.9, 0.999)):
    """sqrt(1 - beta2^t) / (1 - beta1^t) in double."""
    return math.sqrt(1.0 - betas[1] ** step) / (1.0 - betas[0] ** step)


def step(rule, w, g, m, v, sc):
    """One step on the named rows only.  w, g, m: float64 [n, W] (the stored values, widened); v: float64 [n, W] (adam)
    or float64 [n] (rowwise_adam); sc: scalars(...).  Returns a dict of float64 arrays: w, m, v (the exact new values),
    m_terms = |beta1 m| + |(1 - beta1) g|, decay = |decay term|, reach = lr * c * m_terms / (sqrt(v') + eps)."""
    w = np.asarray(w, dtype=np.float64)
    g = np.asarray(g, dtype=np.float64)
    m = np.asarray(m, dtype=np.float64)
    v = np.asarray(v, dtype=np.float64)
    decay = sc["decay"] * w
    m_new = sc["beta1"] * m + sc["omb1"] * g
    m_terms = np.abs(sc["beta1"] * m) + np.abs(sc["omb1"] * g)
    if rule == "adam":
        v_new = sc["beta2"] * v + sc["omb2"] * (g * g)
        denom = np.sqrt(v_new) + sc["eps"]
    elif rule == "rowwise_adam":
        v_new = sc["beta2"] * v + sc["omb2"] * ((g * g).sum(axis=1) / g.shape[1])
        denom = (np.sqrt(v_new) + sc["eps"])[:, None]
    else:
        raise ValueError(rule)
    with np.errstate(divide="ignore", invalid="ignore"):
        w_new = w - decay - sc["step"] * m_new / denom
        reach = sc["step"] * m_terms / denom
    return dict(w=w_new, m=m_new, v=v_new, m_terms=m_terms, decay=np.abs(decay), reach=reach)


def weight_bound(kind, r, w, k=16):
    """r: step's result; w: the weights before, float64."""
    return EPS[kind] * np.abs(r["w"]) + SPACING[kind] + k * U * (np.abs(w) + r["decay"] + r["reach"])


def exp_avg_bound(r, k=16):
    return k * U * r["m_terms"] + 2.0 ** -149


def exp_avg_sq_bound(r, k=16):
    return k * U * np.abs(r["v"]) + 2.0 ** -149


def worst_ratio(got, exact, bound):
    """max over EVERY element of |got - exact| / bound (0 for an empty array); non-finite values count as inf."""
    got = np.asarray(got, dtype=np.float64)
    if got.size == 0:
        return 0.0
    err = np.abs(got - exact)
    err = np.where(np.isfinite(err), err, np.inf)
    return float(np.max(err / bound))
