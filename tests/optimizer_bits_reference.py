"""Bit-level numpy model of the sparse optimizer step (not a test module): the five rules of cuembed_amd.sparse_row_update /
sparse_row_adam as the documents state them -- fp32 arithmetic, one unfused IEEE operation per step, a fixed summation
order for the row-wise rules, one rounding to the table's type at the store.  Every line of arithmetic below is ONE
np.float32 operation (numpy's float32 +, *, / and sqrt are correctly rounded and keep subnormals), so the model shares
nothing with the kernels but the statement of the contract.

    scalars   lr, eps, the bias factor c, beta1, beta2, weight_decay: each rounded once to fp32; 1 - beta formed in
              double, then rounded; step = lr * c and decay = lr * weight_decay: one fp32 product each
    sgd               x = w + -(lr * g)
    adagrad           s' = s + g * g;  d = (lr * g) / (sqrt(s') + eps);  x = w + -d
    rowwise_adagrad   s_r' = s_r + sum / float32(W);  t = lr / (sqrt(s_r') + eps);  x = w + -(t * g)
    adam, rowwise_adam    wd = w + -(decay * w) if weight_decay != 0 else w;  m' = beta1 * m + omb1 * g
    adam              v' = beta2 * v + omb2 * (g * g);  d = (step * m') / (sqrt(v') + eps);  x = wd + -d
    rowwise_adam      v_r' = beta2 * v_r + omb2 * (sum / float32(W));  sc = step / (sqrt(v_r') + eps);  x = wd + -(sc * m')
    sum       the row's squared gradient in the kernel's order (row_sums): a lane holds N = lane bytes / element size
              elements per slice, slice c belongs to lane c % group, a lane adds its slices in ascending c and their
              elements in order (acc = acc + x * x from 0), then a butterfly L[i] = L[i] + L[i ^ d], d = group / 2 .. 1
    store     fp32: as is; 16-bit: to nearest even, or stochastic_rounding_reference.stochastic with the fields of
              (seed, step, table row, column)

Tables and state travel as BIT PATTERNS (uint16 / uint32 arrays); only the valid entries are applied, everything else
is returned untouched.  `step` also returns every intermediate of the valid rows, for finding the operation at which a
device differs.  Two deliberately wrong variants exist for the tests that show what the fingerprints tell apart:
row_sum="sequential" (one accumulator over the row) and fused=True (s' or m' formed with a fused multiply-add, emulated
by computing in float64 and rounding once).
"""
import numpy as np

import stochastic_rounding_reference as S

F = np.float32
RULES = ("sgd", "adagrad", "rowwise_adagrad", "adam", "rowwise_adam")
ELEM_SIZE = {"f32": 4, "f16": 2, "bf16": 2}
BITS = {"f32": np.uint32, "f16": np.uint16, "bf16": np.uint16}
S_KIND = {"f16": "fp16", "bf16": "bf16"}          # stochastic_rounding_reference's names
#: the state tensors of a rule: "e" = fp32 per element [rows, W], "r" = fp32 per row [rows]
STATE = {"sgd": "", "adagrad": "e", "rowwise_adagrad": "r", "adam": "ee", "rowwise_adam": "er"}


def lane_bytes(kind, width, *pointers):
    """Bytes of a row a lane moves: the widest of 16 / 8 / 4 that divides the row size and every base pointer (given as
    addresses or residues; state tensors are taken to be 16-byte aligned)."""
    bits = ELEM_SIZE[kind] * width
    for p in pointers:
        bits |= int(p)
    return 16 if bits % 16 == 0 else (8 if bits % 8 == 0 else 4)


def group_of(lanes_per_row):
    """Lanes per entry: the smallest power of two >= lanes_per_row, at most 64."""
    group = 1
    while group < lanes_per_row and group < 64:
        group *= 2
    return group


def widen(bits, kind):
    """Bit patterns of the table's type -> their exact fp32 values."""
    bits = np.asarray(bits, dtype=BITS[kind])
    return bits.view(np.float32) if kind == "f32" else S.to_f32(bits, S_KIND[kind])


def f32(bits):
    return np.asarray(bits, dtype=np.uint32).view(np.float32)


def u32(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def store(x, kind, rounding="nearest", seed=0, step=0, rows=None):
    """The one rounding to the table's type: fp32 values [n, W] -> bit patterns.  rows: the table rows of x's rows (the
    stochastic fields depend on them)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if kind == "f32":
        assert rounding == "nearest"
        return x.view(np.uint32).copy()
    if rounding == "nearest":
        return S.nearest(x, S_KIND[kind]).astype(np.uint16)
    assert rounding == "stochastic"
    return S.stochastic(x, S.fields(seed, step, rows, x.shape[1]), S_KIND[kind]).astype(np.uint16)


def row_sums(g, per_lane, order="butterfly"):
    """sum_j g[:, j]^2 of every row of g (float32 [n, W]) in the kernel's order, with per_lane = N elements per slice."""
    g = np.asarray(g, dtype=np.float32)
    n, width = g.shape
    with np.errstate(all="ignore"):
        if order == "sequential":
            acc = np.zeros(n, dtype=np.float32)
            for j in range(width):
                acc = acc + g[:, j] * g[:, j]
            return acc
        assert order == "butterfly" and width % per_lane == 0
        lanes_per_row = width // per_lane
        group = group_of(lanes_per_row)
        lane = np.arange(group)
        acc = np.zeros((n, group), dtype=np.float32)
        for first in range(0, lanes_per_row, group):              # the slices first .. first + group - 1: one per lane
            has = first + lane < lanes_per_row
            at = np.minimum(first + lane, lanes_per_row - 1) * per_lane
            for e in range(per_lane):
                x = g[:, at + e]
                acc = np.where(has, acc + x * x, acc)
        d = group // 2
        while d > 0:
            acc = acc + acc[:, lane ^ d]
            d //= 2
        assert np.array_equal(acc.view(np.uint32), np.repeat(acc[:, :1], group, axis=1).view(np.uint32)) or \
            np.isnan(acc).any()                                   # every lane ends with the same bits
        return acc[:, 0].copy()


def scalars(lr, eps=1e-8, bias_factor=1.0, betas=(0.9, 0.999), weight_decay=0.0):
    beta1, beta2 = float(betas[0]), float(betas[1])
    lr32, c32, wd32 = F(lr), F(bias_factor), F(weight_decay)
    return dict(lr=lr32, eps=F(eps), beta1=F(beta1), omb1=F(1.0 - beta1), beta2=F(beta2), omb2=F(1.0 - beta2),
                step=lr32 * c32, decay=lr32 * wd32, decays=bool(wd32 != 0))


def _fma(a, b, c):
    """round(a * b + c) for float32 operands: the product is exact in float64."""
    return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)) \
        .astype(np.float32)


def valid_entries(n, count=None, counts=None, piece_rows=None):
    """The indices of the entries a step applies: the first `count` of n, or, with counts= and piece_rows=, the first
    counts[p] of every piece p (a count below zero or above piece_rows: none)."""
    if counts is None:
        return np.arange(n if count is None else int(count), dtype=np.int64)
    out = [np.arange(c, dtype=np.int64) + p * piece_rows for p, c in enumerate(counts) if 0 <= c <= piece_rows]
    return np.concatenate(out) if out else np.zeros(0, dtype=np.int64)


def step(rule, kind, table, state, ids, grads, valid, *, lr, eps=1e-8, bias_factor=1.0, betas=(0.9, 0.999),
         weight_decay=0.0, lane=None, rounding="nearest", seed=0, step=0, row_sum="butterfly", fused=False):
    """One step.  table: patterns [rows, W] of `kind`; state: the rule's tensors (STATE) as uint32 patterns; ids: int64
    [entries]; grads: patterns [entries, W]; valid: the indices of the entries to apply (distinct rows); lane: bytes per
    lane (default: what aligned buffers get).  Returns (table, state, trace): new arrays, the inputs stay as they are;
    trace maps the name of every intermediate of the valid rows to its float32 array, "x" being the value before the
    store and "rows" the table rows."""
    table = np.array(table, dtype=BITS[kind], copy=True)
    state = [np.array(s, dtype=np.uint32, copy=True) for s in state]
    assert len(state) == len(STATE[rule])
    width = table.shape[1]
    valid = np.asarray(valid, dtype=np.int64)
    rows = np.asarray(ids, dtype=np.int64)[valid]
    assert np.unique(rows).size == rows.size, "the valid entries must name distinct rows"
    per_lane = (lane_bytes(kind, width) if lane is None else lane) // ELEM_SIZE[kind]
    h = scalars(lr, eps, bias_factor, betas, weight_decay)
    g = widen(np.asarray(grads)[valid], kind)
    w = widen(table[rows], kind)
    t = dict(rows=rows, g=g, w=w)
    with np.errstate(all="ignore"):
        if rule in ("rowwise_adagrad", "rowwise_adam"):
            t["sum"] = row_sums(g, per_lane, row_sum)
            t["mean"] = t["sum"] / F(width)
        if rule == "sgd":
            t["lr_g"] = h["lr"] * g
            t["x"] = w + -t["lr_g"]
        elif rule == "adagrad":
            s = f32(state[0][rows])
            t["s"] = _fma(g, g, s) if fused else s + g * g
            t["lr_g"] = h["lr"] * g
            t["denom"] = np.sqrt(t["s"]) + h["eps"]
            t["d"] = t["lr_g"] / t["denom"]
            t["x"] = w + -t["d"]
            state[0][rows] = u32(t["s"])
        elif rule == "rowwise_adagrad":
            t["s"] = f32(state[0][rows]) + t["mean"]
            t["denom"] = np.sqrt(t["s"]) + h["eps"]
            t["scale"] = h["lr"] / t["denom"]
            t["x"] = w + -(t["scale"][:, None] * g)
            state[0][rows] = u32(t["s"])
        else:
            t["wd"] = w + -(h["decay"] * w) if h["decays"] else w
            m = f32(state[0][rows])
            t["m"] = _fma(h["omb1"], g, h["beta1"] * m) if fused else h["beta1"] * m + h["omb1"] * g
            state[0][rows] = u32(t["m"])
            v = f32(state[1][rows])
            if rule == "adam":
                t["v"] = h["beta2"] * v + h["omb2"] * (g * g)
                t["denom"] = np.sqrt(t["v"]) + h["eps"]
                t["d"] = (h["step"] * t["m"]) / t["denom"]
                t["x"] = t["wd"] + -t["d"]
            else:
                t["v"] = h["beta2"] * v + h["omb2"] * t["mean"]
                t["denom"] = np.sqrt(t["v"]) + h["eps"]
                t["scale"] = h["step"] / t["denom"]
                t["x"] = t["wd"] + -(t["scale"][:, None] * t["m"])
            state[1][rows] = u32(t["v"])
        table[rows] = store(t["x"], kind, rounding, seed, step, rows)
    return table, state, t
