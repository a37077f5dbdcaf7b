"""numpy reference of stochastic rounding in the sparse optimizer step (not a test module).

    philox4x32_10(counter, key)            Philox4x32-10 on arrays of counters / keys
    fields(seed, step, rows, width)        the 16-bit random field of every (table row, column): uint32 [len(rows), width]
    round_fp16(x, r) / round_bf16(x, r)    the two rounding rules, written as the specification words them (value
                                           arithmetic in fp64 for fp16, the integer add for bf16) -> uint16 patterns
    sgd(...)                               w + -(lr * g) in fp32, one unfused operation each, then the stochastic rounding
    walk(kind)                             512 steps of an update of 1/64 of a spacing on a table of 1.0 (computed once)

16-bit values travel as uint16 bit patterns; to_f32 / nearest turn them into fp32 values and back (round to nearest even).
"""
import functools

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or ints), key: two.  Returns the four output words as uint64 arrays below 2**32."""
    c = [np.asarray(v, dtype=np.uint64) & np.uint64(MASK) for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = (np.asarray(v, dtype=np.uint64) & np.uint64(MASK) for v in key)
    mask = np.uint64(MASK)
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]        # < 2**64: both factors are below 2**32
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & mask, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & mask]
        k0 = (k0 + np.uint64(W0)) & mask
        k1 = (k1 + np.uint64(W1)) & mask
    return c


def words(seed, step, rows, groups):
    """The call of (seed, step, table row, column group): counter = (row lo, row hi, group, step lo), key = (seed lo,
    seed hi ^ step hi).  rows / groups broadcast; returns uint64 [4, ...]."""
    seed, step = int(seed), int(step)
    rows = np.asarray(rows, dtype=np.int64).astype(np.uint64)
    groups = np.asarray(groups, dtype=np.uint64)
    out = philox4x32_10((rows & np.uint64(MASK), rows >> np.uint64(32), groups, step & MASK),
                        (seed & MASK, (seed >> 32) ^ (step >> 32)))
    return np.stack(out)


def fields(seed, step, rows, width):
    """uint32 [len(rows), width]: column c takes half (c % 8) % 2 (low half first) of word (c % 8) // 2 of the call of
    column group c // 8."""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 1)
    col = np.arange(width, dtype=np.int64).reshape(1, -1)
    w = words(seed, step, rows, col // 8)                       # [4, rows, width]
    j = np.broadcast_to(col % 8, w.shape[1:])
    word = np.take_along_axis(w, (j // 2)[None], axis=0)[0]
    return ((word >> ((j % 2) * 16).astype(np.uint64)) & np.uint64(0xFFFF)).astype(np.uint32)


# ---- 16-bit patterns <-> fp32 -----------------------------------------------------------------------------------------
def to_f32(bits, kind):
    bits = np.asarray(bits, dtype=np.uint16)
    if kind == "fp16":
        return bits.view(np.float16).astype(np.float32)
    return (bits.astype(np.uint32) << np.uint32(16)).view(np.float32)


def nearest(x, kind):
    """fp32 -> 16-bit pattern, round to nearest even (what the table's type conversion does)."""
    x = np.asarray(x, dtype=np.float32)
    if kind == "fp16":
        with np.errstate(over="ignore"):
            return x.astype(np.float16).view(np.uint16)
    b = x.view(np.uint32).astype(np.uint64)
    r = ((b + np.uint64(0x7FFF) + ((b >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)).astype(np.uint16)
    nan = np.isnan(x)
    return np.where(nan, ((b >> np.uint64(16)) | np.uint64(0x40)).astype(np.uint16), r)


# ---- the rules ----------------------------------------------------------------------------------------------------------
def round_fp16(x, r):
    """q = fp16's spacing at |x| (2^(e-10) for |x| >= 2^-14, e = floor(log2 |x|); else 2^-24); m = |x| / q; i = floor(m);
    t = floor((m - i) * 2^13); away from zero iff t + (r & 0x1FFF) >= 2^13; +-(i + up) * q.  (fp64 holds every step
    exactly: m < 2^35 has at most 24 significant bits.)"""
    x = np.asarray(x, dtype=np.float32)
    r = np.asarray(r, dtype=np.int64)
    x, r = np.broadcast_arrays(x, r)
    finite = np.isfinite(x)
    a = np.abs(np.where(finite, x, np.float32(0))).astype(np.float64)
    _, ex = np.frexp(a)                                          # a = f * 2^ex, f in [0.5, 1): floor(log2 a) = ex - 1
    q = np.where(a >= 2.0 ** -14, np.ldexp(1.0, ex - 1 - 10), 2.0 ** -24)
    m = a / q
    i = np.floor(m)
    t = np.floor((m - i) * 8192.0).astype(np.int64)
    up = (t + (r & 0x1FFF)) >= 8192
    with np.errstate(over="ignore"):
        mag = ((i + up) * q).astype(np.float16)                  # representable, or past 65504 -> inf
    bits = mag.view(np.uint16) | (np.signbit(x).astype(np.uint16) << np.uint16(15))
    with np.errstate(over="ignore", invalid="ignore"):
        return np.where(finite, bits, x.astype(np.float16).view(np.uint16)).astype(np.uint16)


def round_bf16(x, r):
    """r (16 bits) is added to the low 16 bits of the fp32 pattern, which are then dropped; inf / NaN convert as usual."""
    x = np.asarray(x, dtype=np.float32)
    r = np.asarray(r, dtype=np.uint64)
    x, r = np.broadcast_arrays(x, r)
    b = x.view(np.uint32).astype(np.uint64)
    out = ((b + (r & np.uint64(0xFFFF))) >> np.uint64(16)).astype(np.uint16)
    return np.where(np.isfinite(x), out, nearest(x, "bf16")).astype(np.uint16)


def stochastic(x, r, kind):
    return round_fp16(x, r) if kind == "fp16" else round_bf16(x, r)


# ---- SGD ------------------------------------------------------------------------------------------------------------------
def sgd_value(w_bits, g_bits, lr, kind):
    """The fp32 value SGD stores: w + -(lr * g), one unfused fp32 operation each."""
    w = to_f32(w_bits, kind)
    g = to_f32(g_bits, kind)
    return (w + -(np.float32(lr) * g)).astype(np.float32)


def sgd(table_bits, ids, grad_bits, lr, kind, seed=None, step=0):
    """table[ids[k]] <- round(table[ids[k]] - lr * grad[k]) on uint16 patterns, in place on a copy: stochastic with the
    fields of (seed, step) or, seed=None, to nearest.  ids must be distinct."""
    out = np.array(table_bits, dtype=np.uint16, copy=True)
    ids = np.asarray(ids, dtype=np.int64)
    x = sgd_value(out[ids], grad_bits, lr, kind)
    if seed is None:
        out[ids] = nearest(x, kind)
    else:
        out[ids] = stochastic(x, fields(seed, step, ids, out.shape[1]), kind)
    return out


# ---- the symptom and the cure ---------------------------------------------------------------------------------------------
WALK_SEED, WALK_STEPS, WALK_ROWS, WALK_WIDTH = 0x1234567, 512, 64, 256
WALK_LR = {"fp16": 2.0 ** -17, "bf16": 2.0 ** -14}          # 1/64 of the spacing below 1.0


@functools.lru_cache(maxsize=None)
def walk(kind):
    """512 SGD steps (step = 0..511, seed WALK_SEED) of g = 1 on a 64 x 256 table of 1.0 with lr = WALK_LR[kind].
    Returns (table after stochastic rounding, moves per element, table after round-to-nearest); read-only arrays."""
    one = int(nearest(np.float32(1.0), kind))
    table = np.full((WALK_ROWS, WALK_WIDTH), one, dtype=np.uint16)
    plain = table.copy()
    grad = table.copy()
    ids = np.arange(WALK_ROWS)
    moves = np.zeros((WALK_ROWS, WALK_WIDTH), dtype=np.int64)
    for step in range(WALK_STEPS):
        new = sgd(table, ids, grad, WALK_LR[kind], kind, seed=WALK_SEED, step=step)
        moves += new != table
        table = new
        plain = sgd(plain, ids, grad, WALK_LR[kind], kind)
    for a in (table, moves, plain):
        a.setflags(write=False)
    return table, moves, plain
