"""fp64 references and error bounds for the paths that are NOT bit-identical to the reference (not a test module).

The library keeps fp32 partial sums where the reference rounds to the gradient's type at every lookup: a run of an
index-sorted COO is summed in fp32 inside one workgroup and rounded once; a run that crosses workgroup boundaries is
combined by one 16-bit (or fp32) hardware atomic per workgroup piece.  The weight gradient is an fp32 dot product
rounded once, the split forward an fp32 pool of per-wave partial rows rounded once.

Every reference here is exact in fp64 and comes with, per output element,
  scale   = sum |term|
  walk    = sqrt(sum term^2)      (the size of a partial sum of random-signed terms)
  flushes = how many times the design rounds that element to the output type
and `error_bound` turns those into what the design may be off by:

  EPS * (|exact| + c * sqrt(flushes - 1) * (walk + |exact|)) + small * scale + floor(flushes)

EPS is the output type's unit roundoff.  The final rounding costs EPS * |exact|; every further rounding is that of a
partial sum or of an intermediate atomic result, whose size is that of a random walk over the terms (`walk`, times c
for its excursions) plus its drift (at most |exact| when the terms have one sign), and independent roundings add up
like sqrt(count).  A run that is rounded ONCE (it lies inside
one workgroup) therefore has no walk term at all: it must be the correctly rounded fp32 sum.  `small * scale` is what
the fp32 accumulation itself may cost.  The floor is of the order of the output type's subnormal spacing (one spacing
for a single rounding, plus half a spacing per further rounding, combined like the walk): a result whose subnormal
inputs or partials were flushed to zero is far outside it.
"""
import numpy as np

EPS = {"f32": 2.0 ** -24, "f16": 2.0 ** -11, "bf16": 2.0 ** -8}
SPACING = {"f32": 2.0 ** -149, "f16": 2.0 ** -24, "bf16": 2.0 ** -133}   # smallest subnormal = subnormal spacing
FP16_INF_FROM = 65520.0                                                    # fp32 values >= this round to fp16 inf
C_WALK = 4.0
SMALL = 1e-5
_CHUNK = 1 << 17                                                           # lookups per vectorised step


def runs(keys):
    """(start, length) of every run of equal keys in nz order."""
    keys = np.asarray(keys)
    n = keys.shape[0]
    if n == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    head = np.flatnonzero(np.concatenate([[True], keys[1:] != keys[:-1]]))
    return head, np.diff(np.concatenate([head, [n]]))


def _chunks(head, n):
    """Cut [0, n) into pieces of about _CHUNK lookups at run starts (a longer run is one piece)."""
    at = np.searchsorted(head, np.arange(_CHUNK, n, _CHUNK))
    cuts = [0] + sorted(set(int(h) for h in head[at[at < head.shape[0]]]) - {0}) + [n]
    return cuts


def backward(gy64, sample_ids, target, rows, w64=None):
    """Exact fp64 scatter-add: out[target[i]] += w64[i] * gy64[sample_ids[i]], for a COO whose equal targets form runs
    (fully sorted, or sorted block by block).  Returns dict(exact, scale, walk, run_len) with [rows, W] / [rows]."""
    target = np.asarray(target).astype(np.int64)
    sample_ids = np.asarray(sample_ids).astype(np.int64)
    n, W = target.shape[0], gy64.shape[1]
    exact, scale, sq = np.zeros((rows, W)), np.zeros((rows, W)), np.zeros((rows, W))
    run_len = np.zeros(rows, np.int64)
    head, lens = runs(target)
    cuts = _chunks(head, n)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        terms = gy64[sample_ids[lo:hi]]
        if w64 is not None:
            terms = terms * w64[lo:hi, None]
        h = head[(head >= lo) & (head < hi)] - lo
        ids = target[lo + h]
        np.add.at(exact, ids, np.add.reduceat(terms, h, axis=0))     # one entry per RUN, not per lookup
        np.add.at(scale, ids, np.add.reduceat(np.abs(terms), h, axis=0))
        np.add.at(sq, ids, np.add.reduceat(terms * terms, h, axis=0))
        np.add.at(run_len, ids, np.diff(np.concatenate([h, [hi - lo]])))
    return dict(exact=exact, scale=scale, walk=np.sqrt(sq), run_len=run_len)


def flushes_from_shape(target, rows, block_len, piece_len=0, extra=0):
    """16-bit roundings per output row for the segmented scatter-add whose workgroups cover `block_len` consecutive
    lookups (backward_launch_shape: segments_per_block * segment_len).  A run inside one workgroup is rounded once; a
    run that crosses b workgroup boundaries reaches the row as b + 1 atomics: b + 1 conversions of an fp32 partial
    plus b rounded additions.  piece_len > 0: the COO is launched piece by piece (sample blocks of that many lookups,
    workgroups restart at every piece) and a row's pieces add up -- one more rounding per earlier piece of the same
    row comes with it.  `extra` roundings are added to every row that receives a run."""
    target = np.asarray(target).astype(np.int64)
    n = target.shape[0]
    out = np.zeros(rows, np.int64)
    if n == 0:
        return out
    cut = np.zeros(n, dtype=bool)
    cut[0] = True
    cut[1:] = target[1:] != target[:-1]
    if piece_len:
        cut[np.arange(0, n, piece_len)] = True
    head = np.flatnonzero(cut)
    last = np.concatenate([head[1:], [n]]) - 1
    base = (head // piece_len) * piece_len if piece_len else 0
    crossings = (last - base) // block_len - (head - base) // block_len
    np.add.at(out, target[head], 1 + 2 * crossings)
    out[out > 0] += extra
    return out


def flushes_conservative(run_len):
    """Where the mapping cannot be derived: one rounding, plus one atomic per 256 lookups and one spare."""
    return 2 + np.asarray(run_len) // 256


def error_bound(kind, exact, scale, walk, flushes, c=C_WALK, small=SMALL):
    """|design - exact| may not exceed this (element-wise; flushes per row or per element)."""
    f = np.asarray(flushes, dtype=np.float64)
    if f.ndim == 1 and np.ndim(exact) == 2:
        f = f[:, None]
    f = np.maximum(f, 1.0)
    floor = SPACING[kind] * (1.0 + 0.5 * c * np.sqrt(f - 1.0))
    return EPS[kind] * (np.abs(exact) + c * np.sqrt(f - 1.0) * (walk + np.abs(exact))) + small * scale + floor


def weight_grad(table64, indices, gy64, sample_of_lookup):
    """Exact fp64 grad_w[i] = <table[indices[i]], gy[sample_of_lookup[i]]>, with scale = sum |t * g| per lookup."""
    indices = np.asarray(indices).astype(np.int64)
    s = np.asarray(sample_of_lookup).astype(np.int64)
    exact = np.empty(indices.shape[0])
    scale = np.empty(indices.shape[0])
    step = _CHUNK // 8
    for lo in range(0, indices.shape[0], step):
        hi = min(indices.shape[0], lo + step)
        t = table64[indices[lo:hi]] * gy64[s[lo:hi]]
        exact[lo:hi] = t.sum(axis=1)
        scale[lo:hi] = np.abs(t).sum(axis=1)
    return exact, scale


def weight_grad_bound(kind, width, exact, scale):
    """An fp32 dot product of `width` products rounded once to the output type."""
    return EPS[kind] * np.abs(exact) + width * 2.0 ** -24 * scale + SPACING[kind]


def forward(table64, indices, offsets, w64=None, mean=False):
    """Exact fp64 pooled rows: sum (or mean) of w * table[idx] over each bag; returns (exact, scale, hot) with
    scale = sum |w * table[idx]| (divided by |sum w| for a mean, like exact)."""
    indices = np.asarray(indices).astype(np.int64)
    offsets = np.asarray(offsets).astype(np.int64)
    B, W = offsets.shape[0] - 1, table64.shape[1]
    terms = table64[indices]
    w = np.ones(indices.shape[0]) if w64 is None else np.asarray(w64, dtype=np.float64)
    terms = terms * w[:, None]
    hot = np.diff(offsets)
    exact, scale = np.zeros((B, W)), np.zeros((B, W))
    full = hot > 0
    starts = offsets[:-1][full]
    if starts.size:
        exact[full] = np.add.reduceat(terms, starts, axis=0)
        scale[full] = np.add.reduceat(np.abs(terms), starts, axis=0)
    if mean:
        ws = np.zeros(B)
        if starts.size:
            ws[full] = np.add.reduceat(w, starts)
        inv = np.where(ws == 0, 0.0, 1.0 / np.where(ws == 0, 1.0, ws))
        exact *= inv[:, None]
        scale *= np.abs(inv)[:, None]
    return exact, scale, hot


def forward_split_bound(kind, exact, scale, hot):
    """fp32 partial pooled rows (one per wave, folded across lanes and through LDS) summed and rounded once: every
    fp32 addition may cost 2^-24 of the summed magnitudes, the final rounding EPS of the result."""
    h = np.asarray(hot, dtype=np.float64)[:, None]
    return EPS[kind] * np.abs(exact) + (h + 4.0) * 2.0 ** -24 * scale + SPACING[kind]


def assert_split_forward_within_bound(kind, fp16_math, g, exact, scale, hot, ora, mean, label):
    """What a forward under reduction_order="split" is held to (g, ora: the device's and the oracle's result as fp64).
    fp32 partials: the per-element bound above, and zeros for empty bags.  fp16 partials (fp16_math): per-element
    sensitivity is weak; per row, no more than twice the oracle's RMS error (a mean also scales the row by a
    reciprocal rounded to fp16 once: EPS of the row's RMS)."""
    if fp16_math:
        rms = np.sqrt(((g - exact) ** 2).mean(axis=1))
        rms_ora = np.sqrt(((ora - exact) ** 2).mean(axis=1))
        recip = EPS["f16"] * np.sqrt((exact ** 2).mean(axis=1)) if mean else 0.0
        assert np.all(rms <= 2.0 * rms_ora + recip + SPACING["f16"]), label
        return
    bound = forward_split_bound(kind, exact, scale, hot)
    worst = np.unravel_index(np.argmax(np.abs(g - exact) - bound), g.shape)
    assert np.all(np.abs(g - exact) <= bound), (label, worst, g[worst], exact[worst], bound[worst])
    assert np.all(g[hot == 0] == 0)


# ---- 16-bit conversions in numpy (round to nearest even), used by the host-side simulations ----
def round_bf16(a):
    x = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((x + 0x7fff + ((x >> 16) & 1)) >> 16).astype(np.uint32) << 16
    return r.astype(np.uint32).view(np.float32).reshape(np.shape(a))


def round_to(kind, a):
    """fp32 (or fp64) values rounded to `kind`, returned as fp32."""
    a32 = np.asarray(a, dtype=np.float32)
    if kind == "f16":
        return a32.astype(np.float16).astype(np.float32)
    if kind == "bf16":
        return round_bf16(a32)
    return a32
