"""Reference for the 8-bit row-wise quantized tables (numpy, no GPU): the quantizer recipe, the values of a fused
table in fp64 and in the kernels' two-rounding fp32 arithmetic, pooled sums / means in fp64, and the error bound the
device forward is held to.

Format (torch's fused 8-bit row-wise layout): uint8 [rows, W + 8]; bytes [0, W) codes, [W, W + 4) fp32 scale,
[W + 4, W + 8) fp32 bias, little endian; value = code * scale + bias.
"""
import numpy as np

F32 = np.float32
WIDTHS = (4, 8, 36, 64, 100, 128, 256, 512)
REGIMES = ("normal", "uniform", "offset", "lognormal", "constant")


def make_table(regime, rows, width, seed):
    """fp32 data of one regime: N(0, 9), U(0, 1), 1e4 + U(-1, 1), lognormal(0, 3), constant rows (a different constant
    per row).  None of them has a row whose scale would be subnormal: (max - min) / 255 < 2^-126 needs a row that spans
    less than 3e-36 without being constant, and those are left out ON PURPOSE -- torch's CPU kernels and the GPU may
    treat subnormal intermediates differently, and no embedding table looks like that."""
    rng = np.random.default_rng(seed)
    if regime == "normal":
        x = rng.normal(0.0, 3.0, (rows, width))
    elif regime == "uniform":
        x = rng.uniform(0.0, 1.0, (rows, width))
    elif regime == "offset":
        x = 1e4 + rng.uniform(-1.0, 1.0, (rows, width))
    elif regime == "lognormal":
        x = rng.lognormal(0.0, 3.0, (rows, width))
    elif regime == "constant":
        x = np.repeat(rng.normal(0.0, 3.0, (rows, 1)), width, axis=1)
    else:
        raise ValueError(regime)
    return x.astype(F32)


def quantize(x):
    """The recipe: every step one IEEE fp32 operation, round-half-even at the end.  x: [rows, W] (fp16 / bf16 data is
    widened to fp32 by the caller, exactly).  Returns uint8 [rows, W + 8]."""
    x = np.ascontiguousarray(x, dtype=F32)
    rows, width = x.shape
    mn = x.min(axis=1)
    mx = x.max(axis=1)
    rng = (mx - mn).astype(F32)
    scale = (rng / F32(255.0)).astype(F32)
    inv = (F32(255.0) / (rng + F32(1e-8)).astype(F32)).astype(F32)
    scaled = ((x - mn[:, None]).astype(F32) * inv[:, None]).astype(F32)
    out = np.empty((rows, width + 8), dtype=np.uint8)
    out[:, :width] = np.rint(scaled).astype(np.uint8)
    out[:, width:width + 4] = scale.astype("<f4").view(np.uint8).reshape(rows, 4)
    out[:, width + 4:] = mn.astype("<f4").view(np.uint8).reshape(rows, 4)
    return out


def split(q):
    """(codes uint8 [rows, W], scale fp32 [rows], bias fp32 [rows]) of a fused table."""
    q = np.ascontiguousarray(q)
    width = q.shape[1] - 8
    scale = q[:, width:width + 4].copy().view("<f4").reshape(-1)
    bias = q[:, width + 4:].copy().view("<f4").reshape(-1)
    return q[:, :width], scale, bias


def dequant64(q):
    """fp64 values of a fused table (exact: an 8-bit code times an fp32 scale plus an fp32 bias fits fp64 to well
    below the bound's resolution)."""
    codes, scale, bias = split(q)
    return codes.astype(np.float64) * scale.astype(np.float64)[:, None] + bias.astype(np.float64)[:, None]


def dequant32(q):
    """The dequantizer's arithmetic: float(code) * scale, rounded, + bias, rounded."""
    codes, scale, bias = split(q)
    return ((codes.astype(F32) * scale[:, None]).astype(F32) + bias[:, None]).astype(F32)


def bags_of(indices, offsets=None, num_hots=0):
    """[(begin, end)] of every bag."""
    if offsets is not None:
        offsets = np.asarray(offsets, dtype=np.int64)
        return [(int(offsets[s]), int(offsets[s + 1])) for s in range(offsets.size - 1)]
    n = np.asarray(indices).size // num_hots
    return [(s * num_hots, (s + 1) * num_hots) for s in range(n)]


def pooled64(q, indices, offsets=None, num_hots=0, weights=None, mode="sum", out="f32"):
    """(exact, bound) of a batch, both fp64 [batch, W].

    exact = sum_j w_j * (code_j * scale_j + bias_j), evaluated in fp64 from the fused bytes; mean multiplies by the
    reciprocal of the weight sum (zeros when it is 0).
    bound = (H + 2) * 2^-24 * sum_j |w_j| * (code_j * scale_j + |bias_j|), H the bag's length: one fp32 rounding per
    accumulated term plus the final add, against the magnitude of the terms as the cheapest arithmetic sees them -- code
    part and bias part counted separately, because an implementation that sums the biases per bag cancels large terms.
    Mean: the sum's bound times the reciprocal, plus one more 2^-24 relative.  fp16 output: plus 2^-11 |exact| plus
    half an fp16 subnormal (2^-25)."""
    codes, scale, bias = split(q)
    indices = np.asarray(indices, dtype=np.int64).reshape(-1)
    bags = bags_of(indices, offsets, num_hots)
    width = codes.shape[1]
    exact = np.zeros((len(bags), width))
    bound = np.zeros((len(bags), width))
    w_all = None if weights is None else np.asarray(weights).astype(np.float64).reshape(-1)
    for s, (b, e) in enumerate(bags):
        if e == b:
            continue
        r = indices[b:e]
        w = np.ones(e - b) if w_all is None else w_all[b:e]
        code_part = codes[r].astype(np.float64) * scale[r].astype(np.float64)[:, None]      # >= 0
        b64 = bias[r].astype(np.float64)
        total = (w[:, None] * (code_part + b64[:, None])).sum(axis=0)
        magnitude = (np.abs(w)[:, None] * (code_part + np.abs(b64)[:, None])).sum(axis=0)
        limit = (e - b + 2) * 2.0 ** -24 * magnitude
        if mode == "mean":
            wsum = w.sum()
            recip = 0.0 if wsum == 0.0 else 1.0 / wsum
            total = total * recip
            limit = limit * abs(recip) + 2.0 ** -24 * np.abs(total)
        exact[s] = total
        bound[s] = limit
    if out == "f16":
        bound = bound + 2.0 ** -11 * np.abs(exact) + 2.0 ** -25
    return exact, bound


def worst_ratio(got, exact, bound):
    """max |got - exact| / bound over all elements (0 / 0 counts as 0; anything over a zero bound as inf)."""
    err = np.abs(np.asarray(got, dtype=np.float64) - exact)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0.0, 0.0, err / bound)
    return float(np.nan_to_num(ratio, nan=np.inf).max()) if ratio.size else 0.0
