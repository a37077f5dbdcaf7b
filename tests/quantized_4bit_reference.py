"""Reference for the fused 4-bit row-wise quantized tables (numpy, no GPU): the quantizer recipe, the values of a
fused table in fp64 and in the kernels' two-rounding fp32 arithmetic, and an adapter onto tests/quantized_reference.py,
whose pooled64 and worst_ratio then serve as they are (scale and bias are exact in fp32, so the bound needs no new term).

Format (torch's fused 4-bit row-wise layout): uint8 [rows, W / 2 + 4]; byte i holds element 2i in its low nibble and
element 2i + 1 in its high nibble; bytes [W / 2, W / 2 + 2) fp16 scale, [W / 2 + 2, W / 2 + 4) fp16 bias, little endian;
value = code * scale + bias.
"""
import numpy as np

import quantized_reference as R8

F32 = np.float32
F16 = np.float16
WIDTHS = (8, 24, 48, 96, 256)        # 8 / 8 / 16 / 32 / 32 codes per lane: one lane and several of every variant


def quantize(x):
    """The recipe of torch's CPU prepack, every step one IEEE fp32 operation, ties to even.  x: [rows, W], W % 8 == 0
    (fp16 / bf16 data is widened to fp32 by the caller, exactly).  Returns uint8 [rows, W / 2 + 4]."""
    x = np.ascontiguousarray(x, dtype=F32)
    rows, width = x.shape
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        bias = x.min(axis=1).astype(F16)
        mn = bias.astype(F32)
        rng = (x.max(axis=1) - mn).astype(F32)
        scale = np.where(rng == 0, F32(1), (rng / F32(15)).astype(F32)).astype(F16)
        inv = np.where(scale.astype(F32) == 0, F32(1), (F32(1) / scale.astype(F32)).astype(F32)).astype(F32)
        reset = (scale.astype(F32) == 0) | np.isinf(inv)
        scale = np.where(reset, F16(1), scale)
        inv = np.where(reset, F32(1), inv)
        scaled = ((x - mn[:, None]).astype(F32) * inv[:, None]).astype(F32)
        codes = np.clip(np.rint(scaled), 0, 15).astype(np.uint8)
    out = np.empty((rows, width // 2 + 4), dtype=np.uint8)
    out[:, :width // 2] = codes[:, 0::2] | (codes[:, 1::2] << 4)
    out[:, width // 2:width // 2 + 2] = scale.astype("<f2").view(np.uint8).reshape(rows, 2)
    out[:, width // 2 + 2:] = bias.astype("<f2").view(np.uint8).reshape(rows, 2)
    return out


def split(q):
    """(codes uint8 [rows, W], scale fp32 [rows], bias fp32 [rows]) of a fused 4-bit table; scale and bias widened exactly."""
    q = np.ascontiguousarray(q)
    half = q.shape[1] - 4
    codes = np.empty((q.shape[0], 2 * half), dtype=np.uint8)
    codes[:, 0::2] = q[:, :half] & 0xF
    codes[:, 1::2] = q[:, :half] >> 4
    scale = q[:, half:half + 2].copy().view("<f2").reshape(-1).astype(F32)
    bias = q[:, half + 2:].copy().view("<f2").reshape(-1).astype(F32)
    return codes, scale, bias


def as_8bit(q):
    """The adapter: the fused 8-bit table (tests/quantized_reference.py's format) with the same codes, scale and bias --
    the same values exactly, so R8.pooled64 / R8.dequant32 of it are this table's."""
    codes, scale, bias = split(q)
    rows, width = codes.shape
    out = np.empty((rows, width + 8), dtype=np.uint8)
    out[:, :width] = codes
    out[:, width:width + 4] = scale.astype("<f4").view(np.uint8).reshape(rows, 4)
    out[:, width + 4:] = bias.astype("<f4").view(np.uint8).reshape(rows, 4)
    return out


def dequant64(q):
    """fp64 values of a fused 4-bit table (exact)."""
    return R8.dequant64(as_8bit(q))


def dequant32(q):
    """The dequantizer's arithmetic: float(code) * scale, rounded, + bias, rounded."""
    return R8.dequant32(as_8bit(q))


def pooled64(q, *args, **kwargs):
    """R8.pooled64 -- (exact, bound) of a batch -- on the same values."""
    return R8.pooled64(as_8bit(q), *args, **kwargs)
