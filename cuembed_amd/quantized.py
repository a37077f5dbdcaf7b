"""8-bit row-wise quantized tables on the device (an extension: inference only).

The format is PyTorch's fused 8-bit row-wise layout -- what `torch.ops.quantized.embedding_bag_byte_prepack` makes on
the CPU: a uint8 tensor [rows, W + 8]; bytes [0, W) of a row are its codes, [W, W + 4) its fp32 scale, [W + 4, W + 8)
its fp32 bias; a value is code * scale + bias.  A table prepacked by torch and moved to the device is a valid table
here, and `quantize_rows` writes the very bytes torch's prepack would.

    quantize_rows(table)                     fp32 / fp16 / bf16 [rows, W] -> uint8 [rows, W + 8]
    dequantize_rows(qtable, ids, dtype)      the values of all rows, or of the rows `ids` names
    embedding_forward_quantized(qtable, ...) embedding_forward on a fused table (sum / mean / concat)
    QuantizedEmbeddingBag                    a table + the scheduling hints cuemb_embedding(hints="auto") applies

Every function validates its arguments and raises before any launch; the kernels run on torch's current stream
(cuembed::QuantizeRows / DequantizeRows / EmbeddingForwardQuantized through the C ABI).  torch is used for device memory
and streams only.
"""
import ctypes

import torch

from . import _lib
from .ops import _CSR_XOR_FIXED, _MODES, _ROW_LOADS, CONCAT, _check_alignment, _check_dev, _elem_code, _index_code, _ptr, _stream

TRAILER_BYTES = 8                                   # fp32 scale + fp32 bias
_OUT = {torch.float32: 0, torch.float16: 1}


def quantized_row_bytes(width):
    """Bytes of one fused row of `width` values."""
    return int(width) + TRAILER_BYTES


def _no_grad(name, t):
    if t is not None and t.requires_grad:
        raise ValueError("%s requires grad: quantized tables are inference only (detach it)" % name)


def _check_qtable(qtable):
    """Validates a fused table (before the device check: the contract of the FORMAT first) and returns W."""
    if not isinstance(qtable, torch.Tensor):
        raise TypeError("qtable must be a torch.Tensor")
    if qtable.dtype != torch.uint8 or qtable.dim() != 2:
        raise TypeError("qtable must be a 2-D uint8 tensor [rows, width + 8] (the fused 8-bit row-wise layout)")
    if not qtable.is_contiguous():
        raise ValueError("qtable must be contiguous")
    width = qtable.shape[1] - TRAILER_BYTES
    if width <= 0 or width % 4 != 0:
        raise ValueError("row size must be a multiple of 4 bytes: the fused rows hold %d codes" % width)
    return width


def _out_code(name, dtype):
    if dtype not in _OUT:
        raise TypeError("%s must be torch.float32 or torch.float16, got %s" % (name, dtype))
    return _OUT[dtype]


def quantize_rows(table, out=None):
    """fp32 / fp16 / bf16 [rows, W] on the device -> uint8 [rows, W + 8], the fused 8-bit row-wise table.  Per row:
    scale = (max - min) / 255, bias = min, code = rint((x - min) * (255 / (max - min + 1e-8))), every step one fp32
    operation -- bit-identical to torch.ops.quantized.embedding_bag_byte_prepack on the CPU.  One launch."""
    if not isinstance(table, torch.Tensor):
        raise TypeError("table must be a torch.Tensor")
    et = _elem_code("table", table)
    if table.dim() != 2:
        raise ValueError("table must be [rows, width]")
    _no_grad("table", table)
    rows, width = table.shape
    if width <= 0 or width % 4 != 0:
        raise ValueError("row size must be a multiple of 4 bytes: width %d is not a multiple of 4" % width)
    _check_dev("table", table)
    if table.data_ptr() % 16 != 0:
        raise ValueError("table must be 16-byte aligned")
    if out is None:
        out = torch.empty((rows, width + TRAILER_BYTES), dtype=torch.uint8, device=table.device)
    else:
        _check_dev("out", out, table.device)
        if out.dtype != torch.uint8 or tuple(out.shape) != (rows, width + TRAILER_BYTES) or out.data_ptr() % 4 != 0:
            raise ValueError("out must be a 4-byte aligned uint8 tensor [rows, width + 8]")
    # (the quantizer's lane groups loop over a row: no limit on its lanes)
    _check_alignment("out", out.data_ptr(), 1, width, codes=True, max_lanes=None)
    if rows > 0:
        with torch.cuda.device(table.device):
            _lib.lib().cuembed_quantize_rows(_ptr(table), et, width, rows, _ptr(out), _stream(table))
    return out


def dequantize_rows(qtable, ids=None, dtype=torch.float32, out=None):
    """The values of a fused table as `dtype` (float32 or float16): all rows ([rows, W]) or, with `ids` (int32 / int64,
    any shape), the rows they name ([*ids.shape, W]).  float(code) * scale + bias in two rounded fp32 operations, then
    one rounding to `dtype`."""
    width = _check_qtable(qtable)
    oc = _out_code("dtype", dtype)
    _no_grad("qtable", qtable)
    it = 0
    if ids is not None:
        if not isinstance(ids, torch.Tensor):
            raise TypeError("ids must be a torch.Tensor")
        it = _index_code("ids", ids)
    _check_dev("qtable", qtable)
    if qtable.data_ptr() % 4 != 0:
        raise ValueError("qtable must be 4-byte aligned")
    if ids is not None:
        _check_dev("ids", ids, qtable.device)
    n = qtable.shape[0] if ids is None else ids.numel()
    shape = (n, width) if ids is None else tuple(ids.shape) + (width,)
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=qtable.device)
    else:
        _check_dev("out", out, qtable.device)
        if out.dtype != dtype or out.numel() != n * width or out.data_ptr() % 16 != 0:
            raise ValueError("out has the wrong dtype, size or alignment (16 bytes)")
    _check_alignment("qtable", qtable.data_ptr(), 1, width, codes=True)
    if n > 0:
        with torch.cuda.device(qtable.device):
            _lib.lib().cuembed_dequantize_rows(_ptr(qtable), width, _ptr(ids), it, n, _ptr(out), oc, _stream(qtable))
    return out


def quantized_forward_launch_shape(index_dtype, out_dtype, embed_width, batch_size, num_hots, is_csr=False,
                                   is_weighted=False, compute_units=256, xcds=8):
    """Launch shape of the quantized sum / mean forward (pure host arithmetic when compute_units > 0 describes the
    device: e.g. compute_units=32, xcds=1 for a CPX partition; 0 = ask the current device)."""
    out = (ctypes.c_int * 6)()
    _lib.lib().cuembed_quantized_forward_launch_shape(_index_code_of(index_dtype), _out_code("out_dtype", out_dtype),
                                                      int(embed_width), int(batch_size), int(num_hots), int(is_csr),
                                                      int(is_weighted), int(compute_units), int(xcds), out)
    return dict(codes_per_lane=out[0], lanes_per_row=out[1], samples_per_block=out[2], grid=out[3], lds_bytes=out[4],
                staged=out[5] == 1)


def _index_code_of(dtype):
    if dtype not in (torch.int32, torch.int64):
        raise TypeError("index dtype must be int32 or int64, got %s" % dtype)
    return 0 if dtype == torch.int32 else 1


def embedding_forward_quantized(qtable, indices, offsets=None, weights=None, batch_size=None, num_hots=0, mode="sum",
                                out_dtype=torch.float16, out=None, row_loads=None, sample_order=None,
                                row_loads_device=None):
    """out[s] = combine_j weights[s,j] * value(qtable[indices[s,j]]) on a fused 8-bit table.

    Same layouts and modes as embedding_forward: fixed hotness (offsets=None, num_hots>0) or CSR (offsets[batch+1],
    num_hots=0); mode "sum" | "mean" | "concat" (concat: fixed hotness, unweighted -- dequantize_rows on the batch's
    ids).  `weights` have the output's dtype (out_dtype: float16 or float32).  Accumulation is fp32, strictly in lookup
    order; empty bags give zeros.  row_loads ("default" | "streaming" | None), sample_order (CSR only) and
    row_loads_device are the scheduling hints of embedding_forward: they change no bit of the result.  No host
    read-back, no allocation inside the library: with `out=` given the call can be captured into a HIP graph."""
    if mode not in _MODES:
        raise ValueError("mode must be 'sum', 'mean' or 'concat'")
    if row_loads not in _ROW_LOADS:
        raise ValueError("row_loads: None, 'default' or 'streaming'")
    m = _MODES[mode]
    width = _check_qtable(qtable)
    oc = _out_code("out_dtype", out_dtype)
    if not isinstance(indices, torch.Tensor):
        raise TypeError("indices must be a torch.Tensor")
    it = _index_code("indices", indices)
    for name, t in (("qtable", qtable), ("weights", weights)):
        _no_grad(name, t)
    if weights is not None and m == CONCAT:
        raise ValueError("concat does not take weights")
    if not ((offsets is not None and num_hots == 0) or (offsets is None and num_hots > 0)):
        raise ValueError(_CSR_XOR_FIXED)
    if offsets is not None and m == CONCAT:
        raise ValueError("CSR layout does not support concat")
    if weights is not None and weights.dtype != out_dtype:
        raise TypeError("weights must have the output's dtype (%s), got %s" % (out_dtype, weights.dtype))
    ot = 0
    if offsets is not None:
        ot = _index_code("offsets", offsets)
        if batch_size is None:
            batch_size = offsets.numel() - 1
        if offsets.numel() < batch_size + 1:
            raise ValueError("offsets must hold batch_size + 1 entries")
    else:
        if batch_size is None:
            if indices.numel() % num_hots:
                raise ValueError("indices.numel() is not a multiple of num_hots")
            batch_size = indices.numel() // num_hots
        if indices.numel() < batch_size * num_hots:
            raise ValueError("indices must hold batch_size * num_hots entries")
    if weights is not None and weights.numel() < indices.numel():
        raise ValueError("weights must have one entry per index")
    if sample_order is not None and offsets is None:
        raise ValueError("sample_order is a hint for CSR batches (bags of different lengths)")
    # ---- the format and the call are in order: now the devices
    _check_dev("qtable", qtable)
    dev = qtable.device
    if qtable.data_ptr() % 4 != 0:
        raise ValueError("qtable must be 4-byte aligned")
    _check_dev("indices", indices, dev)
    if offsets is not None:
        _check_dev("offsets", offsets, dev)
    if weights is not None:
        _check_dev("weights", weights, dev)
    if sample_order is not None:
        _check_dev("sample_order", sample_order, dev)
        if sample_order.dtype != torch.int32 or sample_order.numel() != batch_size:
            raise ValueError("sample_order must be a contiguous int32 permutation of range(batch_size)")
    if row_loads_device is not None:
        _check_dev("row_loads_device", row_loads_device, dev)
        if row_loads_device.dtype != torch.int32 or row_loads_device.numel() < 4:
            raise ValueError("row_loads_device must be the contiguous 4-word int32 tensor decide_row_loads() fills")
    shape = (batch_size, num_hots, width) if m == CONCAT else (batch_size, width)
    if out is None:
        out = torch.empty(shape, dtype=out_dtype, device=dev)
    else:
        _check_dev("out", out, dev)
        if out.dtype != out_dtype or out.numel() != batch_size * (num_hots if m == CONCAT else 1) * width:
            raise ValueError("out has the wrong dtype or size")
        if out.data_ptr() % 16 != 0:
            raise ValueError("out must be 16-byte aligned")
    _check_alignment("qtable", qtable.data_ptr(), 1, width, codes=True)
    if batch_size > 0:
        with torch.cuda.device(dev):   # the launch must happen on the tensors' device
            _lib.lib().cuembed_embedding_forward_quantized(
                _ptr(qtable), width, _ptr(indices), it, _ptr(offsets), ot, _ptr(weights), batch_size, num_hots, m,
                _ptr(out), oc, _ROW_LOADS[row_loads], _ptr(sample_order), _ptr(row_loads_device), _stream(qtable))
    return out


class QuantizedEmbeddingBag:
    """A fused 8-bit table with the call shape of nn.EmbeddingBag / cuemb_embedding: bag(idx, offsets, weights).
    `offsets` holds batch + 1 entries.  hints="auto" applies the scheduling hints cuemb_embedding(hints="auto")
    applies -- the row-load decision and the bag order, both taken on the device by cuembed_amd.policy; results never
    depend on them."""

    def __init__(self, qtable, mode="sum", out_dtype=torch.float16, hints="auto"):
        _check_qtable(qtable)
        if mode not in ("sum", "mean"):
            raise ValueError("mode must be 'sum' or 'mean'")
        _out_code("out_dtype", out_dtype)
        if hints not in ("auto", None):
            raise ValueError("hints must be 'auto' or None")
        self.qtable = qtable
        self.mode = mode
        self.out_dtype = out_dtype
        self.hints = hints

    @classmethod
    def from_float(cls, table, mode="sum", out_dtype=torch.float16, hints="auto"):
        """Quantizes an fp32 / fp16 / bf16 table on the device."""
        return cls(quantize_rows(table.detach()), mode=mode, out_dtype=out_dtype, hints=hints)

    @property
    def num_embeddings(self):
        return self.qtable.shape[0]

    @property
    def embedding_dim(self):
        return self.qtable.shape[1] - TRAILER_BYTES

    def dequantize(self, ids=None, dtype=torch.float32):
        return dequantize_rows(self.qtable, ids, dtype)

    def __call__(self, idx, offsets, weights=None):
        order = decision = None
        if self.hints == "auto" and self.qtable.is_cuda and isinstance(idx, torch.Tensor) and idx.is_cuda:
            from . import cuembed_pyt, policy  # noqa: F401  (policy's device decisions are torch ops)
            order = policy.sample_order(offsets, idx.numel())
            decision = policy.row_loads_device(self.qtable, idx)
        return embedding_forward_quantized(self.qtable, idx, offsets, weights, mode=self.mode, out_dtype=self.out_dtype,
                                           sample_order=order, row_loads_device=decision)
