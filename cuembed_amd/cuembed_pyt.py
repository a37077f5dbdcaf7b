"""PyTorch op surface: the reference's `cuembed_pyt` torch library, rebuilt on PyTorch-ROCm.

Same op names and schemas as examples/pytorch/cuembed_embedding.cu:169-183 (registered for the
CUDA dispatch key, which is what HIP tensors use on ROCm) and the same Python entry point as
examples/pytorch/cuembed_pyt.py:48-51:

    from cuembed_amd.cuembed_pyt import cuemb_embedding
    out = cuemb_embedding(weight, indices, offsets, per_sample_weights)   # like nn.EmbeddingBag(sum)

The ops live in a native extension, cuembed_amd/lib/libcuembed_pyt.so (TORCH_LIBRARY +
TORCH_LIBRARY_IMPL in cuembed_amd/csrc/torch_binding.cpp, built by cuembed_amd/build.py), loaded
here with torch.ops.load_library exactly like the reference loads its own (cuembed_pyt.py:8-10).
They run the HIP kernels on torch's current stream.  Relative to the reference binding (fp32 /
int64 / sum only, cuembed_embedding.cu:15-32) they also accept fp16 / bf16 tables, int32 indices
and offsets and mode="mean".

CUEMBED_PYT_BACKEND=python registers the same ops from Python instead (torch.library + ctypes
calls into the same HIP library): kept for A/B timing of the binding overhead
(tools/torch_op_step_probe.py), not a fallback -- a missing native library is an error.
"""
import os

import torch

from . import ops as _ops
from . import policy as _policy

BACKEND = os.environ.get("CUEMBED_PYT_BACKEND", "native")
NATIVE_LIB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libcuembed_pyt.so")


def _load_native():
    from . import _lib as _clib
    _clib.lib()                                   # libcuembed_amd.so first: fail loudly if it is absent
    if not os.path.exists(NATIVE_LIB):
        raise _clib.CuembedLibraryError(
            "cuembed_amd: %s not found. Build it with `python -m cuembed_amd.build` (needs g++ and the "
            "torch headers); there is no fallback." % NATIVE_LIB)
    torch.ops.load_library(NATIVE_LIB)


def _define_python_ops():
    global _lib
    _lib = torch.library.Library("cuembed_pyt", "DEF")
    _lib.define("cuembed_extract_row_ids_from_csr(Tensor offsets, int nnz) ->Tensor")
    _lib.define("cuembed_transpose(Tensor rows, Tensor cols, Tensor weights) -> (Tensor, Tensor, Tensor)")
    _lib.define("cuembed_extract_row_ids_from_offsets(Tensor offsets, int nnz) -> Tensor")
    _lib.define("cuembed_transpose_bounded(Tensor rows, Tensor cols, Tensor weights, int num_categories)"
                " -> (Tensor, Tensor, Tensor)")
    _lib.define("cuembed_transpose_sample_ids(Tensor sample_ids, Tensor indices, Tensor weights, int num_categories)"
                " -> (Tensor, Tensor, Tensor)")
    _lib.define("cuembed_transpose_sample_blocks(Tensor sample_ids, Tensor indices, Tensor weights, int num_categories,"
                " int sample_blocks) -> (Tensor, Tensor, Tensor)")
    _lib.define("cuembed_transpose_fixed_hotness(Tensor indices, Tensor weights, int num_categories, bool compressed)"
                " -> (Tensor, Tensor, Tensor, Tensor)")
    _lib.define("cuembed_compute_compressed_grad_indices(Tensor transpose_indices) -> Tensor")
    _lib.define("cuembed_embedding_backward_compressed(Tensor y_grad, int num_unique, Tensor transpose_indices,"
                " Tensor transpose_sample_ids, Tensor transpose_remapped_indices, Tensor transpose_weights)"
                " -> (Tensor, Tensor)")
    _lib.define("cuembed_embedding_forward_fixed(Tensor params, Tensor indices, Tensor weights, str mode)"
                " -> Tensor")
    _lib.define("cuembed_embedding_weight_grad(Tensor params, Tensor indices, Tensor offsets, Tensor y_grad)"
                " -> Tensor")
    _lib.define("cuembed_embedding_forward(Tensor params, Tensor indices, Tensor offsets, Tensor weights,"
                " str mode) -> Tensor")
    _lib.define("cuembed_embedding_backward(Tensor y_grad, int num_categories, Tensor transpose_indices,"
                " Tensor transpose_sample_ids, Tensor transpose_weights) -> Tensor")
    _lib.define("cuembed_embedding_forward_hinted(Tensor params, Tensor indices, Tensor offsets, Tensor? weights,"
                " str mode, int row_loads, Tensor? sample_order, Tensor? row_loads_device) -> Tensor")
    _lib.define("cuembed_bag_order_by_length(Tensor offsets, int max_length) -> Tensor")
    _lib.define("cuembed_decide_row_loads(Tensor indices, int table_bytes, Tensor(a!) decision) -> ()")
    _lib.define("cuembed_sparse_row_update_(Tensor(a!) table, Tensor(b!)? state, Tensor ids, Tensor rows, str rule,"
                " float lr, float eps, Tensor? lr_device, int count, Tensor? counts, Tensor? last_id, int piece_rows,"
                " bool stochastic_rounding=False, int seed=0, int step=0, Tensor? step_device=None) -> ()")
    _lib.define("cuembed_sparse_row_adam_(Tensor(a!) table, Tensor(b!) exp_avg, Tensor(c!) exp_avg_sq, Tensor ids,"
                " Tensor rows, bool rowwise, float lr, float bias_factor, float beta1, float beta2, float eps,"
                " float weight_decay, Tensor? lr_device, Tensor? bias_factor_device, int count, Tensor? counts,"
                " Tensor? last_id, int piece_rows, bool stochastic_rounding=False, int seed=0, int step=0,"
                " Tensor? step_device=None) -> ()")
    _lib.define("cuembed_sparse_row_update_grouped(Tensor(a!)[] tables, Tensor table_ptrs, Tensor(b!)[] states,"
                " Tensor? state_ptrs, Tensor row_base, Tensor ids, Tensor rows, str rule, float lr, float eps,"
                " Tensor? lr_device, int count, Tensor? count_word, Tensor? last_id, bool stochastic_rounding=False,"
                " Tensor? seeds=None, int step=0, Tensor? step_device=None) -> ()")
    _lib.define("cuembed_sparse_row_adam_grouped(Tensor(a!)[] tables, Tensor table_ptrs, Tensor(b!)[] exp_avg,"
                " Tensor exp_avg_ptrs, Tensor(c!)[] exp_avg_sq, Tensor exp_avg_sq_ptrs, Tensor row_base, Tensor ids,"
                " Tensor rows, bool rowwise, float lr, float bias_factor, float beta1, float beta2, float eps,"
                " float weight_decay, Tensor? lr_device, Tensor? bias_factor_device, int count, Tensor? count_word,"
                " Tensor? last_id, bool stochastic_rounding=False, Tensor? seeds=None, int step=0,"
                " Tensor? step_device=None) -> ()")
    _lib.define("quantize_rows(Tensor table) -> Tensor")
    _lib.define("dequantize_rows(Tensor qtable, Tensor? ids, ScalarType dtype) -> Tensor")
    _lib.define("cuemb_embedding_quantized(Tensor qtable, Tensor indices, Tensor? offsets, Tensor? weights, str mode,"
                " ScalarType out_dtype, int row_loads, Tensor? sample_order, Tensor? row_loads_device) -> Tensor")
    _lib.define("cuemb_embedding_grouped(Tensor[] tables, Tensor table_ptrs, Tensor idx, Tensor? offsets, Tensor? weights,"
                " str mode, int row_loads=-1, Tensor? sample_order=None) -> Tensor")
    _lib.define("cuemb_embedding_quantized_grouped(Tensor[] qtables, Tensor table_ptrs, Tensor idx, Tensor? offsets,"
                " Tensor? weights, str mode, ScalarType out_dtype, int row_loads=-1, Tensor? sample_order=None) -> Tensor")
    _lib.define("cuemb_embedding_mixed_group(Tensor[] tables, Tensor table_ptrs, Tensor descriptor, int lane_bytes,"
                " Tensor idx, Tensor? offsets, Tensor? weights, str mode, int row_loads=-1) -> Tensor")
    _lib.define("cuembed_grouped_backward_keys(Tensor idx, Tensor? offsets, Tensor row_base, int num_tables, int batch,"
                " int num_hots, bool narrow) -> (Tensor, Tensor)")
    _lib.define("cuembed_grouped_table_cuts(Tensor ids, Tensor count_word, Tensor row_base, bool last_id=False) -> Tensor")
    _lib.define("cuembed_grouped_weight_grad(Tensor[] tables, Tensor table_ptrs, Tensor idx, Tensor? offsets,"
                " Tensor y_grad) -> Tensor")
    _lib.define("cuembed_grouped_mean_scale(Tensor y_grad, Tensor? offsets, Tensor? weights, int num_tables, int hotness)"
                " -> Tensor")
    _lib.define("cuembed_check_indices(Tensor indices, Tensor? offsets, Tensor? row_base, int num_rows, int num_tables,"
                " int batch, int num_hots, bool repair=False) -> (Tensor, Tensor, Tensor)")
    _lib.define("cuembed_embedding_backward_mixed_group(Tensor y_grad, int[] widths, Tensor table_columns,"
                " Tensor transpose_indices, Tensor transpose_sample_ids, Tensor transpose_remapped_indices,"
                " Tensor? transpose_weights, int capacity) -> (Tensor, Tensor, Tensor)")
    _lib.define("cuembed_mixed_group_mean_scale(Tensor y_grad, int[] widths, Tensor table_columns, Tensor? offsets,"
                " Tensor? weights, int hotness) -> Tensor")
    _lib.impl("cuembed_embedding_backward_mixed_group", _backward_mixed_group_impl, "CUDA")
    _lib.impl("cuembed_mixed_group_mean_scale", _mixed_group_mean_scale_impl, "CUDA")
    _lib.impl("cuembed_check_indices", _check_indices_impl, "CUDA")
    _lib.impl("cuembed_grouped_weight_grad", _grouped_weight_grad_impl, "CUDA")
    _lib.impl("cuembed_grouped_mean_scale", _grouped_mean_scale_impl, "CUDA")
    _lib.impl("cuembed_grouped_backward_keys", _grouped_backward_keys_impl, "CUDA")
    _lib.impl("cuembed_grouped_table_cuts", _grouped_table_cuts_impl, "CUDA")
    _lib.impl("cuemb_embedding_grouped", _embedding_grouped_impl, "CUDA")
    _lib.impl("cuemb_embedding_quantized_grouped", _embedding_quantized_grouped_impl, "CUDA")
    _lib.impl("cuemb_embedding_mixed_group", _embedding_mixed_group_impl, "CUDA")
    _lib.impl("quantize_rows", _quantize_rows_impl, "CUDA")
    _lib.impl("dequantize_rows", _dequantize_rows_impl, "CUDA")
    _lib.impl("cuemb_embedding_quantized", _embedding_quantized_impl, "CUDA")
    _lib.impl("cuembed_sparse_row_update_", _sparse_row_update_impl, "CUDA")
    _lib.impl("cuembed_sparse_row_adam_", _sparse_row_adam_impl, "CUDA")
    _lib.impl("cuembed_sparse_row_update_grouped", _sparse_row_update_grouped_impl, "CUDA")
    _lib.impl("cuembed_sparse_row_adam_grouped", _sparse_row_adam_grouped_impl, "CUDA")
    _lib.impl("cuembed_decide_row_loads", _decide_row_loads_impl, "CUDA")
    _lib.impl("cuembed_embedding_forward_hinted", _forward_hinted_impl, "CUDA")
    _lib.impl("cuembed_bag_order_by_length", _bag_order_impl, "CUDA")
    _lib.impl("cuembed_extract_row_ids_from_offsets", _extract_closed_impl, "CUDA")
    _lib.impl("cuembed_transpose_sample_ids", _transpose_sample_ids_impl, "CUDA")
    _lib.impl("cuembed_transpose_sample_blocks", _transpose_sample_blocks_impl, "CUDA")
    _lib.impl("cuembed_transpose_fixed_hotness", _transpose_fixed_impl, "CUDA")
    _lib.impl("cuembed_embedding_weight_grad", _weight_grad_impl, "CUDA")
    _lib.impl("cuembed_embedding_forward_fixed", _forward_fixed_impl, "CUDA")
    _lib.impl("cuembed_compute_compressed_grad_indices", _compress_impl, "CUDA")
    _lib.impl("cuembed_embedding_backward_compressed", _backward_compressed_impl, "CUDA")
    _lib.impl("cuembed_embedding_forward", _forward_impl, "CUDA")
    _lib.impl("cuembed_extract_row_ids_from_csr", _extract_impl, "CUDA")
    _lib.impl("cuembed_transpose", _transpose_impl, "CUDA")
    _lib.impl("cuembed_transpose_bounded", _transpose_bounded_impl, "CUDA")
    _lib.impl("cuembed_embedding_backward", _backward_impl, "CUDA")


# Extension ops beyond the reference's four (same list in torch_binding.cpp):
#   cuembed_transpose_bounded / _sample_ids   the transpose when the caller knows indices < num_categories
#                                             (and that `rows` are sample ids)
#   cuembed_transpose_sample_blocks           the transpose in blocks of samples, each sorted on its own (compressed
#                                             gradient only: uncoalesced, but every L2 gathers from 1 / blocks of
#                                             grad_y at a time -- C4 backward 0.258 -> 0.19 ms)
#   cuembed_transpose_fixed_hotness           row ids + transpose (+ dense ids) of a [batch, hotness] index
#                                             tensor in one call, sample ids never materialised
#   cuembed_compute_compressed_grad_indices,  compressed (sparse) table gradient: only the rows that were looked
#   cuembed_embedding_backward_compressed     up are materialised (293 MB instead of a zero-filled 5.12 GB at
#                                             the north-star shape)
#   cuembed_embedding_forward_fixed           fixed-hotness forward with every combine mode of the C++ API (the
#                                             reference binding only exposes CSR + sum, cuembed_embedding.cu:29-32)
#   cuembed_embedding_weight_grad             gradient w.r.t. the per-lookup weights
#   cuembed_sparse_row_update_                the sparse optimizer step on a compressed gradient, in place (SGD, Adagrad,
#                                             row-wise Adagrad; the entry count may stay on the device)
#   cuembed_sparse_row_adam_                  the same for the Adam family (lazy Adam, row-wise Adam; decoupled weight
#                                             decay; the bias factor may stay on the device)
#   cuembed_sparse_row_update_grouped,        both steps on a group of SEPARATE table tensors, in one launch each: the
#   cuembed_sparse_row_adam_grouped           kernel finds every entry's table itself (global row ids, row_base)
#   quantize_rows, dequantize_rows,           8-bit row-wise quantized tables in torch's own fused layout (inference
#   cuemb_embedding_quantized                 only): the quantizer, its inverse, and the lookup on a fused table
#   cuemb_embedding_grouped,                  a group of tables of one width and dtype pooled in ONE launch into
#   cuemb_embedding_quantized_grouped         [batch, tables, width] (forward only: no autograd formula)
#   cuemb_embedding_mixed_group               a group of plain tables of DIFFERENT widths pooled in ONE launch into
#                                             [batch, sum of widths] (forward only: no autograd formula)
#   cuembed_grouped_backward_keys,            the backward of a group through ONE sort and ONE scatter-add: global row
#   cuembed_grouped_table_cuts                keys + output-row sample ids in front of the single-table pipeline, the
#                                             table boundaries of the compressed gradient behind it
#                                             (cuemb_embedding_grouped_trainable is the autograd surface over them)
#   cuembed_grouped_weight_grad,              a trained group beyond sum pooling with table gradients: the gradient with
#   cuembed_grouped_mean_scale                respect to the per-lookup weights in ONE launch, and the launch that turns
#                                             the y_grad of a mean-pooled group into that of the sum-pooled one
#   cuembed_embedding_backward_mixed_group,   the backward of a MIXED-WIDTH group: the scatter-add for all widths (the
#   cuembed_mixed_group_mean_scale            compressed gradient padded to the widest table) behind the same keys and
#                                             sort, and the mean's scale on [batch, sum of widths]
#                                             (cuemb_embedding_mixed_group_trainable is the autograd surface over them)

_FLOATS = (torch.float32, torch.float16, torch.bfloat16)
_INTS = (torch.int64, torch.int32)


def _require(cond, msg):
    if not cond:
        raise RuntimeError("cuembed_pyt: " + msg)


def _forward_hinted_impl(params, indices, offsets, weights, mode, row_loads, sample_order, row_loads_device=None):
    return _forward_impl(params, indices, offsets, weights, mode, row_loads, sample_order, row_loads_device)


def _decide_row_loads_impl(indices, table_bytes, decision):
    _ops.decide_row_loads(indices, int(table_bytes), decision)


def _bag_order_impl(offsets, max_length):
    return _ops.bag_order_by_length(offsets.contiguous(), max_length=int(max_length))


def _forward_impl(params, indices, offsets, weights, mode, row_loads=-1, sample_order=None, row_loads_device=None):
    _require(params.is_cuda and indices.is_cuda and offsets.is_cuda, "tensors must be on the GPU")
    _require(params.dtype in _FLOATS, "params must be float32 or float16")
    _require(indices.dtype in _INTS and offsets.dtype in _INTS, "indices/offsets must be int64 or int32")
    _require(mode in ("sum", "mean"), "mode must be 'sum' (or 'mean')")
    if weights is not None:
        _require(weights.dtype == params.dtype, "weights must have the dtype of params")
        weights = weights.contiguous()
    batch_size = offsets.numel() - 1
    return _ops.embedding_forward(params.contiguous(), indices.contiguous(), offsets.contiguous(), weights,
                                  batch_size=batch_size, num_hots=0, mode=mode,
                                  row_loads=_ops._ROW_LOADS_BY_CODE[int(row_loads)],
                                  sample_order=sample_order, row_loads_device=row_loads_device)


def _extract_impl(offsets, nnz):
    _require(offsets.is_cuda, "offsets must be on the GPU")
    _require(offsets.dtype in _INTS, "offsets must be int64 or int32")
    # The reference passes `offsets[:-1]` and lets the kernel read one element past the slice
    # (cuembed_pyt.py:23 / cuembed_embedding.cu:60).  Here the end of the last bag is made
    # explicit from `nnz`, which is correct for the sliced AND the full offsets tensor.
    closed = torch.cat([offsets.reshape(-1), torch.tensor([nnz], dtype=offsets.dtype, device=offsets.device)])
    return _ops.extract_row_ids_from_csr(closed, nnz=nnz, dtype=offsets.dtype, batch_size=offsets.numel())


def _extract_closed_impl(offsets, nnz):
    _require(offsets.is_cuda and offsets.dtype in _INTS, "offsets must be int tensors on the GPU")
    return _ops.extract_row_ids_from_csr(offsets.contiguous(), nnz=nnz, dtype=offsets.dtype,
                                         batch_size=offsets.numel() - 1)


def _transpose_bounded_impl(rows, cols, weights, num_categories):
    return _transpose_impl(rows, cols, weights, num_categories)


def _transpose_sample_ids_impl(sample_ids, indices, weights, num_categories):
    return _transpose_impl(sample_ids, indices, weights, num_categories, num_rows=1 << 31)


def _transpose_sample_blocks_impl(sample_ids, indices, weights, num_categories, sample_blocks):
    return _transpose_impl(sample_ids, indices, weights, num_categories, num_rows=1 << 31, sample_blocks=sample_blocks)


def _transpose_fixed_impl(indices, weights, num_categories, compressed):
    _require(indices.is_cuda and indices.dim() == 2, "indices must be [batch, hotness] on the GPU")
    batch, hot = indices.shape
    w = None if weights is None else weights.contiguous().view(-1)
    t_idx, t_sid, t_w = _ops.transpose_fixed_hotness(indices.contiguous().view(-1), batch, hot, w,
                                                     num_categories=num_categories if num_categories > 0 else None)
    if t_w is None:
        t_w = torch.empty(0, dtype=torch.float32, device=indices.device)
    remap = _ops.compute_compressed_grad_indices(t_idx) if compressed else \
        torch.empty(0, dtype=indices.dtype, device=indices.device)
    return t_idx, t_sid, t_w, remap


def _transpose_impl(rows, cols, weights, num_categories=None, num_rows=None, sample_blocks=1):
    _require(rows.is_cuda and cols.is_cuda, "tensors must be on the GPU")
    _require(rows.dtype in _INTS and cols.dtype == rows.dtype, "rows/cols must both be int64 or int32")
    if weights is not None:
        _require(weights.dtype in _FLOATS, "weights must be float32 or float16")
        weights = weights.contiguous()
    t_rows, t_cols, t_w = _ops.transpose(rows.contiguous(), cols.contiguous(), weights,
                                         num_categories=num_categories, num_rows=num_rows, sample_blocks=sample_blocks)
    if t_w is None:  # the reference returns a 0-length float tensor (cuembed_embedding.cu:90-93)
        t_w = torch.empty(0, dtype=torch.float32, device=rows.device)
    return t_rows, t_cols, t_w


def _backward_impl(y_grad, num_categories, transpose_indices, transpose_sample_ids, transpose_weights):
    _require(y_grad.is_cuda and transpose_indices.is_cuda and transpose_sample_ids.is_cuda,
             "tensors must be on the GPU")
    _require(y_grad.dtype in _FLOATS, "y_grad must be float32 or float16")
    _require(transpose_indices.dtype in _INTS and transpose_sample_ids.dtype == transpose_indices.dtype,
             "transposed indices must be int64 or int32")
    if transpose_weights is not None:
        transpose_weights = transpose_weights.contiguous()
    width = y_grad.size(1)
    grad = torch.zeros((num_categories, width), dtype=y_grad.dtype, device=y_grad.device)
    _ops.embedding_backward(y_grad.contiguous(), num_categories, transpose_indices.contiguous(),
                            transpose_sample_ids.contiguous(), None, transpose_weights,
                            skip_grad_init=True, grad_embedding=grad)
    return grad


def _forward_fixed_impl(params, indices, weights, mode):
    _require(params.is_cuda and indices.is_cuda, "tensors must be on the GPU")
    _require(params.dtype in _FLOATS and indices.dtype in _INTS, "unsupported dtypes")
    _require(indices.dim() == 2, "indices must be [batch, hotness]")
    _require(mode in ("sum", "mean", "concat"), "mode must be 'sum', 'mean' or 'concat'")
    batch, hot = indices.shape
    if weights is not None:
        _require(weights.dtype == params.dtype and weights.shape == indices.shape,
                 "weights must match indices in shape and params in dtype")
        weights = weights.contiguous().view(-1)
    return _ops.embedding_forward(params.contiguous(), indices.contiguous().view(-1), None, weights,
                                  batch_size=batch, num_hots=hot, mode=mode)


def _weight_grad_impl(params, indices, offsets, y_grad):
    _require(params.is_cuda and indices.is_cuda and offsets.is_cuda and y_grad.is_cuda, "tensors must be on the GPU")
    return _ops.embedding_weight_grad(params.contiguous(), indices.contiguous(), y_grad.contiguous(),
                                      offsets=offsets.contiguous(), batch_size=offsets.numel() - 1, num_hots=0)


def _sparse_row_update_impl(table, state, ids, rows, rule, lr, eps, lr_device, count, counts, last_id, piece_rows,
                            stochastic_rounding=False, seed=0, step=0, step_device=None):
    _require((count >= 0) + (counts is not None) + (last_id is not None) <= 1,
             "give at most one of count, counts and last_id")
    if counts is not None and piece_rows > 0:
        kw = dict(counts=counts, piece_rows=piece_rows)
    elif counts is not None:
        kw = dict(count=counts)                 # one word for all entries
    elif last_id is not None:
        kw = dict(last_id=last_id)
    else:
        kw = dict(count=count if count >= 0 else None)
    if stochastic_rounding:     # (the schema's ints are signed 64-bit words: the same bits as the unsigned seed / step)
        kw.update(stochastic_rounding=True, seed=seed % 2 ** 64,
                  step=step % 2 ** 64 if step_device is None else step_device)
    _ops.sparse_row_update(table, ids, rows, rule=rule, lr=lr if lr_device is None else lr_device, state=state, eps=eps,
                           **kw)


def _sparse_row_adam_impl(table, exp_avg, exp_avg_sq, ids, rows, rowwise, lr, bias_factor, beta1, beta2, eps,
                          weight_decay, lr_device, bias_factor_device, count, counts, last_id, piece_rows,
                          stochastic_rounding=False, seed=0, step=0, step_device=None):
    _require((count >= 0) + (counts is not None) + (last_id is not None) <= 1,
             "give at most one of count, counts and last_id")
    if counts is not None and piece_rows > 0:
        kw = dict(counts=counts, piece_rows=piece_rows)
    elif counts is not None:
        kw = dict(count=counts)                 # one word for all entries
    elif last_id is not None:
        kw = dict(last_id=last_id)
    else:
        kw = dict(count=count if count >= 0 else None)
    if stochastic_rounding:     # (the schema's ints are signed 64-bit words: the same bits as the unsigned seed / step)
        kw.update(stochastic_rounding=True, seed=seed % 2 ** 64,
                  step=step % 2 ** 64 if step_device is None else step_device)
    _ops.sparse_row_adam(table, ids, rows, exp_avg=exp_avg, exp_avg_sq=exp_avg_sq,
                         lr=lr if lr_device is None else lr_device,
                         bias_factor=bias_factor if bias_factor_device is None else bias_factor_device,
                         betas=(beta1, beta2), eps=eps, weight_decay=weight_decay, rowwise=rowwise, **kw)


def _unsigned(word):
    """The unsigned 64-bit value whose bits the schema's int carries."""
    return int(word) & (2 ** 64 - 1)


def _signed(word):
    """An unsigned 64-bit value as the int of a schema (its bits, two's complement)."""
    word = int(word)
    return word - 2 ** 64 if word >= 2 ** 63 else word


def _grouped_count(count, count_word, last_id):
    _require((count >= 0) + (count_word is not None) + (last_id is not None) <= 1,
             "give at most one of count, count_word and last_id")
    if count_word is not None:
        return dict(count=count_word)
    if last_id is not None:
        return dict(last_id=last_id)
    return dict(count=count if count >= 0 else None)


def _sparse_row_update_grouped_impl(tables, table_ptrs, states, state_ptrs, row_base, ids, rows, rule, lr, eps, lr_device,
                                    count, count_word, last_id, stochastic_rounding=False, seeds=None, step=0,
                                    step_device=None):
    from . import grouped as _g, grouped_backward as _gb
    _gb.sparse_row_update_grouped(_g.TableGroup(tables, table_ptrs=table_ptrs), ids, rows, rule=rule,
                                  lr=lr if lr_device is None else lr_device, states=list(states) or None, eps=eps,
                                  stochastic_rounding=stochastic_rounding, seeds=seeds,
                                  step=_unsigned(step) if step_device is None else step_device,
                                  **_grouped_count(count, count_word, last_id))


def _sparse_row_adam_grouped_impl(tables, table_ptrs, exp_avg, exp_avg_ptrs, exp_avg_sq, exp_avg_sq_ptrs, row_base, ids,
                                  rows, rowwise, lr, bias_factor, beta1, beta2, eps, weight_decay, lr_device,
                                  bias_factor_device, count, count_word, last_id, stochastic_rounding=False, seeds=None,
                                  step=0, step_device=None):
    from . import grouped as _g, grouped_backward as _gb
    _gb.sparse_row_adam_grouped(_g.TableGroup(tables, table_ptrs=table_ptrs), ids, rows, exp_avg=list(exp_avg),
                                exp_avg_sq=list(exp_avg_sq), lr=lr if lr_device is None else lr_device,
                                bias_factor=bias_factor if bias_factor_device is None else bias_factor_device,
                                betas=(beta1, beta2), eps=eps, weight_decay=weight_decay, rowwise=rowwise,
                                stochastic_rounding=stochastic_rounding, seeds=seeds,
                                step=_unsigned(step) if step_device is None else step_device,
                                **_grouped_count(count, count_word, last_id))


def _quantize_rows_impl(table):
    from . import quantized as _q
    return _q.quantize_rows(table.contiguous())


def _dequantize_rows_impl(qtable, ids, dtype):
    from . import quantized as _q
    return _q.dequantize_rows(qtable, None if ids is None else ids.contiguous(), dtype)


def _embedding_quantized_impl(qtable, indices, offsets, weights, mode, out_dtype, row_loads, sample_order, row_loads_device):
    from . import quantized as _q
    if offsets is None:
        _require(indices.dim() == 2 and indices.shape[1] > 0, "without offsets, indices must be [batch, hotness]")
    return _q.embedding_forward_quantized(
        qtable, indices.contiguous(), None if offsets is None else offsets.contiguous(),
        None if weights is None else weights.contiguous(), num_hots=0 if offsets is not None else indices.shape[1],
        mode=mode, out_dtype=out_dtype, row_loads=_ops._ROW_LOADS_BY_CODE[int(row_loads)],
        sample_order=sample_order, row_loads_device=row_loads_device)


def _grouped_group(tables, table_ptrs):
    from . import grouped as _g
    return _g.TableGroup(tables, table_ptrs=table_ptrs)     # the caller's device pointers: nothing is copied here


def _embedding_grouped_impl(tables, table_ptrs, idx, offsets, weights, mode, row_loads=-1, sample_order=None):
    from . import grouped as _g
    if offsets is None:
        _require(idx.dim() == 3, "without offsets, idx must be [num_tables, batch, hotness]")
    return _g.embedding_forward_grouped(
        _grouped_group(tables, table_ptrs), idx.contiguous(), None if offsets is None else offsets.contiguous(),
        None if weights is None else weights.contiguous(), num_hots=0 if offsets is not None else idx.shape[2], mode=mode,
        row_loads=_ops._ROW_LOADS_BY_CODE[int(row_loads)], sample_order=sample_order)


def _embedding_mixed_group_impl(tables, table_ptrs, descriptor, lane_bytes, idx, offsets, weights, mode, row_loads=-1):
    from . import mixed_group as _m
    if offsets is None:
        _require(idx.dim() == 3, "without offsets, idx must be [num_tables, batch, hotness]")
    group = _m.MixedTableGroup(tables, table_ptrs=table_ptrs)   # the caller's device pointers: nothing is copied here
    batch = (offsets.numel() - 1) // len(tables) if offsets is not None else idx.shape[1]
    _require(descriptor.is_cuda and descriptor.dtype == torch.int32 and descriptor.is_contiguous() and
             descriptor.numel() == (len(tables) + 1) * 4,
             "descriptor must be the contiguous int32 tensor of (num_tables + 1) * 4 words on the tables' device")
    out = torch.empty((batch, group.embedding_dim), dtype=group.dtype, device=group.device)
    _require(group.lane_bytes(out.data_ptr()) == lane_bytes, "the descriptor was filled for another lane width")
    group._descriptors[(int(batch), int(lane_bytes))] = descriptor
    return _m.embedding_forward_mixed_group(
        group, idx.contiguous(), None if offsets is None else offsets.contiguous(),
        None if weights is None else weights.contiguous(), num_hots=0 if offsets is not None else idx.shape[2], mode=mode,
        row_loads=_ops._ROW_LOADS_BY_CODE[int(row_loads)], out=out)


def _embedding_quantized_grouped_impl(qtables, table_ptrs, idx, offsets, weights, mode, out_dtype, row_loads=-1,
                                      sample_order=None):
    from . import grouped as _g
    if offsets is None:
        _require(idx.dim() == 3, "without offsets, idx must be [num_tables, batch, hotness]")
    return _g.embedding_forward_quantized_grouped(
        _grouped_group(qtables, table_ptrs), idx.contiguous(), None if offsets is None else offsets.contiguous(),
        None if weights is None else weights.contiguous(), num_hots=0 if offsets is not None else idx.shape[2], mode=mode,
        out_dtype=out_dtype, row_loads=_ops._ROW_LOADS_BY_CODE[int(row_loads)],
        sample_order=sample_order)


def _grouped_backward_keys_impl(idx, offsets, row_base, num_tables, batch, num_hots, narrow):
    _require(idx.is_cuda and row_base.is_cuda and idx.dtype in _INTS, "idx must be an int tensor on the GPU")
    _require(row_base.dtype == torch.int64 and row_base.numel() == num_tables + 1 and row_base.is_contiguous(),
             "row_base must be the contiguous int64 tensor of num_tables + 1 row offsets")
    _require(num_tables >= 1 and batch >= 0 and num_tables * batch < 2 ** 31, "num_tables * batch must fit a 32-bit int")
    idx = idx.contiguous()
    nnz = idx.numel()
    if offsets is not None:
        _require(offsets.is_cuda and offsets.dtype in _INTS and num_hots == 0 and offsets.numel() == num_tables * batch + 1,
                 "CSR: num_hots = 0 and offsets of num_tables * batch + 1 entries")
        offsets = offsets.contiguous()
    else:
        _require(num_hots > 0 and nnz == num_tables * batch * num_hots,
                 "fixed hotness: num_hots > 0 and num_tables * batch * num_hots indices")
    kd = torch.int32 if narrow else torch.int64
    keys = torch.empty((nnz,), dtype=kd, device=idx.device)
    sample_ids = torch.empty((nnz,), dtype=kd, device=idx.device)
    if nnz > 0:
        from . import _lib as _clib
        with torch.cuda.device(idx.device):
            _clib.lib().cuembed_grouped_backward_keys(
                _ops._ptr(idx), _ops._INDEX[idx.dtype], _ops._ptr(offsets),
                0 if offsets is None else _ops._INDEX[offsets.dtype], _ops._ptr(row_base), int(num_tables), int(batch),
                int(num_hots), nnz, _ops._ptr(keys), _ops._ptr(sample_ids), _ops._INDEX[kd], _ops._stream(idx))
    return keys, sample_ids


def _grouped_table_cuts_impl(ids, count_word, row_base, last_id=False):
    from . import grouped_backward as _gb
    _require(ids.is_cuda and count_word.is_cuda and row_base.is_cuda, "tensors must be on the GPU")
    kw = dict(last_id=count_word) if last_id else dict(count=count_word)
    return _gb.grouped_table_cuts(ids.contiguous(), row_base, **kw)


def _grouped_weight_grad_impl(tables, table_ptrs, idx, offsets, y_grad):
    from . import grouped_backward as _gb
    if offsets is None:
        _require(idx.dim() == 3, "without offsets, idx must be [num_tables, batch, hotness]")
    _require(y_grad.dim() == 3, "y_grad must be [batch, num_tables, width]")
    return _gb.embedding_weight_grad_grouped(
        _grouped_group(tables, table_ptrs), y_grad.contiguous(), idx.contiguous(),
        None if offsets is None else offsets.contiguous(), num_hots=0 if offsets is not None else idx.shape[2])


def _mean_scale_batch(y_grad, offsets, weights, num_tables, batch, hotness):
    """What both mean scales check of their batch (the batch size is y_grad's): the contiguous (offsets, weights)."""
    if offsets is not None:
        _require(offsets.is_cuda and offsets.dtype in _INTS and hotness == 0 and offsets.numel() == num_tables * batch + 1,
                 "CSR: hotness = 0 and offsets of num_tables * batch + 1 entries")
        offsets = offsets.contiguous()
    else:
        _require(hotness > 0, "fixed hotness: hotness > 0")
    if weights is not None:
        _require(weights.is_cuda and weights.dtype == y_grad.dtype and
                 (offsets is not None or weights.numel() >= num_tables * batch * hotness),
                 "weights must have one entry per lookup, of y_grad's dtype")
        weights = weights.contiguous()
    return offsets, weights


def _grouped_mean_scale_impl(y_grad, offsets, weights, num_tables, hotness):
    from . import _lib as _clib
    _require(y_grad.is_cuda and y_grad.dtype in _FLOATS and y_grad.dim() == 3 and y_grad.shape[1] == num_tables >= 1,
             "y_grad must be a float [batch, num_tables, width] tensor on the GPU")
    batch, width = y_grad.shape[0], y_grad.shape[2]
    _require(num_tables * batch < 2 ** 31, "num_tables * batch must fit a 32-bit int")
    y_grad = y_grad.contiguous()
    offsets, weights = _mean_scale_batch(y_grad, offsets, weights, num_tables, batch, hotness)
    out = torch.empty_like(y_grad)
    if y_grad.numel() > 0:
        _ops._check_alignment("y_grad", y_grad.data_ptr(), y_grad.element_size(), width, others=(("out", out.data_ptr()),))
        with torch.cuda.device(y_grad.device):
            _clib.lib().cuembed_grouped_mean_scale(
                _ops._ptr(y_grad), _ops._ELEM[y_grad.dtype], int(width), _ops._ptr(offsets),
                0 if offsets is None else _ops._INDEX[offsets.dtype], _ops._ptr(weights), int(num_tables), int(batch),
                int(hotness), _ops._ptr(out), _ops._stream(y_grad))
    return out


def _mixed_columns(y_grad, widths, table_columns):
    """The widths as the C ABI takes them, checked against y_grad and table_columns: (ctypes array, D, W_max).
    table_columns must be MixedTableGroup.table_columns_device of the group the widths belong to: its dtype and size are
    checked, its contents (on the device) are not -- the kernels address y_grad and pick their lanes from them."""
    import ctypes
    widths = [int(w) for w in widths]
    _require(y_grad.is_cuda and y_grad.dtype in _FLOATS, "y_grad must be a float tensor on the GPU")
    _require(len(widths) >= 1 and all(w > 0 and (w * y_grad.element_size()) % 4 == 0 for w in widths) and
             sum(widths) < 2 ** 31, "every row must be a multiple of 4 bytes and the widths sum to at most 2^31 - 1")
    _require(table_columns.is_cuda and table_columns.dtype == torch.int32 and table_columns.is_contiguous() and
             table_columns.numel() == 2 * len(widths),
             "table_columns must be the contiguous int32 [num_tables, 2] tensor of (column base, width)")
    _require(y_grad.dim() == 2 and y_grad.shape[1] == sum(widths), "y_grad must be [batch, sum of the widths]")
    _require(len(widths) * y_grad.shape[0] < 2 ** 31, "num_tables * batch must fit a 32-bit int")
    return (ctypes.c_int * len(widths))(*widths), sum(widths), max(widths)


def _mixed_lane_elems(widths, itemsize, *pointers):
    from .group_layout import mixed_lane_bytes
    _require(all(int(p) % 4 == 0 for p in pointers), "y_grad must be 4-byte aligned")
    return mixed_lane_bytes([int(w) for w in widths], itemsize, [("y_grad", p) for p in pointers]) // itemsize


def _backward_mixed_group_impl(y_grad, widths, table_columns, transpose_indices, transpose_sample_ids,
                               transpose_remapped_indices, transpose_weights, capacity):
    from . import _lib as _clib
    w_host, dim, w_max = _mixed_columns(y_grad, widths, table_columns)
    _require(capacity >= 0, "capacity must not be negative")
    nnz = transpose_indices.numel()
    _require(transpose_indices.is_cuda and transpose_indices.dtype in _INTS and nnz < 2 ** 31,
             "transpose_indices must be an int tensor on the GPU of fewer than 2^31 entries")
    for t in (transpose_sample_ids, transpose_remapped_indices):
        _require(t.is_cuda and t.dtype == transpose_indices.dtype and t.numel() == nnz,
                 "the sample ids and the remapped ids must match transpose_indices")
    y_grad = y_grad.contiguous()
    if transpose_weights is not None and transpose_weights.numel() == 0:
        transpose_weights = None
    if transpose_weights is not None:
        _require(transpose_weights.is_cuda and transpose_weights.dtype == y_grad.dtype and
                 transpose_weights.numel() >= nnz, "transpose_weights must have one entry per lookup, of y_grad's dtype")
        transpose_weights = transpose_weights.contiguous()
    dev = y_grad.device
    rows = torch.empty((capacity, w_max), dtype=y_grad.dtype, device=dev)
    ids = torch.empty((capacity,), dtype=transpose_indices.dtype, device=dev)
    overflow = torch.zeros((1,), dtype=torch.int32, device=dev)
    if nnz == 0:
        return rows, ids, overflow
    if capacity == 0:
        return rows, ids, overflow.fill_(1)
    n = _mixed_lane_elems(widths, y_grad.element_size(), y_grad.data_ptr(), rows.data_ptr())
    _require(w_max // n <= 1024, "the widest table is more than 1024 lanes")
    _require(y_grad.shape[0] * (dim // n) < 2 ** 31, "batch * sum of the widths / elements per lane must stay below 2^31")
    with torch.cuda.device(dev):
        _clib.lib().cuembed_embedding_backward_mixed_group(
            _ops._ptr(y_grad), _ops._ELEM[y_grad.dtype], w_host, _ops._ptr(table_columns), len(widths),
            int(y_grad.shape[0]), nnz, _ops._ptr(transpose_indices.contiguous()),
            _ops._ptr(transpose_sample_ids.contiguous()), _ops._ptr(transpose_remapped_indices.contiguous()),
            _ops._INDEX[transpose_indices.dtype], _ops._ptr(transpose_weights), _ops._ptr(rows), _ops._ptr(ids),
            int(capacity), _ops._ptr(overflow), _ops._stream(y_grad))
    return rows, ids, overflow


def _mixed_group_mean_scale_impl(y_grad, widths, table_columns, offsets, weights, hotness):
    from . import _lib as _clib
    w_host, _, _ = _mixed_columns(y_grad, widths, table_columns)
    num_tables, batch = len(widths), y_grad.shape[0]
    y_grad = y_grad.contiguous()
    offsets, weights = _mean_scale_batch(y_grad, offsets, weights, num_tables, batch, hotness)
    out = torch.empty_like(y_grad)
    if batch > 0:
        _mixed_lane_elems(widths, y_grad.element_size(), y_grad.data_ptr(), out.data_ptr())
        with torch.cuda.device(y_grad.device):
            _clib.lib().cuembed_mixed_group_mean_scale(
                _ops._ptr(y_grad), _ops._ELEM[y_grad.dtype], w_host, _ops._ptr(table_columns), _ops._ptr(offsets),
                0 if offsets is None else _ops._INDEX[offsets.dtype], _ops._ptr(weights), num_tables, int(batch),
                int(hotness), _ops._ptr(out), _ops._stream(y_grad))
    return out


def _check_indices_impl(indices, offsets, row_base, num_rows, num_tables, batch, num_hots, repair=False):
    import ctypes
    from . import _lib as _clib
    _require(indices.is_cuda and indices.dtype in _INTS, "indices must be int tensors on the GPU")
    _require(1 <= num_tables <= 1023, "1 <= num_tables <= 1023")
    if row_base is not None:
        _require(row_base.is_cuda and row_base.dtype == torch.int64 and row_base.numel() == num_tables + 1 and
                 row_base.is_contiguous() and row_base.device == indices.device,
                 "row_base must be the contiguous int64 tensor of num_tables + 1 entries on indices' device")
    else:
        _require(num_tables == 1 and num_rows >= 1, "without row_base: one table of num_rows >= 1 rows")
    _require(batch >= 0 and num_tables * batch < 2 ** 31, "num_tables * batch must fit a 32-bit int")
    indices = indices.contiguous()
    nnz = indices.numel()
    _require(nnz <= 2 ** 38, "at most 2^38 lookups per call")
    if offsets is not None:
        _require(offsets.is_cuda and offsets.dtype in _INTS and num_hots == 0 and offsets.numel() == num_tables * batch + 1
                 and offsets.device == indices.device,
                 "CSR: num_hots = 0 and offsets of num_tables * batch + 1 entries on indices' device")
        _require(offsets.dtype == torch.int64 or nnz < 2 ** 31, "int32 offsets cannot address that many lookups")
        offsets = offsets.contiguous()
    else:
        _require(num_hots > 0 and nnz == num_tables * batch * num_hots,
                 "fixed hotness: num_hots > 0 and indices of num_tables * batch * num_hots entries")
    like = offsets if offsets is not None else indices
    report = torch.empty((4,), dtype=torch.int64, device=indices.device)
    out_i = torch.empty_like(indices) if repair else torch.empty((0,), dtype=indices.dtype, device=indices.device)
    out_o = (torch.empty_like(offsets) if repair and offsets is not None
             else torch.empty((0,), dtype=like.dtype, device=like.device))
    it, ot = _ops._INDEX[indices.dtype], 0 if offsets is None else _ops._INDEX[offsets.dtype]
    shape = (_ops._ptr(row_base), int(num_rows), int(num_tables), int(batch), int(num_hots))
    need = ctypes.c_size_t(0)
    _clib.lib().cuembed_check_indices(None, it, None, ot, nnz, *shape, None, None, None, None, ctypes.byref(need), None)
    work = torch.empty((max(need.value, 8),), dtype=torch.uint8, device=indices.device)
    with torch.cuda.device(indices.device):
        _clib.lib().cuembed_check_indices(
            _ops._ptr(indices), it, _ops._ptr(offsets), ot, nnz, *shape, _ops._ptr(report),
            _ops._ptr(out_i) if repair else None, _ops._ptr(out_o) if repair and offsets is not None else None,
            _ops._ptr(work), ctypes.byref(need), _ops._stream(indices))
    return report, out_i, out_o


def _compress_impl(transpose_indices):
    _require(transpose_indices.is_cuda and transpose_indices.dtype in _INTS, "indices must be int tensors on the GPU")
    return _ops.compute_compressed_grad_indices(transpose_indices.contiguous())


def _backward_compressed_impl(y_grad, num_unique, transpose_indices, transpose_sample_ids,
                              transpose_remapped_indices, transpose_weights):
    _require(y_grad.is_cuda and y_grad.dtype in _FLOATS, "y_grad must be float32/float16 on the GPU")
    if transpose_weights is not None:
        transpose_weights = transpose_weights.contiguous()
    grad, inv = _ops.embedding_backward(y_grad.contiguous(), num_unique, transpose_indices.contiguous(),
                                        transpose_sample_ids.contiguous(),
                                        transpose_remapped_indices.contiguous(), transpose_weights,
                                        skip_grad_init=False)
    return grad, inv




if BACKEND == "python":
    _define_python_ops()
elif BACKEND == "native":
    _load_native()
else:
    raise ValueError("CUEMBED_PYT_BACKEND must be 'native' or 'python'")

cuembed_extract_row_ids_from_csr = torch.ops.cuembed_pyt.cuembed_extract_row_ids_from_csr
cuembed_transpose = torch.ops.cuembed_pyt.cuembed_transpose
cuembed_transpose_bounded = torch.ops.cuembed_pyt.cuembed_transpose_bounded
cuembed_transpose_sample_ids = torch.ops.cuembed_pyt.cuembed_transpose_sample_ids
cuembed_transpose_fixed_hotness = torch.ops.cuembed_pyt.cuembed_transpose_fixed_hotness
cuembed_embedding_forward = torch.ops.cuembed_pyt.cuembed_embedding_forward
cuembed_embedding_backward = torch.ops.cuembed_pyt.cuembed_embedding_backward


def _signed_word(name, v):
    """An int in [0, 2**64) as the signed 64-bit word of the same bits (what a torch op's `int` carries)."""
    if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v < 2 ** 64:
        raise ValueError("%s must be an int in [0, 2**64), got %r" % (name, v))
    return v - 2 ** 64 if v >= 2 ** 63 else v


def cuembed_sparse_row_update_(table, ids, rows, rule, lr, state=None, eps=1e-8, count=None, last_id=None, counts=None,
                               piece_rows=None, stochastic_rounding=False, seed=0, step=0):
    """cuembed_amd.ops.sparse_row_update as the torch op cuembed_pyt::cuembed_sparse_row_update_ (in place on `table` and
    `state`; traces under torch.compile).  Same arguments."""
    lr_device = lr if isinstance(lr, torch.Tensor) else None
    word = count if isinstance(count, torch.Tensor) else None
    if word is not None and counts is not None:
        raise ValueError("give at most one of count=, last_id= and counts=")
    args = (table, state, ids, rows, rule, 0.0 if lr_device is not None else float(lr), float(eps), lr_device,
            -1 if (count is None or word is not None) else int(count), counts if word is None else word, last_id,
            0 if piece_rows is None else int(piece_rows))
    if not stochastic_rounding:
        torch.ops.cuembed_pyt.cuembed_sparse_row_update_(*args)
        return
    step_device = step if isinstance(step, torch.Tensor) else None
    torch.ops.cuembed_pyt.cuembed_sparse_row_update_(
        *args, True, _signed_word("seed", seed), 0 if step_device is not None else _signed_word("step", step), step_device)


def cuembed_sparse_row_adam_(table, ids, rows, *, exp_avg, exp_avg_sq, lr, bias_factor=1.0, betas=(0.9, 0.999), eps=1e-8,
                             weight_decay=0.0, rowwise=False, count=None, last_id=None, counts=None, piece_rows=None,
                             stochastic_rounding=False, seed=0, step=0):
    """cuembed_amd.ops.sparse_row_adam as the torch op cuembed_pyt::cuembed_sparse_row_adam_ (in place on `table`,
    `exp_avg` and `exp_avg_sq`; traces under torch.compile).  Same arguments."""
    lr_device = lr if isinstance(lr, torch.Tensor) else None
    bias_device = bias_factor if isinstance(bias_factor, torch.Tensor) else None
    word = count if isinstance(count, torch.Tensor) else None
    if word is not None and counts is not None:
        raise ValueError("give at most one of count=, last_id= and counts=")
    beta1, beta2 = betas
    args = (table, exp_avg, exp_avg_sq, ids, rows, bool(rowwise), 0.0 if lr_device is not None else float(lr),
            1.0 if bias_device is not None else float(bias_factor), float(beta1), float(beta2), float(eps),
            float(weight_decay), lr_device, bias_device, -1 if (count is None or word is not None) else int(count),
            counts if word is None else word, last_id, 0 if piece_rows is None else int(piece_rows))
    if not stochastic_rounding:
        torch.ops.cuembed_pyt.cuembed_sparse_row_adam_(*args)
        return
    step_device = step if isinstance(step, torch.Tensor) else None
    torch.ops.cuembed_pyt.cuembed_sparse_row_adam_(
        *args, True, _signed_word("seed", seed), 0 if step_device is not None else _signed_word("step", step), step_device)


def _grouped_step_args(group, count, last_id):
    from . import grouped as _g
    group = _g._as_group(group)
    word = count if isinstance(count, torch.Tensor) else None
    return group, -1 if (count is None or word is not None) else int(count), word


def _grouped_rounding_args(group, seeds, step):
    """(seeds tensor or None, step, step_device) of a grouped op.  Whether the rounding and the seeds go together is the
    op's to say: only the seeds themselves are validated here, since they have to be put on the device."""
    from . import grouped_backward as _gb
    if seeds is not None and not isinstance(seeds, torch.Tensor):
        seeds = _gb._seeds_tensor(group, _gb._check_seeds(group, True, seeds))
    if isinstance(step, torch.Tensor):
        return seeds, 0, step
    if isinstance(step, bool) or not isinstance(step, int) or not 0 <= step < 2 ** 64:
        raise ValueError("step must be an int in [0, 2**64) or a one-element int64 device tensor, got %r" % (step,))
    return seeds, _signed(step), None


def cuembed_sparse_row_update_grouped(group, ids, rows, *, rule, lr, states=None, eps=1e-8, count=None, last_id=None,
                                      stochastic_rounding=False, seeds=None, step=0):
    """cuembed_amd.sparse_row_update_grouped as the torch op cuembed_pyt::cuembed_sparse_row_update_grouped (in place on the
    group's tables and on `states`; traces under torch.compile).  Same arguments; the op takes the seeds as the int64
    device tensor [num_tables] of their bits, which is built once per tuple of seeds and kept on the group."""
    from . import grouped_backward as _gb
    group, host_count, word = _grouped_step_args(group, count, last_id)
    seeds, step, step_device = _grouped_rounding_args(group, seeds, step)
    lr_device = lr if isinstance(lr, torch.Tensor) else None
    state_ptrs = None if not states else _gb._state_ptrs(group, states)[1]
    torch.ops.cuembed_pyt.cuembed_sparse_row_update_grouped(
        list(group.tables), group.table_ptrs, list(states or ()), state_ptrs, group.row_base_device, ids, rows, rule,
        0.0 if lr_device is not None else float(lr), float(eps), lr_device, host_count, word, last_id,
        bool(stochastic_rounding), seeds, step, step_device)


def cuembed_sparse_row_adam_grouped(group, ids, rows, *, exp_avg, exp_avg_sq, lr, bias_factor=1.0, betas=(0.9, 0.999),
                                    eps=1e-8, weight_decay=0.0, rowwise=False, count=None, last_id=None,
                                    stochastic_rounding=False, seeds=None, step=0):
    """cuembed_amd.sparse_row_adam_grouped as the torch op cuembed_pyt::cuembed_sparse_row_adam_grouped (in place on the
    group's tables, `exp_avg` and `exp_avg_sq`; traces under torch.compile).  Same arguments."""
    from . import grouped_backward as _gb
    group, host_count, word = _grouped_step_args(group, count, last_id)
    seeds, step, step_device = _grouped_rounding_args(group, seeds, step)
    lr_device = lr if isinstance(lr, torch.Tensor) else None
    bias_device = bias_factor if isinstance(bias_factor, torch.Tensor) else None
    beta1, beta2 = betas
    torch.ops.cuembed_pyt.cuembed_sparse_row_adam_grouped(
        list(group.tables), group.table_ptrs, list(exp_avg), _gb._state_ptrs(group, exp_avg)[1], list(exp_avg_sq),
        _gb._state_ptrs(group, exp_avg_sq)[1], group.row_base_device, ids, rows, bool(rowwise),
        0.0 if lr_device is not None else float(lr), 1.0 if bias_device is not None else float(bias_factor), float(beta1),
        float(beta2), float(eps), float(weight_decay), lr_device, bias_device, host_count, word, last_id,
        bool(stochastic_rounding), seeds, step, step_device)


def quantize_rows(table):
    """cuembed_amd.quantize_rows as the torch op cuembed_pyt::quantize_rows (traces under torch.compile)."""
    return torch.ops.cuembed_pyt.quantize_rows(table)


def dequantize_rows(qtable, ids=None, dtype=torch.float32):
    """cuembed_amd.dequantize_rows as the torch op cuembed_pyt::dequantize_rows."""
    return torch.ops.cuembed_pyt.dequantize_rows(qtable, ids, dtype)


def cuemb_embedding_quantized(qtable, idx, offsets=None, weights=None, mode="sum", out_dtype=torch.float16, hints="auto"):
    """The lookup on a fused 8-bit row-wise table (torch's quantized::embedding_bag_byte_prepack layout) as the torch op
    cuembed_pyt::cuemb_embedding_quantized: CSR with `offsets` (batch + 1 entries), fixed hotness with idx [batch,
    hotness] and no offsets (then mode may be "concat").  Inference only: nothing here is differentiable.
    hints="auto" applies cuembed_amd.policy's scheduling hints like cuemb_embedding; results never depend on them."""
    order = decision = None
    if hints == "auto" and not torch.compiler.is_compiling():
        order = _policy.sample_order(offsets, idx.numel())
        decision = _policy.row_loads_device(qtable, idx)
    return torch.ops.cuembed_pyt.cuemb_embedding_quantized(qtable, idx, offsets, weights, mode, out_dtype, -1, order,
                                                           decision)


def _forward_only(tables, weights):
    if torch.is_grad_enabled() and (any(t.requires_grad for t in tables) or
                                    (weights is not None and weights.requires_grad)):
        raise RuntimeError("cuembed_pyt: the grouped forward is forward only: a table (or the weights) requires grad; "
                           "call it under torch.no_grad() or detach")


def cuemb_embedding_grouped(group, idx, offsets=None, weights=None, mode="sum", row_loads=None, sample_order=None):
    """cuembed_amd.embedding_forward_grouped as the torch op cuembed_pyt::cuemb_embedding_grouped: `group` is a
    cuembed_amd.TableGroup (the tables and the device tensor of their base pointers, built once); CSR with `offsets`
    (num_tables * batch + 1 entries) or fixed hotness with idx [num_tables, batch, hotness].  Returns [batch, num_tables,
    width].  Forward only: the op has no autograd formula."""
    _forward_only(group.tables, weights)
    return torch.ops.cuembed_pyt.cuemb_embedding_grouped(list(group.tables), group.table_ptrs, idx, offsets, weights, mode,
                                                         _ops._ROW_LOADS[row_loads], sample_order)


def cuemb_embedding_mixed_group(group, idx, offsets=None, weights=None, mode="sum", row_loads=None):
    """cuembed_amd.embedding_forward_mixed_group as the torch op cuembed_pyt::cuemb_embedding_mixed_group: `group` is a
    cuembed_amd.MixedTableGroup (tables of different widths; the device tensors of their pointers and of the
    per-batch-size descriptor are built once); CSR with `offsets` (num_tables * batch + 1 entries) or fixed hotness with
    idx [num_tables, batch, hotness].  Returns [batch, group.embedding_dim].  Forward only: no autograd formula."""
    _forward_only(group.tables, weights)
    batch, _ = _grouped_batch(group.num_tables, idx, offsets)
    lane = group.lane_bytes()          # (the op's result is a fresh, 16-byte aligned tensor)
    return torch.ops.cuembed_pyt.cuemb_embedding_mixed_group(list(group.tables), group.table_ptrs,
                                                             group.descriptor(batch, lane), lane, idx, offsets, weights,
                                                             mode, _ops._ROW_LOADS[row_loads])


def cuemb_embedding_quantized_grouped(group, idx, offsets=None, weights=None, mode="sum", out_dtype=torch.float16,
                                      row_loads=None, sample_order=None):
    """cuembed_amd.embedding_forward_quantized_grouped as the torch op cuembed_pyt::cuemb_embedding_quantized_grouped
    (a TableGroup of fused 8-bit tables).  Inference only."""
    _forward_only(group.tables, weights)
    return torch.ops.cuembed_pyt.cuemb_embedding_quantized_grouped(list(group.tables), group.table_ptrs, idx, offsets,
                                                                   weights, mode, out_dtype, _ops._ROW_LOADS[row_loads],
                                                                   sample_order)


def _grouped_batch(num_tables, idx, offsets):
    """(batch, hotness) of a grouped call: CSR offsets of num_tables * batch + 1 entries, or idx [num_tables, batch, hot]."""
    if offsets is not None:
        from .group_layout import csr_batch_size
        batch = csr_batch_size(num_tables, offsets.numel())
        if batch is None:
            raise ValueError("offsets must hold num_tables * batch + 1 entries")
        return batch, 0
    if idx.dim() != 3 or idx.shape[0] != num_tables or idx.shape[2] < 1:
        raise ValueError("without offsets, idx must be [num_tables, batch, hotness]")
    return idx.shape[1], idx.shape[2]


def _empty_sparse(rows, width, dtype, device):
    return torch.sparse_coo_tensor(torch.empty((1, 0), dtype=torch.int64, device=device),
                                   torch.empty((0, width), dtype=dtype, device=device), size=(rows, width),
                                   is_coalesced=True)


def _per_table(head, wanted, make):
    return head + tuple(make(t) if wanted[t] else None for t in range(len(wanted)))


def _sparse_table_grads(head, wanted, group, width_of, dtype, inv=None, last_id=None, rows_of=None):
    """The tail of a group's sparse backward on separate tensors: `head` and, for every wanted table t, ONE coalesced
    sparse COO gradient [rows_t, width_of(t)].  inv: the ascending global ids of the compressed gradient, last_id its
    count word; rows_of(t, lo, hi): the values of table t, whose entries are [lo, hi) -- ONE read-back, of the
    num_tables + 1 cuts.  inv None: a batch without lookups, empty gradients and no launch."""
    base = group.row_base
    if inv is None:
        return _per_table(head, wanted, lambda t: _empty_sparse(base[t + 1] - base[t], width_of(t), dtype, group.device))
    cuts = torch.ops.cuembed_pyt.cuembed_grouped_table_cuts(inv, last_id, group.row_base_device, True).tolist()

    def table_grad(t):
        lo, hi = cuts[t], cuts[t + 1]
        return torch.sparse_coo_tensor((inv[lo:hi].to(torch.int64) - base[t]).unsqueeze(0), rows_of(t, lo, hi),
                                       size=(base[t + 1] - base[t], width_of(t)), is_coalesced=True)
    return _per_table(head, wanted, table_grad)


class _CuEmbGrouped(torch.autograd.Function):
    """cuemb_embedding_grouped_trainable: the grouped forward, and the backward of all tables through one sort and one
    scatter-add.  `params` is (group.flat,) for a one-storage group, else the group's tables."""

    @staticmethod
    def forward(ctx, group, idx, offsets, weights, sparse_grad, row_loads, sample_order, mode, weight_grad, *params):
        ctx.save_for_backward(idx, offsets, weights)
        ctx.group = group
        ctx.sparse_grad = sparse_grad
        ctx.mode = mode
        ctx.weight_grad = weight_grad
        tables = [t.detach() for t in group.tables]
        w = None if weights is None else weights.detach()
        return torch.ops.cuembed_pyt.cuemb_embedding_grouped(tables, group.table_ptrs, idx, offsets, w, mode,
                                                             _ops._ROW_LOADS[row_loads], sample_order)

    @staticmethod
    def backward(ctx, out_grad):
        idx, offsets, weights = ctx.saved_tensors
        group, kind = ctx.group, ctx.sparse_grad
        T, width, total, base = group.num_tables, group.width, group.total_rows, group.row_base
        one_storage = group.flat is not None
        wanted = ctx.needs_input_grad[9:]
        batch, hot = _grouped_batch(T, idx, offsets)
        nnz = idx.numel()
        dev, dtype = out_grad.device, out_grad.dtype
        out_grad = out_grad.contiguous()
        w_grad = None
        if ctx.weight_grad and ctx.needs_input_grad[3]:     # (sum pooling: the entry point refuses the mean)
            w_grad = torch.ops.cuembed_pyt.cuembed_grouped_weight_grad([t.detach() for t in group.tables],
                                                                       group.table_ptrs, idx, offsets, out_grad)
            if weights.numel() == nnz:
                w_grad = w_grad.view(weights.shape)
            else:                                           # (more weights than lookups: the spare ones took no part)
                spare = torch.zeros(weights.shape, dtype=dtype, device=dev)
                spare.view(-1)[:nnz] = w_grad.view(-1)
                w_grad = spare
        head = (None, None, None, w_grad) + (None,) * 5
        if not any(wanted):
            return head + (None,) * len(wanted)
        if ctx.mode == "mean" and nnz > 0:
            out_grad = torch.ops.cuembed_pyt.cuembed_grouped_mean_scale(
                out_grad, offsets, None if weights is None else weights.detach(), T, hot)
        grad_2d = out_grad.view(batch * T, width)

        def dense_views(dense):
            return head + (dense,) if one_storage else _per_table(head, wanted, lambda t: dense[base[t]:base[t + 1]])

        if nnz == 0:
            if kind is False:
                return dense_views(torch.zeros((total, width), dtype=dtype, device=dev))
            if one_storage:
                return head + (_empty_sparse(total, width, dtype, dev),)
            return _sparse_table_grads(head, wanted, group, lambda t: width, dtype)
        # ---- one key launch, one sort, (one remap,) one scatter-add for all tables
        keys, sample_ids = torch.ops.cuembed_pyt.cuembed_grouped_backward_keys(idx, offsets, group.row_base_device, T,
                                                                               batch, hot, total < 2 ** 31)
        w = None if weights is None else weights.detach().reshape(-1)
        t_keys, t_sids, t_w = cuembed_transpose_sample_ids(sample_ids, keys, w, total)
        t_w = t_w if t_w.numel() else None
        if kind is False:
            return dense_views(cuembed_embedding_backward(grad_2d, total, t_keys, t_sids, t_w))
        remap = torch.ops.cuembed_pyt.cuembed_compute_compressed_grad_indices(t_keys)
        if one_storage and kind is True:      # the count is read back once, after everything is enqueued
            num_unique = int(remap[-1].item()) + 1
            rows, inv = torch.ops.cuembed_pyt.cuembed_embedding_backward_compressed(grad_2d, num_unique, t_keys, t_sids,
                                                                                    remap, t_w)
            return head + (torch.sparse_coo_tensor(inv.to(torch.int64).unsqueeze(0), rows, size=(total, width),
                                                   is_coalesced=True),)
        capacity = min(nnz, total)
        rows = torch.empty((capacity, width), dtype=dtype, device=dev)
        inv = torch.empty((capacity,), dtype=t_keys.dtype, device=dev)
        _ops.embedding_backward(grad_2d, None, t_keys, t_sids, remap, t_w, grad_embedding=rows, inverse_mapping=inv,
                                pad_to_capacity=one_storage)
        if one_storage:                        # "padded": nothing is read back, the step can be captured
            return head + (torch.sparse_coo_tensor(inv.to(torch.int64).unsqueeze(0), rows, size=(total, width),
                                                   is_coalesced=False),)
        # separate tensors, sparse: ONE read-back, of the num_tables + 1 cuts
        return _sparse_table_grads(head, wanted, group, lambda t: width, dtype, inv, remap[-1:],
                                   lambda t, lo, hi: rows[lo:hi])


def _check_grouped_training(mode, weight_grad):
    if mode not in ("sum", "mean"):
        raise ValueError("mode must be 'sum' or 'mean', got %r: a trained group has no other pooling" % (mode,))
    if not isinstance(weight_grad, bool):
        raise ValueError("weight_grad must be True or False, got %r" % (weight_grad,))


def cuemb_embedding_grouped_trainable(group, idx, offsets=None, weights=None, sparse_grad=False, row_loads=None,
                                      sample_order=None, mode="sum", weight_grad=False):
    """cuemb_embedding_grouped (sum or mean pooling, [batch, num_tables, width]) on a cuembed_amd.TableGroup that is TRAINED: the
    forward is the grouped op, the backward runs ONE key launch, ONE sort and ONE scatter-add for all tables
    (cuembed_amd.grouped_backward) instead of one single-table chain per table.  A Python autograd.Function over the
    torch ops cuembed_grouped_backward_keys / cuembed_grouped_table_cuts and the single-table pipeline's.

    A one-storage group (TableGroup.allocate / from_flat; group.flat requires grad) is differentiated with respect to
    group.flat, which gets ONE gradient with global row ids:
        sparse_grad=False      a dense [total_rows, width] gradient;
        sparse_grad=True       a COALESCED sparse COO tensor of exactly the distinct rows (the count is read back once);
        sparse_grad="padded"   padded to min(lookups, total_rows) entries (is_coalesced=False) as in cuemb_embedding:
                               nothing is read back, the step can be captured into a HIP graph.
    A group of separate tensors: every table that requires grad gets its own gradient, the others none:
        sparse_grad=False      dense views of one [total_rows, width] buffer;
        sparse_grad=True       one coalesced sparse COO tensor per table, after ONE read-back of the table cuts;
        sparse_grad="padded"   ValueError: the tables' segments have no fixed size.
    mode="mean" pools with the mean (nn.EmbeddingBag's default; with weights, the sum divided by the bag's summed
    weights, as the grouped forward does): the backward multiplies out_grad by each bag's mean factor in ONE more launch
    (cuembed_grouped_mean_scale) and runs the same chain; every sparse_grad form works as for the sum.
    weight_grad=True also differentiates a SUM with respect to `weights` where they require grad -- nn.EmbeddingBag's
    per_sample_weights gradient, in ONE launch for all tables (cuembed_grouped_weight_grad) -- even when no table
    requires grad.  It is opt-in: it reads every looked-up row a second time in the backward.  By default the weight
    gradient is not taken (weights.requires_grad raises).  The weight gradient of a weighted MEAN needs the forward's
    output and is not provided: mode="mean" with weight_grad=True and weights that require grad raises.
    With grad mode off, or nothing requiring grad, the call is just the forward."""
    if not (sparse_grad is False or sparse_grad is True or sparse_grad == "padded"):
        raise ValueError("sparse_grad must be False, True or 'padded', got %r" % (sparse_grad,))
    _check_grouped_training(mode, weight_grad)
    if group.quantized:
        raise TypeError("a group of fused 8-bit tables is inference only: cuemb_embedding_quantized_grouped")
    weights_need_grad = weights is not None and weights.requires_grad
    if weights_need_grad and not weight_grad:
        raise ValueError("the grouped backward does not take the weight gradient: detach the weights, or pass "
                         "weight_grad=True (sum pooling only: one more pass over the looked-up rows)")
    if weights_need_grad and mode == "mean":
        raise ValueError("the weight gradient of a weighted mean, (<x_j, g> - <y, g>) / S, needs the forward's output and "
                         "is not provided: weight_grad=True takes mode='sum' only; detach the weights")
    one_storage = group.flat is not None
    if sparse_grad == "padded" and not one_storage:
        raise ValueError("sparse_grad='padded' needs a one-storage group (TableGroup.allocate / from_flat): the "
                         "per-table segments of a compressed gradient have no fixed size")
    params = (group.flat,) if one_storage else tuple(group.tables)
    if not torch.is_grad_enabled() or not (any(p.requires_grad for p in params) or weights_need_grad):
        return torch.ops.cuembed_pyt.cuemb_embedding_grouped([t.detach() for t in group.tables], group.table_ptrs, idx,
                                                             offsets, None if weights is None else weights.detach(),
                                                             mode, _ops._ROW_LOADS[row_loads], sample_order)
    return _CuEmbGrouped.apply(group, idx, offsets, weights, sparse_grad, row_loads, sample_order, mode, weight_grad,
                               *params)


class TrainableEmbeddingBagGroup(torch.nn.Module):
    """A TableGroup that is trained, with EmbeddingBagGroup's call shape (mode "sum" or "mean"): bags(idx, offsets,
    weights) with CSR offsets, or bags(idx) with idx [num_tables, batch, hotness]; returns [batch, num_tables, width] and
    differentiates through cuemb_embedding_grouped_trainable.  parameters() yields group.flat of a one-storage group,
    else the tables, where they are nn.Parameters.  weight_grad=True (sum pooling) also gives weights that require grad
    their gradient."""

    def __init__(self, group, sparse_grad=False, mode="sum", weight_grad=False):
        super().__init__()
        if not (sparse_grad is False or sparse_grad is True or sparse_grad == "padded"):
            raise ValueError("sparse_grad must be False, True or 'padded', got %r" % (sparse_grad,))
        _check_grouped_training(mode, weight_grad)
        if group.quantized:
            raise TypeError("a group of fused 8-bit tables is inference only")
        if sparse_grad == "padded" and group.flat is None:
            raise ValueError("sparse_grad='padded' needs a one-storage group (TableGroup.allocate / from_flat)")
        self.group = group
        self.sparse_grad = sparse_grad
        self.mode = mode
        self.weight_grad = weight_grad
        if isinstance(group.flat, torch.nn.Parameter):
            self.weight = group.flat
        elif group.flat is None:
            self.tables = torch.nn.ParameterList([t for t in group.tables if isinstance(t, torch.nn.Parameter)])

    @property
    def num_tables(self):
        return self.group.num_tables

    @property
    def embedding_dim(self):
        return self.group.width

    def forward(self, idx, offsets=None, weights=None, sample_order=None):
        return cuemb_embedding_grouped_trainable(self.group, idx, offsets, weights, sparse_grad=self.sparse_grad,
                                                 sample_order=sample_order, mode=self.mode, weight_grad=self.weight_grad)


class _CuEmbMixedGroup(torch.autograd.Function):
    """cuemb_embedding_mixed_group_trainable: the mixed-width forward, and the backward of all tables through one sort and
    one scatter-add for all widths.  `params` are the group's tables."""

    @staticmethod
    def forward(ctx, group, idx, offsets, weights, mode, *params):
        ctx.save_for_backward(idx, offsets, weights)
        ctx.group = group
        ctx.mode = mode
        batch, _ = _grouped_batch(group.num_tables, idx, offsets)
        lane = group.lane_bytes()          # (the op's result is a fresh, 16-byte aligned tensor)
        return torch.ops.cuembed_pyt.cuemb_embedding_mixed_group(
            [t.detach() for t in group.tables], group.table_ptrs, group.descriptor(batch, lane), lane, idx, offsets,
            None if weights is None else weights.detach(), mode, -1)

    @staticmethod
    def backward(ctx, out_grad):
        idx, offsets, weights = ctx.saved_tensors
        group = ctx.group
        T, total, widths = group.num_tables, group.total_rows, group.widths
        wanted = ctx.needs_input_grad[5:]
        head = (None,) * 5
        if not any(wanted):
            return head + (None,) * T
        batch, hot = _grouped_batch(T, idx, offsets)
        nnz = idx.numel()
        dtype = out_grad.dtype
        out_grad = out_grad.contiguous()
        if nnz == 0:
            return _sparse_table_grads(head, wanted, group, widths.__getitem__, dtype)
        w = None if weights is None else weights.detach()
        if ctx.mode == "mean":
            out_grad = torch.ops.cuembed_pyt.cuembed_mixed_group_mean_scale(out_grad, list(widths),
                                                                            group.table_columns_device, offsets, w, hot)
        # ---- one key launch, one sort, one remap, one scatter-add for all tables and widths
        keys, sample_ids = torch.ops.cuembed_pyt.cuembed_grouped_backward_keys(idx, offsets, group.row_base_device, T,
                                                                               batch, hot, total < 2 ** 31)
        t_keys, t_sids, t_w = cuembed_transpose_sample_ids(sample_ids, keys, None if w is None else w.reshape(-1), total)
        remap = torch.ops.cuembed_pyt.cuembed_compute_compressed_grad_indices(t_keys)
        rows, inv, _ = torch.ops.cuembed_pyt.cuembed_embedding_backward_mixed_group(
            out_grad, list(widths), group.table_columns_device, t_keys, t_sids, remap, t_w if t_w.numel() else None,
            min(nnz, total))
        # ONE read-back, of the num_tables + 1 cuts
        return _sparse_table_grads(head, wanted, group, widths.__getitem__, dtype, inv, remap[-1:],
                                   lambda t, lo, hi: rows[lo:hi, :widths[t]].contiguous())


def cuemb_embedding_mixed_group_trainable(group_or_tables, idx, offsets=None, weights=None, num_hots=0, mode="sum"):
    """cuemb_embedding_mixed_group (sum or mean pooling, [batch, sum of the widths]) on a cuembed_amd.MixedTableGroup --
    or a list of tables, from which one is built -- that is TRAINED: the forward is the mixed-width op, the backward runs
    ONE key launch, ONE sort and ONE scatter-add for all tables and widths (cuembed_amd.mixed_group_backward) instead of
    one single-table chain per table on a column slice of out_grad.  A Python autograd.Function over the torch ops
    cuembed_grouped_backward_keys, cuembed_embedding_backward_mixed_group, cuembed_mixed_group_mean_scale and
    cuembed_grouped_table_cuts.

    Every table that requires grad gets a COALESCED sparse COO gradient [rows_t, W_t] of exactly its looked-up rows,
    after ONE read-back (the num_tables + 1 table cuts); its values are made contiguous per table (the compressed
    gradient is padded to the widest table).  CSR with `offsets` (num_tables * batch + 1 entries), or fixed hotness with
    idx [num_tables, batch, hotness] (num_hots, if given, must then agree).  mode="mean" as in
    cuemb_embedding_grouped_trainable.  There is no weight gradient: weights that require grad raise.  With grad mode
    off, or no table requiring grad, the call is just the forward."""
    from . import mixed_group as _m
    if mode not in ("sum", "mean"):
        raise ValueError("mode must be 'sum' or 'mean', got %r: a trained group has no other pooling" % (mode,))
    group = _m._as_mixed_group(group_or_tables)
    if weights is not None and weights.requires_grad:
        raise ValueError("the mixed-width backward does not take the weight gradient: detach the weights")
    if offsets is None and num_hots and (idx.dim() != 3 or idx.shape[2] != num_hots):
        raise ValueError("without offsets, idx must be [num_tables, batch, num_hots = %d]" % num_hots)
    if offsets is not None and num_hots:
        raise ValueError("either CSR (offsets given, num_hots == 0) or fixed hotness (offsets None)")
    if not torch.is_grad_enabled() or not any(t.requires_grad for t in group.tables):
        with torch.no_grad():
            return cuemb_embedding_mixed_group(group, idx, offsets, None if weights is None else weights.detach(), mode)
    return _CuEmbMixedGroup.apply(group, idx, offsets, weights, mode, *group.tables)


class TrainableMixedEmbeddingBagGroup(torch.nn.Module):
    """A MixedTableGroup that is trained, with MixedEmbeddingBagGroup's call shape (mode "sum" or "mean"): bags(idx,
    offsets, weights) with CSR offsets, or bags(idx) with idx [num_tables, batch, hotness]; returns [batch, sum of the
    widths] and differentiates through cuemb_embedding_mixed_group_trainable: every table that is an nn.Parameter gets a
    coalesced sparse gradient.  parameters() yields those tables."""

    def __init__(self, tables, mode="sum"):
        super().__init__()
        from . import mixed_group as _m
        if mode not in ("sum", "mean"):
            raise ValueError("mode must be 'sum' or 'mean'")
        self.group = _m._as_mixed_group(tables)
        self.mode = mode
        self.tables = torch.nn.ParameterList([t for t in self.group.tables if isinstance(t, torch.nn.Parameter)])

    @property
    def num_tables(self):
        return self.group.num_tables

    @property
    def embedding_dim(self):
        return self.group.embedding_dim

    def forward(self, idx, offsets=None, weights=None):
        return cuemb_embedding_mixed_group_trainable(self.group, idx, offsets, weights, mode=self.mode)


def cuembed_forward(params, idx, offsets, weights, hints=None):
    if hints is None:
        return cuembed_embedding_forward(params, idx, offsets, weights, mode="sum")
    return torch.ops.cuembed_pyt.cuembed_embedding_forward_hinted(params, idx, offsets, weights, "sum", hints[0], hints[1],
                                                                  hints[2] if len(hints) > 2 else None)


def _auto_hints(params, idx, offsets):
    """(row_loads, sample_order, row_loads_device) chosen by cuembed_amd.policy for this table and this batch -- both
    decided on the device, no read-back; never changes a result."""
    return -1, _policy.sample_order(offsets, idx.numel()), _policy.row_loads_device(params, idx)


def _narrow_for_index_work(idx, offsets, num_categories):
    """The reference's binding takes int64 indices (cuembed_embedding.cu:18-23).  When the table has fewer
    than 2^31 rows and the batch fewer than 2^31 lookups, the index work of the backward (row ids, radix
    sort, remap, scatter-add) runs on int32 copies: half the bytes through every sorting pass
    (C4 step 0.624 -> 0.597 ms for one 17 MB conversion; small batches are launch-bound and the two extra
    conversion launches cost more than they save -- B = 1024: 0.199 -> 0.228 ms -- hence the size gate)."""
    if idx.dtype == torch.int64 and num_categories < 2 ** 31 and (1 << 18) <= idx.numel() < 2 ** 31:
        return idx.to(torch.int32), (None if offsets is None else offsets.to(torch.int32))
    if offsets is not None and offsets.dtype != idx.dtype:
        # the forward takes indices and offsets of different integer types; the index work has ONE type for lookups and
        # sample ids, the one of the indices (offsets hold values <= nnz, which fits it)
        offsets = offsets.to(idx.dtype)
    return idx, offsets


def cuembed_backward(ctx, out_grad):
    idx, offsets, weights = ctx.saved_tensors
    nnz = idx.size(0)
    idx, offsets = _narrow_for_index_work(idx, offsets, ctx.num_categories)
    if getattr(ctx, "sparse_grad", False):
        return _sparse_backward(ctx, out_grad, idx, offsets, weights, nnz)
    # equivalent of nn.EmbeddingBag(include_last_offset=True).  (The reference slices offsets[:-1] for its
    # op, cuembed_pyt.py:23; the saved tensor already has the closing entry, so no copy is needed.)
    sample_ids = torch.ops.cuembed_pyt.cuembed_extract_row_ids_from_offsets(offsets, nnz)
    transpose_indices, transpose_sample_ids, transpose_weights = cuembed_transpose_sample_ids(
        sample_ids, idx, weights, ctx.num_categories)
    if transpose_weights.numel() == 0:  # forward ran without weights
        transpose_weights = None
    grad_embedding = cuembed_embedding_backward(out_grad, ctx.num_categories, transpose_indices,
                                                transpose_sample_ids, transpose_weights)
    return grad_embedding, None, None, None  # no grad for indices, offsets or weights


def _sparse_backward(ctx, out_grad, idx, offsets, weights, nnz):
    """Compressed gradient as a sparse COO tensor (like nn.EmbeddingBag(sparse=True)); True / "reference" / "blocked":
    coalesced, exactly num_unique ascending rows.  Reads num_unique back to the host (one sync), exactly like the
    reference's benchmark does (manual_benchmark.cu:392-394) -- except "padded", which never does."""
    width = out_grad.size(1)
    if weights is not None and weights.numel() != nnz:
        raise ValueError("weights must have one entry per index")
    if nnz == 0:
        return (torch.sparse_coo_tensor(torch.empty((1, 0), dtype=torch.int64, device=out_grad.device),
                                        torch.empty((0, width), dtype=out_grad.dtype, device=out_grad.device),
                                        size=(ctx.num_categories, width)), None, None, None)
    sample_ids = torch.ops.cuembed_pyt.cuembed_extract_row_ids_from_offsets(offsets, nnz)
    blocks = 1
    if ctx.sparse_grad == "padded":
        # min(lookups, rows) entries, the tail zero rows naming rows of the batch in turn: no read-back at any size
        t_idx, t_sid, t_w = cuembed_transpose_sample_ids(sample_ids, idx, weights, ctx.num_categories)
        remap = torch.ops.cuembed_pyt.cuembed_compute_compressed_grad_indices(t_idx)
        capacity = min(nnz, ctx.num_categories)
        rows = torch.empty((capacity, width), dtype=out_grad.dtype, device=out_grad.device)
        inv = torch.empty((capacity,), dtype=t_idx.dtype, device=out_grad.device)
        _ops.embedding_backward(out_grad.contiguous(), None, t_idx, t_sid, remap, t_w if t_w.numel() else None,
                                grad_embedding=rows, inverse_mapping=inv, pad_to_capacity=True)
        grad = torch.sparse_coo_tensor(inv.to(torch.int64).unsqueeze(0), rows, size=(ctx.num_categories, width),
                                       is_coalesced=False)
        return grad, None, None, None
    if ctx.sparse_grad not in (True, "reference"):
        # while a block of samples is scattered every L2 gathers from 1 / blocks of out_grad only
        blocks = _ops.recommended_sample_blocks(out_grad.dtype, width, out_grad.size(0), nnz)
        if ctx.sparse_grad == "blocked":
            # "blocked" promises the COALESCED tensor: never fall through to the uncoalesced path because the
            # recommendation (up to 64 blocks for very wide rows) exceeds what the coalescing remap handles
            blocks = min(blocks, _ops.MAX_COALESCED_BLOCKS)
    if blocks > 1 and ctx.sparse_grad == "blocked":
        # the COALESCED gradient from the blocked order: the same rows and ids as the fully sorted order gives
        # (ComputeCompressedGradIndicesBlocked + EmbeddingBackward(sample_blocks); EmbeddingBackward at C4 0.257 -> 0.232 ms)
        t_idx, t_sid, t_w = torch.ops.cuembed_pyt.cuembed_transpose_sample_blocks(sample_ids, idx, weights,
                                                                                  ctx.num_categories, blocks)
        if t_w.numel() == 0:
            t_w = None
        pairs, pair_rows, count = _ops.compute_compressed_grad_indices_blocked(t_idx, blocks)
        num_unique = int(count.item())
        rows, inv = _ops.embedding_backward(out_grad.contiguous(), num_unique, t_idx, t_sid, pairs, t_w,
                                            sample_blocks=blocks, block_row_ids=pair_rows)
        grad = torch.sparse_coo_tensor(inv.to(torch.int64).unsqueeze(0), rows, size=(ctx.num_categories, width),
                                       is_coalesced=True)
        return grad, None, None, None
    if blocks > 1:
        # one gradient row per (block of samples, table row): the fastest backward (C4: 0.257 -> 0.185 ms)
        t_idx, t_sid, t_w = torch.ops.cuembed_pyt.cuembed_transpose_sample_blocks(sample_ids, idx, weights,
                                                                                  ctx.num_categories, blocks)
    else:
        t_idx, t_sid, t_w = cuembed_transpose_sample_ids(sample_ids, idx, weights, ctx.num_categories)
    if t_w.numel() == 0:
        t_w = None
    remap = torch.ops.cuembed_pyt.cuembed_compute_compressed_grad_indices(t_idx)
    num_unique = int(remap[-1].item()) + 1
    rows, inv = torch.ops.cuembed_pyt.cuembed_embedding_backward_compressed(out_grad, num_unique, t_idx, t_sid,
                                                                            remap, t_w)
    grad = torch.sparse_coo_tensor(inv.to(torch.int64).unsqueeze(0), rows, size=(ctx.num_categories, width),
                                   is_coalesced=blocks == 1)
    return grad, None, None, None


class _CuEmbEmbedding(torch.autograd.Function):
    @staticmethod
    def forward(ctx, params, idx, offsets, weights=None, sparse_grad=False, hints=None):
        ctx.save_for_backward(idx, offsets, weights)
        ctx.num_categories = params.size(0)
        ctx.sparse_grad = sparse_grad
        # the weight gradient (an extension; the reference returns None) needs the table rows
        ctx.params_for_weight_grad = params.detach() if (weights is not None and weights.requires_grad) else None
        return cuembed_forward(params, idx, offsets, weights, hints)

    @staticmethod
    def backward(ctx, out_grad):
        if ctx.needs_input_grad[0]:
            grads = list(cuembed_backward(ctx, out_grad))
        else:
            grads = [None, None, None, None]
        if ctx.params_for_weight_grad is not None:
            idx, offsets, _ = ctx.saved_tensors
            grads[3] = torch.ops.cuembed_pyt.cuembed_embedding_weight_grad(
                ctx.params_for_weight_grad, idx, offsets, out_grad.to(ctx.params_for_weight_grad.dtype))
        return tuple(grads) + (None, None)


# (native CuEmbEmbeddingNode: GradKind)
_GRAD_KINDS = {False: 0, True: 2, "reference": 2, "fastest": 1, "uncoalesced": 3, "padded": 4}
_SPARSE_KINDS = (False, True, "reference", "fastest", "uncoalesced", "padded", "blocked")


def cuemb_embedding(params, idx, offsets, weights=None, sparse_grad=False, hints="auto"):
    """Sum-pooled embedding bag (offsets include the last offset), the reference's entry point
    (examples/pytorch/cuembed_pyt.py:48-51).  Differentiable w.r.t. params and -- an extension over the reference --
    w.r.t. the per-lookup weights.

    sparse_grad (extension; False = the reference's dense, table-sized gradient).  Every sparse kind densifies to the
    same gradient; they differ in which entries the COO tensor holds:
      True           params.grad is a COALESCED sparse COO tensor holding exactly the rows that were looked up, ascending
                     (grad._nnz() == number of distinct rows; grad.indices() / .values() work) -- the reference's fully
                     sorted order, on either backend and under torch.compile alike.  The row count is read back once
                     per step (after everything is enqueued), so the step cannot be captured into a HIP graph;
      "reference"    the same, by its older name;
      "blocked"      the same coalesced tensor computed from the sample-blocked order (a faster EmbeddingBackward for
                     more index work; through this op surface the two cancel at C4);
      "uncoalesced"  where the backward gains from scattering the batch in blocks of samples (C4: 0.56 -> 0.49 ms per
                     step) a row may appear once per block (is_coalesced=False; what torch.sparse consumers -- SGD,
                     SparseAdam, .coalesce(), .to_dense() -- take as it is); exactly one entry per (block, row);
      "padded"       one block, PADDED to min(lookups, rows) entries (zero rows naming rows of the batch in turn;
                     is_coalesced=False): the step never waits for the device and can be captured into a HIP graph --
                     the entry count of torch's own EmbeddingBag(sparse=True) gradient; a consumer that pays per entry
                     (torch.optim.SGD) is better served by True;
      "fastest"      whichever of the above is fastest for the shape (native backend: "padded" while the worst case
                     fits 64 MiB, else "uncoalesced"); the entry count is an implementation detail -- consume it with
                     .coalesce(), .to_dense() or an optimizer.
    hints="auto" lets cuembed_amd.policy pick the forward's scheduling options for this table and batch (non-temporal
    row loads, bag order); None = the library defaults.  Results never depend on hints.

    Outside torch.compile the step runs as ONE native autograd node (forward, and row ids -> transpose + remap ->
    scatter-add in the backward, one dispatcher hop each; libcuembed_pyt.so: CuEmbEmbeddingNode); under torch.compile,
    for the weight gradient and for "blocked" it runs as a Python autograd.Function over the same ops."""
    if not (isinstance(sparse_grad, bool) or (isinstance(sparse_grad, str) and sparse_grad in _SPARSE_KINDS)):
        raise ValueError("sparse_grad must be one of %r" % (_SPARSE_KINDS,))
    needs_grad = params.requires_grad or (weights is not None and weights.requires_grad)
    quiet = torch.compiler.is_compiling()
    chosen = _auto_hints(params, idx, offsets) if (hints == "auto" and not quiet) else None
    if chosen is not None and chosen[0] < 0 and chosen[1] is None and chosen[2] is None:
        chosen = None
    if not torch.is_grad_enabled() or not needs_grad:
        return cuembed_forward(params, idx, offsets, weights, chosen)
    native = (BACKEND == "native" and not quiet and sparse_grad in _GRAD_KINDS and
              not (weights is not None and weights.requires_grad))
    if native:
        row_loads, order, decision = chosen if chosen is not None else (-1, None, None)
        return torch.ops.cuembed_pyt.cuemb_embedding_step(params, idx, offsets, weights, _GRAD_KINDS[sparse_grad],
                                                          row_loads, order, decision)
    return _CuEmbEmbedding.apply(params, idx, offsets, weights, sparse_grad, chosen)


class _CuEmbFixed(torch.autograd.Function):
    """Fixed-hotness lookup: indices [B, H]; mode sum / mean -> [B, W], concat -> [B, H, W]."""

    @staticmethod
    def forward(ctx, params, idx, weights, mode):
        ctx.save_for_backward(idx, weights)
        ctx.num_categories = params.size(0)
        ctx.mode = mode
        return torch.ops.cuembed_pyt.cuembed_embedding_forward_fixed(params, idx, weights, mode)

    @staticmethod
    def backward(ctx, out_grad):
        idx, weights = ctx.saved_tensors
        batch, hot = idx.shape
        idx, _ = _narrow_for_index_work(idx, None, ctx.num_categories)
        if ctx.mode == "concat":   # every lookup has its own gradient row: sample id = position
            y = out_grad.reshape(batch * hot, -1)
            layout = idx.contiguous().view(batch * hot, 1)
        else:
            y = out_grad if ctx.mode == "sum" else out_grad * (1.0 / hot)
            layout = idx
        if ctx.mode == "mean" and weights is not None:      # out = sum(w x) / sum(w)
            y = out_grad / weights.sum(1, keepdim=True).to(out_grad.dtype)
        # row ids + transpose in one call; the sample ids are never materialised
        t_idx, t_sid, t_w, _ = cuembed_transpose_fixed_hotness(layout, weights, ctx.num_categories, False)
        if t_w.numel() == 0:
            t_w = None
        grad = cuembed_embedding_backward(y.contiguous(), ctx.num_categories, t_idx, t_sid, t_w)
        return grad, None, None, None


def cuemb_embedding_fixed(params, idx, weights=None, mode="sum"):
    """Fixed-hotness lookup (this library's extension of the reference's Python surface):
    idx is [batch, hotness]; weights (optional, sum/mean only) has the same shape."""
    if not torch.is_grad_enabled() or not params.requires_grad:
        return torch.ops.cuembed_pyt.cuembed_embedding_forward_fixed(params, idx, weights, mode)
    return _CuEmbFixed.apply(params, idx, weights, mode)


# Shape functions so that torch.compile can trace through the ops without running them.
@torch.library.register_fake("cuembed_pyt::cuembed_embedding_forward_fixed")
def _(params, indices, weights=None, mode="sum"):
    b, h = indices.shape
    shape = (b, h, params.shape[1]) if mode == "concat" else (b, params.shape[1])
    return torch.empty(shape, device=params.device, dtype=params.dtype)


@torch.library.register_fake("cuembed_pyt::cuembed_extract_row_ids_from_csr")
def _(offsets, nnz):
    return torch.empty((nnz,), device=offsets.device, dtype=offsets.dtype)


@torch.library.register_fake("cuembed_pyt::cuembed_extract_row_ids_from_offsets")
def _(offsets, nnz):
    return torch.empty((nnz,), device=offsets.device, dtype=offsets.dtype)


@torch.library.register_fake("cuembed_pyt::cuembed_transpose")
def _(rows, cols, weights=None):
    n = 0 if weights is None else cols.shape[0]
    return (torch.empty_like(cols), torch.empty_like(rows),
            torch.empty((n,), device=rows.device, dtype=torch.float32 if weights is None else weights.dtype))


@torch.library.register_fake("cuembed_pyt::cuembed_embedding_weight_grad")
def _(params, indices, offsets, y_grad):
    return torch.empty((indices.shape[0],), device=params.device, dtype=params.dtype)


@torch.library.register_fake("cuembed_pyt::cuembed_transpose_bounded")
def _(rows, cols, weights=None, num_categories=0):
    n = 0 if weights is None else cols.shape[0]
    return (torch.empty_like(cols), torch.empty_like(rows),
            torch.empty((n,), device=rows.device, dtype=torch.float32 if weights is None else weights.dtype))


@torch.library.register_fake("cuembed_pyt::cuembed_transpose_sample_ids")
def _(sample_ids, indices, weights=None, num_categories=0):
    n = 0 if weights is None else indices.shape[0]
    return (torch.empty_like(indices), torch.empty_like(sample_ids),
            torch.empty((n,), device=indices.device, dtype=torch.float32 if weights is None else weights.dtype))


@torch.library.register_fake("cuembed_pyt::cuembed_transpose_sample_blocks")
def _(sample_ids, indices, weights=None, num_categories=0, sample_blocks=1):
    n = 0 if weights is None else indices.shape[0]
    return (torch.empty_like(indices), torch.empty_like(sample_ids),
            torch.empty((n,), device=indices.device, dtype=torch.float32 if weights is None else weights.dtype))


@torch.library.register_fake("cuembed_pyt::cuembed_transpose_fixed_hotness")
def _(indices, weights=None, num_categories=0, compressed=False):
    nnz = indices.shape[0] * indices.shape[1]
    flat = dict(device=indices.device, dtype=indices.dtype)
    return (torch.empty((nnz,), **flat), torch.empty((nnz,), **flat),
            torch.empty((0 if weights is None else nnz,), device=indices.device,
                        dtype=torch.float32 if weights is None else weights.dtype),
            torch.empty((nnz if compressed else 0,), **flat))


@torch.library.register_fake("cuembed_pyt::cuembed_compute_compressed_grad_indices")
def _(transpose_indices):
    return torch.empty_like(transpose_indices)


@torch.library.register_fake("cuembed_pyt::cuembed_embedding_backward_compressed")
def _(y_grad, num_unique, transpose_indices, transpose_sample_ids, transpose_remapped_indices, transpose_weights=None):
    return (torch.empty((num_unique, y_grad.shape[1]), device=y_grad.device, dtype=y_grad.dtype),
            torch.empty((num_unique,), device=y_grad.device, dtype=transpose_indices.dtype))


@torch.library.register_fake("cuembed_pyt::cuembed_embedding_forward")
def _(params, idx, offsets, weights=None, mode="sum"):
    return torch.empty((offsets.shape[0] - 1, params.shape[1]), device=params.device, dtype=params.dtype)


@torch.library.register_fake("cuembed_pyt::cuembed_decide_row_loads")
def _(indices, table_bytes, decision):
    return None


@torch.library.register_fake("cuembed_pyt::cuembed_sparse_row_update_")
def _(table, state, ids, rows, rule, lr, eps, lr_device=None, count=-1, counts=None, last_id=None, piece_rows=0,
      stochastic_rounding=False, seed=0, step=0, step_device=None):
    return None


@torch.library.register_fake("cuembed_pyt::cuembed_sparse_row_adam_")
def _(table, exp_avg, exp_avg_sq, ids, rows, rowwise, lr, bias_factor, beta1, beta2, eps, weight_decay, lr_device=None,
      bias_factor_device=None, count=-1, counts=None, last_id=None, piece_rows=0, stochastic_rounding=False, seed=0,
      step=0, step_device=None):
    return None


@torch.library.register_fake("cuembed_pyt::cuembed_sparse_row_update_grouped")
def _(tables, table_ptrs, states, state_ptrs, row_base, ids, rows, rule, lr, eps, lr_device=None, count=-1,
      count_word=None, last_id=None, stochastic_rounding=False, seeds=None, step=0, step_device=None):
    return None


@torch.library.register_fake("cuembed_pyt::cuembed_sparse_row_adam_grouped")
def _(tables, table_ptrs, exp_avg, exp_avg_ptrs, exp_avg_sq, exp_avg_sq_ptrs, row_base, ids, rows, rowwise, lr,
      bias_factor, beta1, beta2, eps, weight_decay, lr_device=None, bias_factor_device=None, count=-1, count_word=None,
      last_id=None, stochastic_rounding=False, seeds=None, step=0, step_device=None):
    return None


@torch.library.register_fake("cuembed_pyt::quantize_rows")
def _(table):
    return torch.empty((table.shape[0], table.shape[1] + 8), device=table.device, dtype=torch.uint8)


@torch.library.register_fake("cuembed_pyt::dequantize_rows")
def _(qtable, ids=None, dtype=torch.float32):
    lead = (qtable.shape[0],) if ids is None else tuple(ids.shape)
    return torch.empty(lead + (qtable.shape[1] - 8,), device=qtable.device, dtype=dtype)


@torch.library.register_fake("cuembed_pyt::cuemb_embedding_quantized")
def _(qtable, indices, offsets=None, weights=None, mode="sum", out_dtype=torch.float16, row_loads=-1, sample_order=None,
      row_loads_device=None):
    width = qtable.shape[1] - 8
    if offsets is not None:
        shape = (offsets.shape[0] - 1, width)
    elif mode == "concat":
        shape = (indices.shape[0], indices.shape[1], width)
    else:
        shape = (indices.shape[0], width)
    return torch.empty(shape, device=qtable.device, dtype=out_dtype)


def _grouped_fake_shape(tables, idx, offsets, width):
    if offsets is not None:
        return ((offsets.shape[0] - 1) // len(tables), len(tables), width)
    return (idx.shape[1], len(tables), width)


@torch.library.register_fake("cuembed_pyt::cuemb_embedding_grouped")
def _(tables, table_ptrs, idx, offsets=None, weights=None, mode="sum", row_loads=-1, sample_order=None):
    return torch.empty(_grouped_fake_shape(tables, idx, offsets, tables[0].shape[1]), device=tables[0].device,
                       dtype=tables[0].dtype)


@torch.library.register_fake("cuembed_pyt::cuemb_embedding_mixed_group")
def _(tables, table_ptrs, descriptor, lane_bytes, idx, offsets=None, weights=None, mode="sum", row_loads=-1):
    batch = (offsets.shape[0] - 1) // len(tables) if offsets is not None else idx.shape[1]
    return torch.empty((batch, sum(t.shape[1] for t in tables)), device=tables[0].device, dtype=tables[0].dtype)


@torch.library.register_fake("cuembed_pyt::cuemb_embedding_quantized_grouped")
def _(qtables, table_ptrs, idx, offsets=None, weights=None, mode="sum", out_dtype=torch.float16, row_loads=-1,
      sample_order=None):
    return torch.empty(_grouped_fake_shape(qtables, idx, offsets, qtables[0].shape[1] - 8), device=qtables[0].device,
                       dtype=out_dtype)


@torch.library.register_fake("cuembed_pyt::cuembed_grouped_backward_keys")
def _(idx, offsets, row_base, num_tables, batch, num_hots, narrow):
    flat = dict(device=idx.device, dtype=torch.int32 if narrow else torch.int64)
    return torch.empty((idx.numel(),), **flat), torch.empty((idx.numel(),), **flat)


@torch.library.register_fake("cuembed_pyt::cuembed_grouped_table_cuts")
def _(ids, count_word, row_base, last_id=False):
    return torch.empty((row_base.shape[0],), device=ids.device, dtype=torch.int64)


@torch.library.register_fake("cuembed_pyt::cuembed_grouped_weight_grad")
def _(tables, table_ptrs, idx, offsets, y_grad):
    return torch.empty(idx.shape, device=tables[0].device, dtype=tables[0].dtype)


@torch.library.register_fake("cuembed_pyt::cuembed_grouped_mean_scale")
def _(y_grad, offsets, weights, num_tables, hotness):
    return torch.empty(y_grad.shape, device=y_grad.device, dtype=y_grad.dtype)


@torch.library.register_fake("cuembed_pyt::cuembed_embedding_backward_mixed_group")
def _(y_grad, widths, table_columns, transpose_indices, transpose_sample_ids, transpose_remapped_indices,
      transpose_weights, capacity):
    return (torch.empty((capacity, max(widths)), device=y_grad.device, dtype=y_grad.dtype),
            torch.empty((capacity,), device=y_grad.device, dtype=transpose_indices.dtype),
            torch.empty((1,), device=y_grad.device, dtype=torch.int32))


@torch.library.register_fake("cuembed_pyt::cuembed_mixed_group_mean_scale")
def _(y_grad, widths, table_columns, offsets, weights, hotness):
    return torch.empty(y_grad.shape, device=y_grad.device, dtype=y_grad.dtype)


@torch.library.register_fake("cuembed_pyt::cuembed_check_indices")
def _(indices, offsets, row_base, num_rows, num_tables, batch, num_hots, repair=False):
    like = offsets if offsets is not None else indices
    return (torch.empty((4,), device=indices.device, dtype=torch.int64),
            torch.empty(indices.shape if repair else (0,), device=indices.device, dtype=indices.dtype),
            torch.empty(offsets.shape if repair and offsets is not None else (0,), device=like.device, dtype=like.dtype))


@torch.library.register_fake("cuembed_pyt::cuembed_embedding_forward_hinted")
def _(params, idx, offsets, weights=None, mode="sum", row_loads=-1, sample_order=None, row_loads_device=None):
    return torch.empty((offsets.shape[0] - 1, params.shape[1]), device=params.device, dtype=params.dtype)


@torch.library.register_fake("cuembed_pyt::cuembed_bag_order_by_length")
def _(offsets, max_length=0):
    return torch.empty((offsets.shape[0] - 1,), device=offsets.device, dtype=torch.int32)


@torch.library.register_fake("cuembed_pyt::cuembed_embedding_backward")
def _(y_grad, num_categories, transpose_indices, transpose_sample_ids, transpose_weights=None):
    return torch.empty((num_categories, y_grad.shape[1]), device=y_grad.device, dtype=y_grad.dtype)
