// PyTorch-ROCm binding of the embedding-lookup library: the reference's torch library
// `cuembed_pyt` (examples/pytorch/cuembed_embedding.cu:169-190) rebuilt natively.
//
//   TORCH_LIBRARY(cuembed_pyt, m)            the reference's four schemas, verbatim, + extensions
//   TORCH_LIBRARY_IMPL(cuembed_pyt, CUDA, m) HIP tensors dispatch on the CUDA key on ROCm
//
// Every op validates like the reference's binding (AT_ASSERT -> TORCH_CHECK: a Python exception,
// not an abort), makes its inputs contiguous, allocates its outputs with ATen and enqueues the
// HIP kernels on torch's CURRENT stream (c10::hip::getCurrentHIPStream(), the counterpart of
// at::cuda::getCurrentCUDAStream() at cuembed_embedding.cu:49) of the tensors' device.  The
// kernels are reached through the library's C ABI (include/cuembed_amd.h; every entry point is an
// explicit instantiation of the header-only templates), so this translation unit holds no device
// code and builds with the host compiler in seconds.
//
// Relative to the reference binding (fp32 / int64 / sum only, cuembed_embedding.cu:15-32) the
// ops accept fp16 and bf16 tables, int32 indices / offsets and mode = "mean"; the extension ops
// are listed in INTEGRATION.md section 4.
#include <ATen/ATen.h>
#include <ATen/DeviceGuard.h>
#include <c10/hip/HIPGraphsC10Utils.h>
#include <c10/hip/HIPStream.h>
#include <torch/csrc/autograd/custom_function.h>
#include <torch/library.h>

#include <cstdint>
#include <cstdlib>
#include <initializer_list>
#include <string>
#include <tuple>
#include <vector>

#include "cuembed_amd.h"

namespace {

int ElemCode(const at::Tensor& t, const char* what) {
  switch (t.scalar_type()) {
    case at::kFloat: return CUEMBED_F32;
    case at::kHalf: return CUEMBED_F16;
    case at::kBFloat16: return CUEMBED_BF16;
    default: TORCH_CHECK(false, "cuembed_pyt: ", what, " must be float32, float16 or bfloat16");
  }
  return 0;
}

int IndexCode(const at::Tensor& t, const char* what) {
  switch (t.scalar_type()) {
    case at::kInt: return CUEMBED_I32;
    case at::kLong: return CUEMBED_I64;
    default: TORCH_CHECK(false, "cuembed_pyt: ", what, " must be int32 or int64");
  }
  return 0;
}

void CheckGpu(const at::Tensor& t, const char* what) {
  TORCH_CHECK(t.is_cuda(), "cuembed_pyt: ", what, " must be on the GPU (there is no CPU path)");
}

const void* Ptr(const at::Tensor& t) { return t.defined() ? t.data_ptr() : nullptr; }
void* MutPtr(at::Tensor& t) { return t.defined() ? t.data_ptr() : nullptr; }

at::Tensor ContiguousOrUndefined(const at::Tensor& t) { return t.defined() ? t.contiguous() : t; }

cuembed_stream_t CurrentStream(const at::Tensor& t) {
  return static_cast<cuembed_stream_t>(c10::hip::getCurrentHIPStream(t.device().index()).stream());
}

int Mode(const std::string& mode, bool allow_concat) {
  if (mode == "sum") return CUEMBED_SUM;
  if (mode == "mean") return CUEMBED_MEAN;
  TORCH_CHECK(allow_concat && mode == "concat", "cuembed_pyt: mode must be 'sum', 'mean'",
              allow_concat ? " or 'concat'" : "");
  return CUEMBED_CONCAT;
}

// What the library's dispatchers (SplitRow, UpdateLaneBytes) would abort on, as exceptions: a row size or a data pointer
// that is not a multiple of 4 bytes, and -- `limit_lanes`: the kernels that give every lane of a row a thread -- a row of
// more than 1,024 lanes of the widest of 16 / 8 / 4 bytes that the row size and every pointer divide by.
void CheckRowAlignment(const char* what, const int64_t width, const int64_t element_size,
                       std::initializer_list<const void*> pointers, const bool limit_lanes) {
  const int64_t row_bytes = width * element_size;
  TORCH_CHECK(width > 0 && row_bytes % 4 == 0, "cuembed_pyt: the row size of ", what, " must be a multiple of 4 bytes");
  uintptr_t bits = static_cast<uintptr_t>(row_bytes);
  for (const void* p : pointers) {
    TORCH_CHECK(reinterpret_cast<uintptr_t>(p) % 4 == 0, "cuembed_pyt: ", what, " must be 4-byte aligned");
    bits |= reinterpret_cast<uintptr_t>(p);
  }
  const int64_t lane_bytes = bits % 16 == 0 ? 16 : (bits % 8 == 0 ? 8 : 4);
  TORCH_CHECK(!limit_lanes || row_bytes / lane_bytes <= 1024, "cuembed_pyt: ", what, ": a row of ", row_bytes,
              " bytes needs ", row_bytes / lane_bytes, " lanes of ", lane_bytes,
              " bytes, more than 1024; align the data to 16 bytes");
}

int IndexBits(const int64_t num_categories) {
  if (num_categories <= 0) return 0;
  int bits = 1;
  while (bits < 63 && (int64_t{1} << bits) < num_categories) ++bits;
  return bits;
}

// ---- the reference's four ops --------------------------------------------------------------

// reference: cuembed_embedding.cu:10-52 (CSR layout, offsets has batch + 1 entries)
// `row_loads` -1 = the process-wide default, 0 / 1 = RowLoadPolicy; `sample_order` = ForwardOptions::sample_order
// (a permutation of the samples; undefined = none): scheduling hints, never a different result.
at::Tensor ForwardImpl(const at::Tensor& params, const at::Tensor& indices, const at::Tensor& offsets,
                       const at::Tensor& weights, const std::string& mode, const int row_loads,
                       const at::Tensor& sample_order, const at::Tensor& row_loads_device = at::Tensor()) {
  CheckGpu(params, "params");
  CheckGpu(indices, "indices");
  CheckGpu(offsets, "offsets");
  TORCH_CHECK(params.dim() == 2, "cuembed_pyt: params must be [num_categories, embed_width]");
  const int elem = ElemCode(params, "params");
  const int idx = IndexCode(indices, "indices");
  const int off = IndexCode(offsets, "offsets");
  if (weights.defined()) {
    CheckGpu(weights, "weights");
    TORCH_CHECK(weights.scalar_type() == params.scalar_type(), "cuembed_pyt: weights must have the dtype of params");
    TORCH_CHECK(weights.numel() >= indices.numel(), "cuembed_pyt: weights must have one entry per index");
  }
  const int m = Mode(mode, false);
  const at::DeviceGuard guard(params.device());
  const at::Tensor p = params.contiguous(), i = indices.contiguous(), o = offsets.contiguous();
  const at::Tensor w = ContiguousOrUndefined(weights);
  const int64_t batch = o.numel() - 1;
  TORCH_CHECK(batch >= 0, "cuembed_pyt: offsets must hold batch_size + 1 entries");
  CheckRowAlignment("params", p.size(1), p.element_size(), {Ptr(p)}, true);
  at::Tensor out = at::empty({batch, p.size(1)}, p.options());
  if (sample_order.defined())
    TORCH_CHECK(sample_order.is_cuda() && sample_order.scalar_type() == at::kInt && sample_order.numel() == batch &&
                    sample_order.is_contiguous(),
                "cuembed_pyt: sample_order must be a contiguous int32 permutation of the samples on the GPU");
  if (row_loads_device.defined())      // the words cuembed_decide_row_loads works on: the kernels read the decision themselves
    TORCH_CHECK(row_loads_device.is_cuda() && row_loads_device.scalar_type() == at::kInt && row_loads_device.numel() >= 4 &&
                    row_loads_device.is_contiguous(),
                "cuembed_pyt: row_loads_device must be the contiguous 4-word int32 tensor of cuembed_decide_row_loads");
  if (batch > 0)
    ::cuembed_embedding_forward_device_hints(Ptr(p), elem, static_cast<int>(p.size(1)), Ptr(i), idx, Ptr(o), off, Ptr(w),
                                             static_cast<int>(batch), 0, m, 0, MutPtr(out), /*reduction_order=*/-1, row_loads,
                                             static_cast<const int32_t*>(Ptr(sample_order)),
                                             static_cast<const uint32_t*>(Ptr(row_loads_device)), CurrentStream(p));
  return out;
}

at::Tensor cuembed_embedding_forward_op(const at::Tensor& params, const at::Tensor& indices,
                                     const at::Tensor& offsets, const at::Tensor& weights,
                                     const std::string& mode) {
  return ForwardImpl(params, indices, offsets, weights, mode, -1, at::Tensor());
}

// Extension: ... with the per-call scheduling hints of cuembed::ForwardOptions.
at::Tensor cuembed_embedding_forward_hinted_op(const at::Tensor& params, const at::Tensor& indices,
                                            const at::Tensor& offsets, const c10::optional<at::Tensor>& weights,
                                            const std::string& mode, const int64_t row_loads,
                                            const c10::optional<at::Tensor>& sample_order,
                                            const c10::optional<at::Tensor>& row_loads_device) {
  return ForwardImpl(params, indices, offsets, weights.has_value() ? *weights : at::Tensor(), mode,
                     static_cast<int>(row_loads), sample_order.has_value() ? *sample_order : at::Tensor(),
                     row_loads_device.has_value() ? *row_loads_device : at::Tensor());
}

// Extension (cuembed::DecideRowLoads): the row-load policy decided on the device from the batch's indices; `decision` is
// four int32 words zeroed once by the caller, handed to the forward as row_loads_device.  One launch, no read-back.
void cuembed_decide_row_loads_op(const at::Tensor& indices, const int64_t table_bytes, at::Tensor decision) {
  CheckGpu(indices, "indices");
  CheckGpu(decision, "decision");
  const int idx = IndexCode(indices, "indices");
  TORCH_CHECK(decision.scalar_type() == at::kInt && decision.numel() >= 4 && decision.is_contiguous(),
              "cuembed_pyt: decision must be a contiguous int32 tensor of 4 words");
  const at::DeviceGuard guard(indices.device());
  const at::Tensor i = indices.contiguous();
  ::cuembed_decide_row_loads(Ptr(i), idx, i.numel(), table_bytes, static_cast<uint32_t*>(decision.data_ptr()), 0u,
                             CurrentStream(i));
}

// Extension (cuembed::BagOrderByLength): the samples of a CSR batch by descending bag length, for sample_order.
at::Tensor cuembed_bag_order_by_length_op(const at::Tensor& offsets, const int64_t max_length) {
  CheckGpu(offsets, "offsets");
  const int off = IndexCode(offsets, "offsets");
  const at::DeviceGuard guard(offsets.device());
  const at::Tensor o = offsets.contiguous();
  const int64_t batch = o.numel() - 1;
  TORCH_CHECK(batch >= 0, "cuembed_pyt: offsets must hold batch_size + 1 entries");
  at::Tensor order = at::empty({batch}, o.options().dtype(at::kInt));
  if (batch == 0) return order;
  size_t lwork = 0;
  ::cuembed_bag_order_by_length(nullptr, off, static_cast<int>(batch), static_cast<int>(max_length), nullptr, nullptr,
                                &lwork, nullptr);
  at::Tensor work = at::empty({static_cast<int64_t>(lwork > 0 ? lwork : 1)}, o.options().dtype(at::kByte));
  ::cuembed_bag_order_by_length(Ptr(o), off, static_cast<int>(batch), static_cast<int>(max_length),
                                static_cast<int32_t*>(order.data_ptr()), static_cast<char*>(work.data_ptr()), &lwork,
                                CurrentStream(o));
  return order;
}

// reference: cuembed_embedding.cu:54-68.  The reference's Python passes offsets[:-1] and the
// kernel reads one element past the slice; here the end of the last bag is `nnz`, which is right
// for the sliced and for the full offsets tensor alike.
at::Tensor cuembed_extract_row_ids_from_csr_op(const at::Tensor& offsets, const int64_t nnz) {
  CheckGpu(offsets, "offsets");
  const int off = IndexCode(offsets, "offsets");
  const at::DeviceGuard guard(offsets.device());
  const int64_t batch = offsets.numel();
  at::Tensor closed = at::empty({batch + 1}, offsets.options());
  closed.narrow(0, 0, batch).copy_(offsets.reshape({-1}));
  closed.narrow(0, batch, 1).fill_(nnz);
  at::Tensor row_ids = at::empty({nnz}, offsets.options());
  if (batch > 0 && nnz > 0)
    ::cuembed_extract_row_ids_from_csr(Ptr(closed), off, static_cast<int>(batch), off, MutPtr(row_ids),
                                       CurrentStream(offsets));
  return row_ids;
}

// Extension: the same for an offsets tensor that already holds batch + 1 entries (what callers of
// cuembed_embedding_forward have anyway): no copy, one launch.
at::Tensor cuembed_extract_row_ids_from_offsets_op(const at::Tensor& offsets, const int64_t nnz) {
  CheckGpu(offsets, "offsets");
  const int off = IndexCode(offsets, "offsets");
  TORCH_CHECK(offsets.numel() >= 1, "cuembed_pyt: offsets must hold batch_size + 1 entries");
  const at::DeviceGuard guard(offsets.device());
  const at::Tensor o = offsets.contiguous();
  const int64_t batch = o.numel() - 1;
  at::Tensor row_ids = at::empty({nnz}, o.options());
  if (batch > 0 && nnz > 0)
    ::cuembed_extract_row_ids_from_csr(Ptr(o), off, static_cast<int>(batch), off, MutPtr(row_ids), CurrentStream(o));
  return row_ids;
}

std::tuple<at::Tensor, at::Tensor, at::Tensor> TransposeImpl(const at::Tensor& rows, const at::Tensor& cols,
                                                             const at::Tensor& weights, const int index_bits,
                                                             const int row_bits, const int sample_blocks = 1) {
  CheckGpu(rows, "rows");
  CheckGpu(cols, "cols");
  const int idx = IndexCode(rows, "rows");
  TORCH_CHECK(cols.scalar_type() == rows.scalar_type() && cols.numel() == rows.numel(),
              "cuembed_pyt: rows and cols must have the same dtype and length");
  int wt = CUEMBED_F32;
  if (weights.defined()) {
    CheckGpu(weights, "weights");
    wt = ElemCode(weights, "weights");
    TORCH_CHECK(weights.numel() == rows.numel(), "cuembed_pyt: weights must have nnz entries");
  }
  const at::DeviceGuard guard(rows.device());
  const at::Tensor r = rows.contiguous(), c = cols.contiguous(), w = ContiguousOrUndefined(weights);
  const int64_t nnz = r.numel();
  TORCH_CHECK(nnz <= INT32_MAX, "cuembed_pyt: nnz must fit an int (reference API, index_transforms.cuh:224-234)");
  at::Tensor t_rows = at::empty_like(c), t_cols = at::empty_like(r);
  // the reference returns a 0-length float tensor when there are no weights (cuembed_embedding.cu:90-93)
  at::Tensor t_w = w.defined() ? at::empty_like(w) : at::empty({0}, r.options().dtype(at::kFloat));
  if (nnz == 0) return {t_rows, t_cols, t_w};
  size_t lwork = 0;
  const void* query_weights = w.defined() ? reinterpret_cast<const void*>(256) : nullptr;  // only its nullness matters
  ::cuembed_transpose_sample_blocks(nullptr, nullptr, query_weights, static_cast<int>(nnz), idx, wt, nullptr, nullptr,
                                    nullptr, nullptr, &lwork, index_bits, row_bits, sample_blocks, nullptr);
  at::Tensor work = at::empty({static_cast<int64_t>(lwork)}, r.options().dtype(at::kByte));
  ::cuembed_transpose_sample_blocks(Ptr(r), Ptr(c), Ptr(w), static_cast<int>(nnz), idx, wt, MutPtr(t_rows),
                                    MutPtr(t_cols), w.defined() ? MutPtr(t_w) : nullptr,
                                    static_cast<char*>(work.data_ptr()), &lwork, index_bits, row_bits, sample_blocks,
                                    CurrentStream(r));
  return {t_rows, t_cols, t_w};
}

// reference: cuembed_embedding.cu:70-120
std::tuple<at::Tensor, at::Tensor, at::Tensor> cuembed_transpose_op(const at::Tensor& rows, const at::Tensor& cols,
                                                                 const at::Tensor& weights) {
  return TransposeImpl(rows, cols, weights, 0, 0);
}

// reference: cuembed_embedding.cu:122-167 (dense gradient: torch::zeros + skip_grad_init)
at::Tensor cuembed_embedding_backward_op(const at::Tensor& y_grad, const int64_t num_categories,
                                      const at::Tensor& transpose_indices, const at::Tensor& transpose_sample_ids,
                                      const at::Tensor& transpose_weights) {
  CheckGpu(y_grad, "y_grad");
  CheckGpu(transpose_indices, "transpose_indices");
  CheckGpu(transpose_sample_ids, "transpose_sample_ids");
  TORCH_CHECK(y_grad.dim() == 2, "cuembed_pyt: y_grad must be [rows, embed_width]");
  const int elem = ElemCode(y_grad, "y_grad");
  const int idx = IndexCode(transpose_indices, "transpose_indices");
  TORCH_CHECK(transpose_sample_ids.scalar_type() == transpose_indices.scalar_type() &&
                  transpose_sample_ids.numel() == transpose_indices.numel(),
              "cuembed_pyt: transpose_sample_ids must match transpose_indices");
  if (transpose_weights.defined())
    TORCH_CHECK(transpose_weights.scalar_type() == y_grad.scalar_type() &&
                    transpose_weights.numel() == transpose_indices.numel(),
                "cuembed_pyt: transpose_weights must be nnz entries of y_grad's dtype");
  TORCH_CHECK(num_categories <= INT32_MAX && transpose_indices.numel() <= INT32_MAX, "cuembed_pyt: sizes must fit an int");
  const at::DeviceGuard guard(y_grad.device());
  const at::Tensor g = y_grad.contiguous(), ti = transpose_indices.contiguous(),
                   ts = transpose_sample_ids.contiguous(), tw = ContiguousOrUndefined(transpose_weights);
  CheckRowAlignment("y_grad", g.size(1), g.element_size(), {Ptr(g)}, true);
  at::Tensor grad = at::zeros({num_categories, g.size(1)}, g.options());
  ::cuembed_embedding_backward(Ptr(g), elem, static_cast<int>(g.size(1)), static_cast<int>(num_categories),
                               static_cast<int>(ti.numel()), Ptr(ti), Ptr(ts), nullptr, idx, Ptr(tw),
                               /*skip_grad_init=*/1, MutPtr(grad), nullptr, CurrentStream(g));
  return grad;
}

// ---- extensions ------------------------------------------------------------------------------

std::tuple<at::Tensor, at::Tensor, at::Tensor> cuembed_transpose_bounded_op(const at::Tensor& rows, const at::Tensor& cols,
                                                                         const at::Tensor& weights,
                                                                         const int64_t num_categories) {
  return TransposeImpl(rows, cols, weights, IndexBits(num_categories), 0);
}

// sample ids of a CSR / fixed-hotness batch are < nnz: int64 ids travel as 32 bits without a look
std::tuple<at::Tensor, at::Tensor, at::Tensor> cuembed_transpose_sample_ids_op(const at::Tensor& sample_ids,
                                                                            const at::Tensor& indices,
                                                                            const at::Tensor& weights,
                                                                            const int64_t num_categories) {
  return TransposeImpl(sample_ids, indices, weights, IndexBits(num_categories), 31);
}

// Transpose in blocks of samples (cuembed::Transpose, sample_blocks): for the compressed gradient only -- with the
// plain remap the result is an UNCOALESCED compressed gradient, one row per (block, table row).  sample_blocks is
// forwarded as given (<= 1: one block, the reference's fully sorted order); the caller asks
// cuembed_recommended_sample_blocks for a recommendation (cuembed_pyt.py does).
std::tuple<at::Tensor, at::Tensor, at::Tensor> cuembed_transpose_sample_blocks_op(const at::Tensor& sample_ids,
                                                                               const at::Tensor& indices,
                                                                               const at::Tensor& weights,
                                                                               const int64_t num_categories,
                                                                               const int64_t sample_blocks) {
  return TransposeImpl(sample_ids, indices, weights, IndexBits(num_categories), 31, static_cast<int>(sample_blocks));
}

at::Tensor cuembed_compute_compressed_grad_indices_op(const at::Tensor& transpose_indices) {
  CheckGpu(transpose_indices, "transpose_indices");
  const int idx = IndexCode(transpose_indices, "transpose_indices");
  const at::DeviceGuard guard(transpose_indices.device());
  const at::Tensor ti = transpose_indices.contiguous();
  TORCH_CHECK(ti.numel() <= INT32_MAX, "cuembed_pyt: nnz must fit an int");
  at::Tensor remapped = at::empty_like(ti);
  if (ti.numel() == 0) return remapped;
  size_t lwork = 0;
  ::cuembed_compute_compressed_grad_indices(nullptr, static_cast<int>(ti.numel()), idx, nullptr, nullptr, &lwork, nullptr);
  at::Tensor work = at::empty({static_cast<int64_t>(lwork > 0 ? lwork : 1)}, ti.options().dtype(at::kByte));
  ::cuembed_compute_compressed_grad_indices(Ptr(ti), static_cast<int>(ti.numel()), idx, MutPtr(remapped),
                                            static_cast<char*>(work.data_ptr()), &lwork, CurrentStream(ti));
  return remapped;
}

// compressed gradient: (rows[num_unique, W], inverse_mapping[num_unique])
std::tuple<at::Tensor, at::Tensor> cuembed_embedding_backward_compressed_op(
    const at::Tensor& y_grad, const int64_t num_unique, const at::Tensor& transpose_indices,
    const at::Tensor& transpose_sample_ids, const at::Tensor& transpose_remapped_indices,
    const at::Tensor& transpose_weights) {
  CheckGpu(y_grad, "y_grad");
  TORCH_CHECK(y_grad.dim() == 2, "cuembed_pyt: y_grad must be [rows, embed_width]");
  const int elem = ElemCode(y_grad, "y_grad");
  const int idx = IndexCode(transpose_indices, "transpose_indices");
  TORCH_CHECK(transpose_sample_ids.scalar_type() == transpose_indices.scalar_type() &&
                  transpose_remapped_indices.scalar_type() == transpose_indices.scalar_type() &&
                  transpose_sample_ids.numel() == transpose_indices.numel() &&
                  transpose_remapped_indices.numel() == transpose_indices.numel(),
              "cuembed_pyt: the transposed index tensors must agree in dtype and length");
  if (transpose_weights.defined())
    TORCH_CHECK(transpose_weights.scalar_type() == y_grad.scalar_type() &&
                    transpose_weights.numel() == transpose_indices.numel(),
                "cuembed_pyt: transpose_weights must be nnz entries of y_grad's dtype");
  TORCH_CHECK(num_unique <= INT32_MAX && transpose_indices.numel() <= INT32_MAX, "cuembed_pyt: sizes must fit an int");
  const at::DeviceGuard guard(y_grad.device());
  const at::Tensor g = y_grad.contiguous(), ti = transpose_indices.contiguous(),
                   ts = transpose_sample_ids.contiguous(), tr = transpose_remapped_indices.contiguous(),
                   tw = ContiguousOrUndefined(transpose_weights);
  CheckRowAlignment("y_grad", g.size(1), g.element_size(), {Ptr(g)}, true);
  at::Tensor grad = at::empty({num_unique, g.size(1)}, g.options());
  at::Tensor inv = at::empty({num_unique}, ti.options());
  const int width = static_cast<int>(g.size(1)), nnz = static_cast<int>(ti.numel());
  ::cuembed_embedding_backward(Ptr(g), elem, width, static_cast<int>(num_unique), nnz, Ptr(ti), Ptr(ts), Ptr(tr), idx,
                               Ptr(tw), /*skip_grad_init=*/0, MutPtr(grad), MutPtr(inv), CurrentStream(g));
  return {grad, inv};
}

at::Tensor cuembed_embedding_forward_fixed_op(const at::Tensor& params, const at::Tensor& indices,
                                           const at::Tensor& weights, const std::string& mode) {
  CheckGpu(params, "params");
  CheckGpu(indices, "indices");
  TORCH_CHECK(params.dim() == 2 && indices.dim() == 2, "cuembed_pyt: params [rows, width], indices [batch, hotness]");
  const int elem = ElemCode(params, "params");
  const int idx = IndexCode(indices, "indices");
  const int m = Mode(mode, true);
  if (weights.defined()) {
    TORCH_CHECK(m != CUEMBED_CONCAT, "cuembed_pyt: concat does not take weights");
    TORCH_CHECK(weights.scalar_type() == params.scalar_type() && weights.sizes() == indices.sizes(),
                "cuembed_pyt: weights must match indices in shape and params in dtype");
  }
  const at::DeviceGuard guard(params.device());
  const at::Tensor p = params.contiguous(), i = indices.contiguous(), w = ContiguousOrUndefined(weights);
  const int64_t batch = i.size(0), hot = i.size(1), width = p.size(1);
  TORCH_CHECK(hot > 0, "cuembed_pyt: hotness must be positive");
  CheckRowAlignment("params", width, p.element_size(), {Ptr(p)}, true);
  at::Tensor out = m == CUEMBED_CONCAT ? at::empty({batch, hot, width}, p.options()) : at::empty({batch, width}, p.options());
  if (batch > 0)
    ::cuembed_embedding_forward(Ptr(p), elem, static_cast<int>(width), Ptr(i), idx, nullptr, 0, Ptr(w),
                                static_cast<int>(batch), static_cast<int>(hot), m, 0, MutPtr(out), CurrentStream(p));
  return out;
}

at::Tensor cuembed_embedding_weight_grad_op(const at::Tensor& params, const at::Tensor& indices,
                                         const at::Tensor& offsets, const at::Tensor& y_grad) {
  CheckGpu(params, "params");
  CheckGpu(indices, "indices");
  CheckGpu(offsets, "offsets");
  CheckGpu(y_grad, "y_grad");
  const int elem = ElemCode(params, "params");
  const int idx = IndexCode(indices, "indices");
  const int off = IndexCode(offsets, "offsets");
  TORCH_CHECK(y_grad.scalar_type() == params.scalar_type() && y_grad.dim() == 2 && y_grad.size(1) == params.size(1),
              "cuembed_pyt: y_grad must be [batch, width] of the table's dtype");
  const at::DeviceGuard guard(params.device());
  const at::Tensor p = params.contiguous(), i = indices.contiguous(), o = offsets.contiguous(), g = y_grad.contiguous();
  const int64_t batch = o.numel() - 1;
  TORCH_CHECK(p.dim() == 2, "cuembed_pyt: params must be [num_categories, embed_width]");
  CheckRowAlignment("params / y_grad", p.size(1), p.element_size(), {Ptr(p), Ptr(g)}, true);
  at::Tensor out = at::empty({i.numel()}, p.options());
  if (batch > 0 && i.numel() > 0)
    ::cuembed_embedding_weight_grad(Ptr(p), elem, static_cast<int>(p.size(1)), Ptr(i), idx, Ptr(o), off, Ptr(g),
                                    static_cast<int>(batch), 0, MutPtr(out), CurrentStream(p));
  return out;
}

// One call for the index work of a fixed-hotness training step: (sorted indices, sample ids,
// weights, dense ids) = TransposeFixedHotness + ComputeCompressedGradIndices.
std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor> cuembed_transpose_fixed_hotness_op(
    const at::Tensor& indices, const at::Tensor& weights, const int64_t num_categories, const bool compressed) {
  CheckGpu(indices, "indices");
  TORCH_CHECK(indices.dim() == 2, "cuembed_pyt: indices must be [batch, hotness]");
  const int idx = IndexCode(indices, "indices");
  int wt = CUEMBED_F32;
  if (weights.defined()) {
    wt = ElemCode(weights, "weights");
    TORCH_CHECK(weights.numel() == indices.numel(), "cuembed_pyt: weights must match indices");
  }
  const at::DeviceGuard guard(indices.device());
  const at::Tensor i = indices.contiguous(), w = ContiguousOrUndefined(weights);
  const int64_t batch = i.size(0), hot = i.size(1), nnz = batch * hot;
  TORCH_CHECK(nnz <= INT32_MAX && hot > 0, "cuembed_pyt: batch * hotness must fit an int");
  const auto flat = i.options();
  at::Tensor t_idx = at::empty({nnz}, flat), t_sid = at::empty({nnz}, flat);
  at::Tensor t_w = w.defined() ? at::empty({nnz}, w.options()) : at::empty({0}, flat.dtype(at::kFloat));
  at::Tensor remap = at::empty({compressed ? nnz : 0}, flat);
  if (nnz == 0) return {t_idx, t_sid, t_w, remap};
  size_t lwork = 0, lwork2 = 0;
  const void* query_weights = w.defined() ? reinterpret_cast<const void*>(256) : nullptr;
  ::cuembed_transpose_fixed_hotness(nullptr, query_weights, static_cast<int>(batch), static_cast<int>(hot), idx, wt,
                                    nullptr, nullptr, nullptr, nullptr, &lwork, IndexBits(num_categories), nullptr);
  ::cuembed_compute_compressed_grad_indices(nullptr, static_cast<int>(nnz), idx, nullptr, nullptr, &lwork2, nullptr);
  size_t both = lwork > lwork2 ? lwork : lwork2;
  at::Tensor work = at::empty({static_cast<int64_t>(both)}, flat.dtype(at::kByte));
  const cuembed_stream_t stream = CurrentStream(i);
  ::cuembed_transpose_fixed_hotness(Ptr(i), Ptr(w), static_cast<int>(batch), static_cast<int>(hot), idx, wt,
                                    MutPtr(t_idx), MutPtr(t_sid), w.defined() ? MutPtr(t_w) : nullptr,
                                    static_cast<char*>(work.data_ptr()), &both, IndexBits(num_categories), stream);
  if (compressed)
    ::cuembed_compute_compressed_grad_indices(Ptr(t_idx), static_cast<int>(nnz), idx, MutPtr(remap),
                                              static_cast<char*>(work.data_ptr()), &both, stream);
  return {t_idx, t_sid, t_w, remap};
}


// ---- the whole training step of cuemb_embedding as ONE autograd node -------------------------------------------
// examples/pytorch/cuembed_pyt.py:12-51 runs forward and backward as a Python autograd.Function over four ops; at small
// batches that is host-bound (B = 1024, H = 64: 0.236 ms per step for ~0.09 ms of kernels, most of it the Python
// dispatch of six ops and a read-back of num_unique in the MIDDLE of the backward).  Here forward and backward are one
// C++ node each: the backward enqueues row ids -> transpose (+ remap in the same call) -> scatter-add without returning
// to Python, and for a sparse gradient the row count is read back AFTER everything is enqueued (the scatter runs into
// buffers of capacity min(nnz, rows) under cuembed_embedding_backward_bounded and the result is narrowed to
// num_unique rows), so the host waits for the device once, at the end, instead of stalling the pipeline in the middle.
// Above kCapacityBytes of worst-case gradient the count is read back first, as before (2.1 GB at the C4 shape; there
// the device is the bottleneck, not the host: running the scatter into 5/4 of the table's LAST row count under the
// capacity check and reading the count at the end was built and measured 0.53-0.63 ms against 0.49 -- 435 MB
// allocations of changing size churn the caching allocator).
constexpr int64_t kCapacityBytes = int64_t{192} << 20;
// Up to this much worst-case gradient the "fastest order" kinds do not read the count back AT ALL: the gradient is
// handed on padded to min(nnz, rows) entries (zero rows that name a row of the batch: an uncoalesced COO tensor of the
// same value), so the host never waits for the device inside a step -- at B = 1024 the wait was a third of the step.
// Why not more: with the limit raised (tools/torch_padded_limit_probe.py, profiles/r05_torch_padded_limit_probe.txt) the step
// alone gains further (4,096 samples, 128 MB: 0.193 -> 0.122 ms; 8,192: 0.187 -> 0.164; slower from 16,384 on), but whoever
// consumes the gradient pays for min(lookups, rows) entries instead of num_unique (tools/padded_gradient_consumer_probe.py:
// step + torch.optim.SGD at 4,096 samples 0.236 -> 0.448 ms, at 1,024 samples 0.16 -> 0.22; step + coalesce() 0.29 -> 0.23 at
// 1,024, 0.32 -> 0.37 at 4,096) -- the entry count of torch's own EmbeddingBag(sparse=True) gradient, but not what
// "reference" hands on.  CUEMBED_PYT_PADDED_MB moves the limit (0: never pad).
constexpr int64_t kPaddedBytesDefault = int64_t{64} << 20;
// (tuning: CUEMBED_PYT_PADDED_MB, read once)
inline int64_t PaddedBytes() {
  static const int64_t v = [] {
    const char* e = std::getenv("CUEMBED_PYT_PADDED_MB");
    return e != nullptr ? (static_cast<int64_t>(std::atoll(e)) << 20) : kPaddedBytesDefault;
  }();
  return v;
}

// What the caller asked for (cuembed_pyt.py: sparse_grad=).  kGradSparseReference is the CONTRACT of sparse_grad=True: a
// coalesced tensor of exactly num_unique ascending rows, whatever the backend and whether or not torch.compile traces
// the call; the other sparse kinds are explicit opt-ins whose entry count differs from that (same dense value).
enum GradKind : int64_t {
  kGradDense = 0,
  kGradSparseFastest = 1,      // sample blocks when the shape gains from them, padded when the step would wait on the count
  kGradSparseReference = 2,    // fully sorted order: coalesced, num_unique rows
  kGradSparseUncoalesced = 3,  // sample blocks when the shape gains from them, exactly one entry per (block, row): never padded
  kGradSparsePadded = 4        // one block, min(lookups, rows) entries at ANY size: never reads the count, capturable
};

struct NarrowedIndices {
  at::Tensor idx, offsets;
};
// int64 indices of a table with < 2^31 rows: the index work of the backward runs on int32 copies (half the bytes through
// every sorting pass) -- from 2^18 lookups up, where the two conversions cost less than they save (cuembed_pyt.py).
NarrowedIndices NarrowForIndexWork(const at::Tensor& idx, const at::Tensor& offsets, const int64_t num_categories) {
  if (idx.scalar_type() == at::kLong && num_categories < (int64_t{1} << 31) && idx.numel() >= (int64_t{1} << 18) &&
      idx.numel() < (int64_t{1} << 31))
    return {idx.to(at::kInt), offsets.to(at::kInt)};
  // The forward takes indices and offsets of different integer types (ForwardImpl passes a type code for each); the index
  // work below has ONE type for lookups and sample ids, the one of the indices: offsets follow (their values are <= nnz,
  // which fits whatever type holds the lookups' count; int64 -> int32 is checked by the caller against INT32_MAX).
  if (offsets.scalar_type() != idx.scalar_type()) return {idx, offsets.to(idx.scalar_type())};
  return {idx, offsets};
}

struct TransposedLookups {
  at::Tensor t_idx, t_sid, t_w, remap;
};
// Transpose (+ ComputeCompressedGradIndices from the same call) of (sample_ids, indices[, weights]).
TransposedLookups TransposeWithRemap(const at::Tensor& sample_ids, const at::Tensor& indices, const at::Tensor& weights,
                                     const int64_t num_categories, const int sample_blocks, const bool want_remap) {
  CheckGpu(sample_ids, "sample_ids");
  CheckGpu(indices, "indices");
  const int idx = IndexCode(indices, "indices");
  // one type code names both arrays below: a pair of different integer types would be read and written past its end
  TORCH_CHECK(sample_ids.scalar_type() == indices.scalar_type() && sample_ids.numel() == indices.numel(),
              "cuembed_pyt: sample ids and indices must have the same dtype and length");
  TORCH_CHECK(indices.numel() <= INT32_MAX, "cuembed_pyt: the number of lookups must fit an int");
  TORCH_CHECK(sample_ids.is_contiguous() && indices.is_contiguous(), "cuembed_pyt: sample ids and indices must be contiguous");
  int wt = CUEMBED_F32;
  if (weights.defined()) {
    CheckGpu(weights, "weights");
    wt = ElemCode(weights, "weights");
    TORCH_CHECK(weights.numel() == indices.numel() && weights.is_contiguous(),
                "cuembed_pyt: weights must be contiguous with one entry per lookup");
  }
  const int nnz = static_cast<int>(indices.numel());
  TransposedLookups t;
  t.t_idx = at::empty_like(indices);
  t.t_sid = at::empty_like(sample_ids);
  if (weights.defined()) t.t_w = at::empty_like(weights);
  if (want_remap) t.remap = at::empty_like(indices);
  size_t lwork = 0;
  const void* query_weights = weights.defined() ? reinterpret_cast<const void*>(256) : nullptr;
  const int bits = IndexBits(num_categories);
  ::cuembed_transpose_remapped(nullptr, nullptr, query_weights, nnz, idx, wt, nullptr, nullptr, nullptr, nullptr, nullptr,
                               &lwork, bits, 31, sample_blocks, nullptr);
  at::Tensor work = at::empty({static_cast<int64_t>(lwork > 0 ? lwork : 1)}, indices.options().dtype(at::kByte));
  ::cuembed_transpose_remapped(Ptr(sample_ids), Ptr(indices), Ptr(weights), nnz, idx, wt, MutPtr(t.t_idx), MutPtr(t.t_sid),
                               weights.defined() ? MutPtr(t.t_w) : nullptr, want_remap ? MutPtr(t.remap) : nullptr,
                               static_cast<char*>(work.data_ptr()), &lwork, bits, 31, sample_blocks, CurrentStream(indices));
  return t;
}

class CuEmbEmbeddingNode : public torch::autograd::Function<CuEmbEmbeddingNode> {
 public:
  // (optional tensors travel as std::optional: autograd's argument scan cannot take an undefined at::Tensor)
  static at::Tensor forward(torch::autograd::AutogradContext* ctx, const at::Tensor& params, const at::Tensor& indices,
                            const at::Tensor& offsets, const c10::optional<at::Tensor>& optional_weights,
                            const int64_t grad_kind, const int64_t row_loads,
                            const c10::optional<at::Tensor>& optional_sample_order,
                            const c10::optional<at::Tensor>& optional_row_loads_device) {
    at::AutoDispatchBelowADInplaceOrView below;
    const at::Tensor weights = optional_weights.has_value() ? *optional_weights : at::Tensor();
    const at::Tensor sample_order = optional_sample_order.has_value() ? *optional_sample_order : at::Tensor();
    ctx->saved_data["num_categories"] = params.size(0);
    ctx->saved_data["grad_kind"] = grad_kind;
    ctx->saved_data["weighted"] = weights.defined();
    if (weights.defined()) ctx->save_for_backward({indices, offsets, weights});
    else ctx->save_for_backward({indices, offsets});
    return ForwardImpl(params, indices, offsets, weights, "sum", static_cast<int>(row_loads), sample_order,
                       optional_row_loads_device.has_value() ? *optional_row_loads_device : at::Tensor());
  }

  static torch::autograd::variable_list backward(torch::autograd::AutogradContext* ctx,
                                                 torch::autograd::variable_list grad_outputs) {
    at::AutoDispatchBelowADInplaceOrView below;
    const auto saved = ctx->get_saved_variables();
    const bool weighted = ctx->saved_data["weighted"].toBool();
    const int64_t num_categories = ctx->saved_data["num_categories"].toInt();
    const int64_t grad_kind = ctx->saved_data["grad_kind"].toInt();
    at::Tensor out_grad = grad_outputs[0];
    torch::autograd::variable_list grads(8);   // (params, indices, offsets, weights, grad_kind, row_loads, sample_order, row_loads_device)
    if (!ctx->needs_input_grad(0)) return grads;
    CheckGpu(out_grad, "the incoming gradient");
    const at::DeviceGuard guard(out_grad.device());
    out_grad = out_grad.contiguous();
    const int64_t width = out_grad.size(1);
    CheckRowAlignment("the incoming gradient", width, out_grad.element_size(), {Ptr(out_grad)}, true);
    const int64_t nnz = saved[0].numel();
    TORCH_CHECK(nnz <= INT32_MAX, "cuembed_pyt: the number of lookups must fit an int");
    const at::Tensor weights = weighted ? saved[2].contiguous() : at::Tensor();
    // (the forward reads the first nnz weights of a longer tensor; the transpose moves exactly nnz)
    TORCH_CHECK(!weighted || weights.numel() == nnz, "cuembed_pyt: weights must have one entry per index");
    if (nnz == 0) {
      if (grad_kind == kGradDense) {
        grads[0] = at::zeros({num_categories, width}, out_grad.options());
      } else {
        grads[0] = at::_sparse_coo_tensor_unsafe(at::empty({1, 0}, out_grad.options().dtype(at::kLong)),
                                                 at::empty({0, width}, out_grad.options()), {num_categories, width},
                                                 out_grad.options().layout(at::kSparse));
      }
      return grads;
    }
    const NarrowedIndices nw = NarrowForIndexWork(saved[0].contiguous(), saved[1].contiguous(), num_categories);
    const at::Tensor sample_ids = cuembed_extract_row_ids_from_offsets_op(nw.offsets, nnz);
    const int elem = ElemCode(out_grad, "the incoming gradient");
    const int idx = IndexCode(nw.idx, "indices");
    const cuembed_stream_t stream = CurrentStream(out_grad);
    if (grad_kind == kGradDense) {   // the reference's gradient: a zero-filled table-sized tensor (cuembed_embedding.cu:122-167)
      const TransposedLookups t = TransposeWithRemap(sample_ids, nw.idx, weights, num_categories, 1, false);
      grads[0] = cuembed_embedding_backward_op(out_grad, num_categories, t.t_idx, t.t_sid, t.t_w);
      return grads;
    }
    // ---- compressed gradient as a sparse COO tensor ----
    int blocks = 1;
    if (grad_kind == kGradSparseFastest || grad_kind == kGradSparseUncoalesced)   // while a block of samples is scattered every L2 gathers from 1 / blocks of out_grad
      blocks = ::cuembed_recommended_sample_blocks(elem, static_cast<int>(width), static_cast<int>(out_grad.size(0)), nnz);
    const TransposedLookups t = TransposeWithRemap(sample_ids, nw.idx, weights, num_categories, blocks, true);
    const bool one_block = ::cuembed_transpose_sample_block_length(nnz, blocks) >= nnz;
    const int64_t row_bound = one_block ? num_categories : static_cast<int64_t>(blocks) * num_categories;
    const int64_t capacity = nnz < row_bound ? nnz : row_bound;
    const int64_t row_bytes = width * static_cast<int64_t>(out_grad.element_size());
    at::Tensor rows, inv;
    int64_t num_unique = -1;
    const int64_t room = (grad_kind == kGradSparsePadded ||
                          capacity * row_bytes <= (kCapacityBytes > PaddedBytes() ? kCapacityBytes : PaddedBytes()))
                             ? capacity : 0;   // rows the scatter may write blind
    const auto exact_backward = [&]() {
      rows = at::empty({num_unique, width}, out_grad.options());
      inv = at::empty({num_unique}, nw.idx.options());
      ::cuembed_embedding_backward(Ptr(out_grad), elem, static_cast<int>(width), static_cast<int>(num_unique),
                                   static_cast<int>(nnz), Ptr(t.t_idx), Ptr(t.t_sid), Ptr(t.remap), idx, Ptr(t.t_w),
                                   /*skip_grad_init=*/0, MutPtr(rows), MutPtr(inv), stream);
      if (inv.scalar_type() != at::kLong) inv = inv.to(at::kLong);
    };
    const bool padded = grad_kind == kGradSparsePadded ||
                        (grad_kind == kGradSparseFastest && one_block && room > 0 && room * row_bytes <= PaddedBytes());
    if (padded) {
      rows = at::empty({room, width}, out_grad.options());
      inv = at::empty({room}, nw.idx.options());
      ::cuembed_embedding_backward_bounded(Ptr(out_grad), elem, static_cast<int>(width), -1, static_cast<int>(nnz),
                                           Ptr(t.t_idx), Ptr(t.t_sid), Ptr(t.remap), idx, Ptr(t.t_w), /*skip_grad_init=*/0,
                                           MutPtr(rows), MutPtr(inv), 1, nullptr, static_cast<int>(room), nullptr,
                                           /*pad_to_capacity=*/1, stream);
      if (inv.scalar_type() != at::kLong) inv = inv.to(at::kLong);
      grads[0] = at::_sparse_coo_tensor_unsafe(inv.unsqueeze(0), rows, {num_categories, width},
                                               out_grad.options().layout(at::kSparse), /*is_coalesced=*/false);
      return grads;
    }
    // (from here on the host has to read the row count: not something a HIP graph can hold)
    TORCH_CHECK(c10::hip::currentStreamCaptureStatusMayInitCtx() == c10::hip::CaptureStatus::None,
                "cuembed_pyt: this sparse gradient needs its row count on the host and cannot be captured into a graph: "
                "sparse_grad=\"padded\" never reads it (min(lookups, rows) entries, here ", (capacity * row_bytes) >> 20,
                " MiB), sparse_grad=\"fastest\" does not while those fit ", PaddedBytes() >> 20,
                " MiB; sparse_grad=True / \"reference\" / \"uncoalesced\" always read the count; sparse_grad=False never does");
    if (room > 0) {
      // everything is enqueued before the host looks at the device: rows for `room`, narrowed afterwards
      rows = at::empty({room, width}, out_grad.options());
      inv = at::empty({room}, nw.idx.options());
      ::cuembed_embedding_backward_bounded(Ptr(out_grad), elem, static_cast<int>(width), -1, static_cast<int>(nnz),
                                           Ptr(t.t_idx), Ptr(t.t_sid), Ptr(t.remap), idx, Ptr(t.t_w), /*skip_grad_init=*/0,
                                           MutPtr(rows), MutPtr(inv), 1, nullptr, static_cast<int>(room), nullptr, 0, stream);
      at::Tensor inv64 = inv.scalar_type() == at::kLong ? inv : inv.to(at::kLong);
      num_unique = t.remap.narrow(0, nnz - 1, 1).item().toLong() + 1;   // (the one wait of the step)
      rows = rows.narrow(0, 0, num_unique);
      inv = inv64.narrow(0, 0, num_unique);
    } else {
      num_unique = t.remap.narrow(0, nnz - 1, 1).item().toLong() + 1;
      exact_backward();
    }
    grads[0] = at::_sparse_coo_tensor_unsafe(inv.unsqueeze(0), rows, {num_categories, width},
                                             out_grad.options().layout(at::kSparse), /*is_coalesced=*/one_block);
    return grads;
  }
};

// ---- multi-GPU: the device-side halves of the sparse gradient exchange (cuembed_amd/distributed.py) ----------------
// As a chain of tensor operations (searchsorted, where, index_select, index_fill_, ...) the index work around the
// collectives was ~60 launches and more host time than the whole forward + backward step; here it is two ops that
// enqueue 2 and ~13 launches without returning to Python.  Nothing is read back.

// What the two single-table optimizer ops below share (GroupedStep further down is the grouped ops'): the type codes,
// the entries and the source of their count, and the one-word device tensors.  The checks run in the order of the
// three functions, with the op's own (the rule, the state tensors, the hyper-parameters) in between.
struct RowStep {
  int elem = CUEMBED_F32, idx = CUEMBED_I32, pieces = 1, words64 = 0;
  int64_t num_rows = -1, piece_rows = 0;
  const void* counts = nullptr;
  const void* last_id = nullptr;
  const float* lr_word = nullptr;
  const float* bias_word = nullptr;
  const int64_t* step_word = nullptr;
};

RowStep RowStepCodes(const at::Tensor& table, const at::Tensor& ids, const at::Tensor& rows) {
  RowStep c;
  CheckGpu(table, "table");
  CheckGpu(ids, "ids");
  CheckGpu(rows, "rows");
  c.elem = ElemCode(table, "table");
  c.idx = IndexCode(ids, "ids");
  return c;
}

void CheckRowStepShapes(const at::Tensor& table, const at::Tensor& ids, const at::Tensor& rows) {
  TORCH_CHECK(rows.scalar_type() == table.scalar_type(), "cuembed_pyt: rows must have the table's dtype");
  TORCH_CHECK(table.dim() == 2 && rows.dim() == 2 && rows.size(1) == table.size(1) && ids.dim() == 1 &&
                  rows.size(0) == ids.numel() && table.is_contiguous() && rows.is_contiguous() && ids.is_contiguous(),
              "cuembed_pyt: table [rows, width], rows [entries, width] and ids [entries] must be contiguous and agree");
  TORCH_CHECK((table.size(1) * table.element_size()) % 4 == 0, "cuembed_pyt: the row size must be a multiple of 4 bytes");
  CheckRowAlignment("table / rows", table.size(1), table.element_size(), {table.data_ptr(), Ptr(rows)}, false);
}

// The count source (count / counts + piece_rows / last_id / none), lr_device and (Adam: bias_factor_device, else
// nullptr) the other one-word tensor, then stochastic rounding and step_device.
void ParseRowStepSources(RowStep& c, const at::Tensor& table, const at::Tensor& ids, const int64_t count,
                         const c10::optional<at::Tensor>& counts, const c10::optional<at::Tensor>& last_id,
                         const int64_t piece_rows_arg, const c10::optional<at::Tensor>& lr_device,
                         const c10::optional<at::Tensor>* bias_factor_device, const bool stochastic_rounding,
                         const c10::optional<at::Tensor>& step_device) {
  const bool has_counts = counts.has_value() && counts->defined();
  const bool has_last = last_id.has_value() && last_id->defined();
  TORCH_CHECK((count >= 0) + has_counts + has_last <= 1, "cuembed_pyt: give at most one of count, counts and last_id");
  c.piece_rows = ids.numel();
  if (has_counts) {
    CheckGpu(*counts, "counts");
    c.words64 = IndexCode(*counts, "counts") == CUEMBED_I64;
    TORCH_CHECK(counts->is_contiguous() && counts->numel() >= 1, "cuembed_pyt: counts must be contiguous words");
    if (piece_rows_arg > 0) {
      c.pieces = static_cast<int>(counts->numel());
      c.piece_rows = piece_rows_arg;
    }
    TORCH_CHECK(c.pieces == counts->numel() && c.pieces * c.piece_rows == ids.numel(),
                "cuembed_pyt: ids must hold counts.numel() * piece_rows entries");
    c.counts = counts->data_ptr();
  } else if (has_last) {
    CheckGpu(*last_id, "last_id");
    TORCH_CHECK(last_id->scalar_type() == ids.scalar_type() && last_id->numel() == 1,
                "cuembed_pyt: last_id must be one word of ids' dtype");
    c.last_id = last_id->data_ptr();
  } else {
    c.num_rows = count >= 0 ? count : ids.numel();
    TORCH_CHECK(c.num_rows <= ids.numel(), "cuembed_pyt: count exceeds the entries");
  }
  const auto word = [&](const c10::optional<at::Tensor>& t, const char* name) -> const float* {
    if (!t.has_value() || !t->defined()) return nullptr;
    CheckGpu(*t, name);
    TORCH_CHECK(t->scalar_type() == at::kFloat && t->numel() == 1, "cuembed_pyt: ", name, " must be one float32 word");
    return static_cast<const float*>(t->data_ptr());
  };
  c.lr_word = word(lr_device, "lr_device");
  if (bias_factor_device != nullptr) c.bias_word = word(*bias_factor_device, "bias_factor_device");
  if (stochastic_rounding) {
    TORCH_CHECK(table.scalar_type() != at::kFloat,
                "cuembed_pyt: stochastic_rounding is for float16 / bfloat16 tables: a float32 table is not rounded");
    if (step_device.has_value() && step_device->defined()) {
      CheckGpu(*step_device, "step_device");
      TORCH_CHECK(step_device->scalar_type() == at::kLong && step_device->numel() == 1 &&
                      step_device->device() == table.device(),
                  "cuembed_pyt: step_device must be one int64 word on the table's device");
      c.step_word = static_cast<const int64_t*>(step_device->data_ptr());
    }
  }
}

// Extension (cuembed::SparseRowUpdate): the sparse optimizer step on a compressed gradient, in place.  rule "sgd" /
// "adagrad" (state fp32 [rows, width]) / "rowwise_adagrad" (state fp32 [rows]).  Valid entries, at most one of:
// count >= 0 (host-known); counts (device words, int32 / int64: with piece_rows > 0 one per piece of piece_rows
// entries, else one word for all entries); last_id (one word of ids' dtype, count = last_id + 1); none: every entry.
// lr_device: one fp32 device word read by the kernel instead of lr.  stochastic_rounding (fp16 / bf16 tables): the
// rounding to the table's type is stochastic with the bits of (seed, step) -- the signed words carry the unsigned 64-bit
// values -- or of (seed, *step_device), one int64 device word.  One launch, nothing read back.
void cuembed_sparse_row_update_op(at::Tensor table, const c10::optional<at::Tensor>& state_arg, const at::Tensor& ids,
                                  const at::Tensor& rows, const std::string& rule, const double lr, const double eps,
                                  const c10::optional<at::Tensor>& lr_device, const int64_t count,
                                  const c10::optional<at::Tensor>& counts, const c10::optional<at::Tensor>& last_id,
                                  const int64_t piece_rows_arg, const bool stochastic_rounding, const int64_t seed,
                                  const int64_t step, const c10::optional<at::Tensor>& step_device) {
  RowStep c = RowStepCodes(table, ids, rows);
  const int code = rule == "sgd" ? CUEMBED_UPDATE_SGD
                   : rule == "adagrad" ? CUEMBED_UPDATE_ADAGRAD
                   : rule == "rowwise_adagrad" ? CUEMBED_UPDATE_ROWWISE_ADAGRAD : -1;
  TORCH_CHECK(code >= 0, "cuembed_pyt: rule must be 'sgd', 'adagrad' or 'rowwise_adagrad'");
  CheckRowStepShapes(table, ids, rows);
  at::Tensor state = state_arg.has_value() ? *state_arg : at::Tensor();
  if (code == CUEMBED_UPDATE_SGD) {
    TORCH_CHECK(!state.defined(), "cuembed_pyt: rule 'sgd' takes no state");
  } else {
    TORCH_CHECK(state.defined() && state.is_cuda() && state.scalar_type() == at::kFloat && state.is_contiguous() &&
                    (code == CUEMBED_UPDATE_ADAGRAD ? state.sizes() == table.sizes()
                                                    : (state.dim() == 1 && state.size(0) == table.size(0))),
                "cuembed_pyt: the state must be a contiguous float32 GPU tensor, [rows, width] for 'adagrad', [rows] for "
                "'rowwise_adagrad'");
    // a lane moves at least 4 bytes of the table, so 4 / sizeof(element) accumulator words at a time
    const uintptr_t state_align = 4 * (4 / static_cast<uintptr_t>(table.element_size()));
    TORCH_CHECK(code != CUEMBED_UPDATE_ADAGRAD || reinterpret_cast<uintptr_t>(state.data_ptr()) % state_align == 0,
                "cuembed_pyt: the state must be ", state_align, "-byte aligned for a ", table.scalar_type(), " table");
  }
  ParseRowStepSources(c, table, ids, count, counts, last_id, piece_rows_arg, lr_device, nullptr, stochastic_rounding,
                      step_device);
  if (ids.numel() == 0) return;
  const at::DeviceGuard guard(table.device());
  float* state_ptr = state.defined() ? static_cast<float*>(state.data_ptr()) : nullptr;
  if (stochastic_rounding) {
    ::cuembed_sparse_row_update_stochastic(table.data_ptr(), c.elem, static_cast<int>(table.size(1)), state_ptr, code,
                                           Ptr(ids), c.idx, Ptr(rows), c.piece_rows, c.pieces, c.num_rows, c.counts,
                                           c.words64, c.last_id, static_cast<float>(lr), c.lr_word,
                                           static_cast<float>(eps), static_cast<uint64_t>(seed),
                                           static_cast<uint64_t>(step), c.step_word, CurrentStream(table));
    return;
  }
  ::cuembed_sparse_row_update(table.data_ptr(), c.elem, static_cast<int>(table.size(1)), state_ptr, code, Ptr(ids), c.idx,
                              Ptr(rows), c.piece_rows, c.pieces, c.num_rows, c.counts, c.words64, c.last_id,
                              static_cast<float>(lr), c.lr_word, static_cast<float>(eps), CurrentStream(table));
}

// Extension (cuembed::SparseRowAdam): the sparse Adam step on a compressed gradient, in place on the table and both
// moments (exp_avg fp32 [rows, width]; exp_avg_sq the same, or fp32 [rows] with rowwise).  bias_factor is
// sqrt(1 - beta2^t) / (1 - beta1^t) of the step (1: no correction); lr_device / bias_factor_device: one fp32 device word
// read by the kernel instead.  The count sources and stochastic rounding are cuembed_sparse_row_update_'s.  1 - beta is
// formed in double and rounded once.  One launch, nothing read back.
void cuembed_sparse_row_adam_op(at::Tensor table, at::Tensor exp_avg, at::Tensor exp_avg_sq, const at::Tensor& ids,
                                const at::Tensor& rows, const bool rowwise, const double lr, const double bias_factor,
                                const double beta1, const double beta2, const double eps, const double weight_decay,
                                const c10::optional<at::Tensor>& lr_device,
                                const c10::optional<at::Tensor>& bias_factor_device, const int64_t count,
                                const c10::optional<at::Tensor>& counts, const c10::optional<at::Tensor>& last_id,
                                const int64_t piece_rows_arg, const bool stochastic_rounding, const int64_t seed,
                                const int64_t step, const c10::optional<at::Tensor>& step_device) {
  RowStep c = RowStepCodes(table, ids, rows);
  CheckRowStepShapes(table, ids, rows);
  TORCH_CHECK(exp_avg.defined() && exp_avg.is_cuda() && exp_avg.scalar_type() == at::kFloat && exp_avg.is_contiguous() &&
                  exp_avg.sizes() == table.sizes(),
              "cuembed_pyt: exp_avg must be a contiguous float32 GPU tensor of the table's shape");
  TORCH_CHECK(exp_avg_sq.defined() && exp_avg_sq.is_cuda() && exp_avg_sq.scalar_type() == at::kFloat &&
                  exp_avg_sq.is_contiguous() &&
                  (rowwise ? (exp_avg_sq.dim() == 1 && exp_avg_sq.size(0) == table.size(0))
                           : exp_avg_sq.sizes() == table.sizes()),
              "cuembed_pyt: exp_avg_sq must be a contiguous float32 GPU tensor, [rows, width] or, rowwise, [rows]");
  TORCH_CHECK(exp_avg.device() == table.device() && exp_avg_sq.device() == table.device(),
              "cuembed_pyt: exp_avg and exp_avg_sq must be on the table's device");
  // a lane moves at least 4 bytes of the table, so 4 / sizeof(element) moment words at a time
  const uintptr_t state_align = 4 * (4 / static_cast<uintptr_t>(table.element_size()));
  TORCH_CHECK(reinterpret_cast<uintptr_t>(exp_avg.data_ptr()) % state_align == 0, "cuembed_pyt: exp_avg must be ",
              state_align, "-byte aligned for a ", table.scalar_type(), " table");
  TORCH_CHECK(rowwise || reinterpret_cast<uintptr_t>(exp_avg_sq.data_ptr()) % state_align == 0,
              "cuembed_pyt: exp_avg_sq must be ", state_align, "-byte aligned for a ", table.scalar_type(), " table");
  TORCH_CHECK(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0, "cuembed_pyt: betas must lie in [0, 1)");
  TORCH_CHECK(eps >= 0.0 && weight_decay >= 0.0, "cuembed_pyt: eps and weight_decay must not be negative");
  ParseRowStepSources(c, table, ids, count, counts, last_id, piece_rows_arg, lr_device, &bias_factor_device,
                      stochastic_rounding, step_device);
  if (ids.numel() == 0) return;
  const at::DeviceGuard guard(table.device());
  const int rule = rowwise ? CUEMBED_ROWWISE_ADAM : CUEMBED_ADAM;
  float* m = static_cast<float*>(exp_avg.data_ptr());
  float* v = static_cast<float*>(exp_avg_sq.data_ptr());
  const float b1 = static_cast<float>(beta1), omb1 = static_cast<float>(1.0 - beta1);
  const float b2 = static_cast<float>(beta2), omb2 = static_cast<float>(1.0 - beta2);
  if (stochastic_rounding) {
    ::cuembed_sparse_row_adam_stochastic(
        table.data_ptr(), c.elem, static_cast<int>(table.size(1)), m, v, rule, Ptr(ids), c.idx, Ptr(rows), c.piece_rows,
        c.pieces, c.num_rows, c.counts, c.words64, c.last_id, static_cast<float>(lr), c.lr_word,
        static_cast<float>(bias_factor), c.bias_word, b1, omb1, b2, omb2, static_cast<float>(eps),
        static_cast<float>(weight_decay), static_cast<uint64_t>(seed), static_cast<uint64_t>(step), c.step_word,
        CurrentStream(table));
    return;
  }
  ::cuembed_sparse_row_adam(table.data_ptr(), c.elem, static_cast<int>(table.size(1)), m, v, rule, Ptr(ids), c.idx, Ptr(rows),
                            c.piece_rows, c.pieces, c.num_rows, c.counts, c.words64, c.last_id, static_cast<float>(lr),
                            c.lr_word, static_cast<float>(bias_factor), c.bias_word, b1, omb1, b2, omb2,
                            static_cast<float>(eps), static_cast<float>(weight_decay), CurrentStream(table));
}

// ---- the optimizer step on a group of SEPARATE table tensors, in one launch (cuembed::SparseRowUpdateGrouped /
// SparseRowAdamGrouped).  tables / table_ptrs as in cuemb_embedding_grouped; row_base the int64 device tensor of
// num_tables + 1 exclusive prefix sums of the row counts; ids GLOBAL rows of the tables laid end to end (the compressed
// gradient of the grouped backward), rows their gradient rows.  Each state list holds one float32 tensor per table and
// comes with the int64 device tensor of its base pointers, built once by the caller.  Valid entries, at most one of:
// count >= 0 (host-known), count_word (one int32 / int64 device word), last_id (one word of ids' dtype, count = last_id +
// 1); none: every entry.  stochastic_rounding = True (float16 / bfloat16 tables) takes `seeds`, the int64 device tensor
// [num_tables] that holds the bits of ONE unsigned 64-bit SEED PER TABLE, and the step, `step` or the one-element int64
// device tensor step_device: the bits of entry k are those of (seeds[t], step, row inside table t, column).  There are
// no default seeds: stochastic_rounding without seeds is refused, and so are seeds without it.  Nothing is read back.

struct GroupedStep {
  std::vector<const void*> table_host;
  int elem = CUEMBED_F32, idx = CUEMBED_I32, words64 = 0;
  int64_t num_rows = -1;
  const void* count_word = nullptr;
  const void* last_id = nullptr;
  const float* lr_word = nullptr;
  const uint64_t* seeds = nullptr;          // one per table, on the device: a stochastic step
  const int64_t* step_word = nullptr;
};

// One state list of a grouped step: `per_element` [rows_t, width] tensors, else [rows_t]; returns the host pointers.
std::vector<const void*> CheckGroupedStates(const at::TensorList tables, const at::TensorList states,
                                            const c10::optional<at::Tensor>& ptrs, const bool per_element, const char* name) {
  TORCH_CHECK(states.size() == tables.size(), "cuembed_pyt: ", name, " must hold one tensor per table");
  std::vector<const void*> host;
  for (size_t t = 0; t < tables.size(); ++t) {
    const at::Tensor& s = states[t];
    TORCH_CHECK(s.defined() && s.is_cuda() && s.device() == tables[0].device() && s.scalar_type() == at::kFloat &&
                    s.is_contiguous() &&
                    (per_element ? s.sizes() == tables[t].sizes() : (s.dim() == 1 && s.size(0) == tables[t].size(0))),
                "cuembed_pyt: ", name, "[", t, "] must be a contiguous float32 GPU tensor, ",
                per_element ? "of its table's shape" : "one word per row of its table");
    host.push_back(s.data_ptr());
  }
  TORCH_CHECK(ptrs.has_value() && ptrs->defined() && ptrs->is_cuda() && ptrs->device() == tables[0].device() &&
                  ptrs->scalar_type() == at::kLong && ptrs->is_contiguous() &&
                  ptrs->numel() == static_cast<int64_t>(tables.size()),
              "cuembed_pyt: ", name, " needs the contiguous int64 tensor of its data pointers on the tables' device");
  return host;
}

GroupedStep CheckGroupedStep(const at::TensorList tables, const at::Tensor& table_ptrs, const at::Tensor& row_base,
                             const at::Tensor& ids, const at::Tensor& rows, const c10::optional<at::Tensor>& lr_device,
                             const int64_t count, const c10::optional<at::Tensor>& count_word,
                             const c10::optional<at::Tensor>& last_id, const bool stochastic_rounding,
                             const c10::optional<at::Tensor>& seeds, const int64_t step,
                             const c10::optional<at::Tensor>& step_device) {
  GroupedStep c;
  const bool has_seeds = seeds.has_value() && seeds->defined();
  TORCH_CHECK(!stochastic_rounding || has_seeds,
              "cuembed_pyt: stochastic rounding on a grouped step takes one seed per table: pass seeds=[...]");
  TORCH_CHECK(stochastic_rounding || !has_seeds, "cuembed_pyt: seeds go with stochastic_rounding = True");
  const int64_t num_tables = static_cast<int64_t>(tables.size());
  TORCH_CHECK(num_tables >= 1 && num_tables <= 1023, "cuembed_pyt: a grouped step takes 1 to 1023 tables");
  c.elem = ElemCode(tables[0], "tables");
  if (stochastic_rounding) {
    TORCH_CHECK(c.elem != CUEMBED_F32,
                "cuembed_pyt: stochastic_rounding is for float16 / bfloat16 tables: a float32 table is not rounded");
    CheckGpu(*seeds, "seeds");
    TORCH_CHECK(seeds->scalar_type() == at::kLong && seeds->is_contiguous() && seeds->dim() == 1 &&
                    seeds->numel() == num_tables && seeds->device() == tables[0].device(),
                "cuembed_pyt: seeds must be the contiguous int64 tensor [num_tables] of the tables' seeds on their device");
    c.seeds = static_cast<const uint64_t*>(seeds->data_ptr());
    if (step_device.has_value() && step_device->defined()) {
      CheckGpu(*step_device, "step_device");
      TORCH_CHECK(step_device->scalar_type() == at::kLong && step_device->numel() == 1 &&
                      step_device->device() == tables[0].device(),
                  "cuembed_pyt: step_device must be one int64 word on the tables' device");
      c.step_word = static_cast<const int64_t*>(step_device->data_ptr());
    }
  }
  for (const at::Tensor& t : tables) {
    CheckGpu(t, "tables");
    TORCH_CHECK(t.dim() == 2 && t.is_contiguous() && t.scalar_type() == tables[0].scalar_type() &&
                    t.size(1) == tables[0].size(1) && t.device() == tables[0].device(),
                "cuembed_pyt: the tables of a group must be contiguous [rows, width] of one dtype, width and device");
    c.table_host.push_back(t.data_ptr());
  }
  const auto on_device = [&](const at::Tensor& t) { return t.is_cuda() && t.device() == tables[0].device(); };
  TORCH_CHECK(on_device(table_ptrs) && table_ptrs.scalar_type() == at::kLong && table_ptrs.is_contiguous() &&
                  table_ptrs.numel() == num_tables,
              "cuembed_pyt: table_ptrs must be the contiguous int64 tensor of the tables' data pointers on their device");
  TORCH_CHECK(on_device(row_base) && row_base.scalar_type() == at::kLong && row_base.is_contiguous() &&
                  row_base.numel() == num_tables + 1,
              "cuembed_pyt: row_base must be the contiguous int64 tensor of num_tables + 1 prefix sums on the tables' device");
  CheckGpu(ids, "ids");
  CheckGpu(rows, "rows");
  c.idx = IndexCode(ids, "ids");
  TORCH_CHECK(rows.scalar_type() == tables[0].scalar_type(), "cuembed_pyt: rows must have the tables' dtype");
  TORCH_CHECK(rows.dim() == 2 && rows.size(1) == tables[0].size(1) && ids.dim() == 1 && rows.size(0) == ids.numel() &&
                  rows.is_contiguous() && ids.is_contiguous() && on_device(ids) && on_device(rows),
              "cuembed_pyt: rows [entries, width] and ids [entries] must be contiguous, agree and be on the tables' device");
  TORCH_CHECK((rows.size(1) * rows.element_size()) % 4 == 0, "cuembed_pyt: the row size must be a multiple of 4 bytes");
  const bool has_word = count_word.has_value() && count_word->defined();
  const bool has_last = last_id.has_value() && last_id->defined();
  TORCH_CHECK((count >= 0) + has_word + has_last <= 1, "cuembed_pyt: give at most one of count, count_word and last_id");
  if (has_word) {
    CheckGpu(*count_word, "count_word");
    c.words64 = IndexCode(*count_word, "count_word") == CUEMBED_I64;
    TORCH_CHECK(count_word->numel() == 1 && on_device(*count_word), "cuembed_pyt: count_word must be one word on the tables' device");
    c.count_word = count_word->data_ptr();
  } else if (has_last) {
    CheckGpu(*last_id, "last_id");
    TORCH_CHECK(last_id->scalar_type() == ids.scalar_type() && last_id->numel() == 1 && on_device(*last_id),
                "cuembed_pyt: last_id must be one word of ids' dtype on the tables' device");
    c.last_id = last_id->data_ptr();
  } else {
    c.num_rows = count >= 0 ? count : ids.numel();
    TORCH_CHECK(c.num_rows <= ids.numel(), "cuembed_pyt: count exceeds the entries");
  }
  if (lr_device.has_value() && lr_device->defined()) {
    CheckGpu(*lr_device, "lr_device");
    TORCH_CHECK(lr_device->scalar_type() == at::kFloat && lr_device->numel() == 1 && on_device(*lr_device),
                "cuembed_pyt: lr_device must be one float32 word on the tables' device");
    c.lr_word = static_cast<const float*>(lr_device->data_ptr());
  }
  return c;
}

// The lane width the library will pick must exist: 4-byte aligned data, and per-element state that the narrowest lane
// (4 bytes of the row: 4 / sizeof(element) fp32 words) can move.
void CheckGroupedAlignment(const GroupedStep& c, const at::Tensor& rows, const int64_t element_size,
                           const std::vector<const std::vector<const void*>*>& per_element_states) {
  uintptr_t bits = reinterpret_cast<uintptr_t>(rows.data_ptr());
  for (const void* p : c.table_host) bits |= reinterpret_cast<uintptr_t>(p);
  TORCH_CHECK(bits % 4 == 0, "cuembed_pyt: tables and rows must be 4-byte aligned");
  const uintptr_t state_align = 4 * (4 / static_cast<uintptr_t>(element_size));
  for (const auto* host : per_element_states)
    for (const void* p : *host)
      TORCH_CHECK(reinterpret_cast<uintptr_t>(p) % state_align == 0, "cuembed_pyt: per-element state must be ", state_align,
                  "-byte aligned for tables of ", element_size, "-byte elements");
}

void cuembed_sparse_row_update_grouped_op(const at::TensorList tables, const at::Tensor& table_ptrs,
                                          const at::TensorList states, const c10::optional<at::Tensor>& state_ptrs,
                                          const at::Tensor& row_base, const at::Tensor& ids, const at::Tensor& rows,
                                          const std::string& rule, const double lr, const double eps,
                                          const c10::optional<at::Tensor>& lr_device, const int64_t count,
                                          const c10::optional<at::Tensor>& count_word,
                                          const c10::optional<at::Tensor>& last_id, const bool stochastic_rounding,
                                          const c10::optional<at::Tensor>& seeds, const int64_t step,
                                          const c10::optional<at::Tensor>& step_device) {
  const int code = rule == "sgd" ? CUEMBED_UPDATE_SGD
                   : rule == "adagrad" ? CUEMBED_UPDATE_ADAGRAD
                   : rule == "rowwise_adagrad" ? CUEMBED_UPDATE_ROWWISE_ADAGRAD : -1;
  TORCH_CHECK(code >= 0, "cuembed_pyt: rule must be 'sgd', 'adagrad' or 'rowwise_adagrad'");
  TORCH_CHECK(!tables.empty(), "cuembed_pyt: a group needs at least one table");
  const GroupedStep c =
      CheckGroupedStep(tables, table_ptrs, row_base, ids, rows, lr_device, count, count_word, last_id, stochastic_rounding,
                       seeds, step, step_device);
  std::vector<const void*> state_host;
  if (code == CUEMBED_UPDATE_SGD) {
    TORCH_CHECK(states.empty(), "cuembed_pyt: rule 'sgd' takes no states");
  } else {
    state_host = CheckGroupedStates(tables, states, state_ptrs, code == CUEMBED_UPDATE_ADAGRAD, "states");
  }
  std::vector<const std::vector<const void*>*> per_element;
  if (code == CUEMBED_UPDATE_ADAGRAD) per_element.push_back(&state_host);
  CheckGroupedAlignment(c, rows, tables[0].element_size(), per_element);
  if (ids.numel() == 0) return;
  const at::DeviceGuard guard(tables[0].device());
  const bool stateful = code != CUEMBED_UPDATE_SGD;
  if (stochastic_rounding) {
    ::cuembed_sparse_row_update_grouped_stochastic(
        c.table_host.data(), static_cast<const void* const*>(table_ptrs.data_ptr()),
        stateful ? state_host.data() : nullptr,
        stateful ? static_cast<const void* const*>(state_ptrs->data_ptr()) : nullptr, static_cast<int>(tables.size()),
        c.elem, static_cast<int>(rows.size(1)), static_cast<const int64_t*>(row_base.data_ptr()), code, Ptr(ids), c.idx,
        Ptr(rows), ids.numel(), c.num_rows, c.count_word, c.words64, c.last_id, static_cast<float>(lr), c.lr_word,
        static_cast<float>(eps), c.seeds, static_cast<uint64_t>(step), c.step_word, CurrentStream(rows));
    return;
  }
  ::cuembed_sparse_row_update_grouped(
      c.table_host.data(), static_cast<const void* const*>(table_ptrs.data_ptr()), stateful ? state_host.data() : nullptr,
      stateful ? static_cast<const void* const*>(state_ptrs->data_ptr()) : nullptr, static_cast<int>(tables.size()),
      c.elem, static_cast<int>(rows.size(1)), static_cast<const int64_t*>(row_base.data_ptr()), code, Ptr(ids), c.idx,
      Ptr(rows), ids.numel(), c.num_rows, c.count_word, c.words64, c.last_id, static_cast<float>(lr), c.lr_word,
      static_cast<float>(eps), CurrentStream(rows));
}

void cuembed_sparse_row_adam_grouped_op(const at::TensorList tables, const at::Tensor& table_ptrs,
                                        const at::TensorList exp_avg, const at::Tensor& exp_avg_ptrs,
                                        const at::TensorList exp_avg_sq, const at::Tensor& exp_avg_sq_ptrs,
                                        const at::Tensor& row_base, const at::Tensor& ids, const at::Tensor& rows,
                                        const bool rowwise, const double lr, const double bias_factor, const double beta1,
                                        const double beta2, const double eps, const double weight_decay,
                                        const c10::optional<at::Tensor>& lr_device,
                                        const c10::optional<at::Tensor>& bias_factor_device, const int64_t count,
                                        const c10::optional<at::Tensor>& count_word,
                                        const c10::optional<at::Tensor>& last_id, const bool stochastic_rounding,
                                        const c10::optional<at::Tensor>& seeds, const int64_t step,
                                        const c10::optional<at::Tensor>& step_device) {
  TORCH_CHECK(!tables.empty(), "cuembed_pyt: a group needs at least one table");
  const GroupedStep c =
      CheckGroupedStep(tables, table_ptrs, row_base, ids, rows, lr_device, count, count_word, last_id, stochastic_rounding,
                       seeds, step, step_device);
  const std::vector<const void*> m_host = CheckGroupedStates(tables, exp_avg, exp_avg_ptrs, true, "exp_avg");
  const std::vector<const void*> v_host = CheckGroupedStates(tables, exp_avg_sq, exp_avg_sq_ptrs, !rowwise, "exp_avg_sq");
  std::vector<const std::vector<const void*>*> per_element = {&m_host};
  if (!rowwise) per_element.push_back(&v_host);
  CheckGroupedAlignment(c, rows, tables[0].element_size(), per_element);
  TORCH_CHECK(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0, "cuembed_pyt: betas must lie in [0, 1)");
  TORCH_CHECK(eps >= 0.0 && weight_decay >= 0.0, "cuembed_pyt: eps and weight_decay must not be negative");
  const float* bias_word = nullptr;
  if (bias_factor_device.has_value() && bias_factor_device->defined()) {
    CheckGpu(*bias_factor_device, "bias_factor_device");
    TORCH_CHECK(bias_factor_device->scalar_type() == at::kFloat && bias_factor_device->numel() == 1 &&
                    bias_factor_device->device() == tables[0].device(),
                "cuembed_pyt: bias_factor_device must be one float32 word on the tables' device");
    bias_word = static_cast<const float*>(bias_factor_device->data_ptr());
  }
  if (ids.numel() == 0) return;
  const at::DeviceGuard guard(tables[0].device());
  if (stochastic_rounding) {
    ::cuembed_sparse_row_adam_grouped_stochastic(
        c.table_host.data(), static_cast<const void* const*>(table_ptrs.data_ptr()), m_host.data(),
        static_cast<const void* const*>(exp_avg_ptrs.data_ptr()), v_host.data(),
        static_cast<const void* const*>(exp_avg_sq_ptrs.data_ptr()), static_cast<int>(tables.size()), c.elem,
        static_cast<int>(rows.size(1)), static_cast<const int64_t*>(row_base.data_ptr()),
        rowwise ? CUEMBED_ROWWISE_ADAM : CUEMBED_ADAM, Ptr(ids), c.idx, Ptr(rows), ids.numel(), c.num_rows, c.count_word,
        c.words64, c.last_id, static_cast<float>(lr), c.lr_word, static_cast<float>(bias_factor), bias_word,
        static_cast<float>(beta1), static_cast<float>(1.0 - beta1), static_cast<float>(beta2),
        static_cast<float>(1.0 - beta2), static_cast<float>(eps), static_cast<float>(weight_decay), c.seeds,
        static_cast<uint64_t>(step), c.step_word, CurrentStream(rows));
    return;
  }
  ::cuembed_sparse_row_adam_grouped(
      c.table_host.data(), static_cast<const void* const*>(table_ptrs.data_ptr()), m_host.data(),
      static_cast<const void* const*>(exp_avg_ptrs.data_ptr()), v_host.data(),
      static_cast<const void* const*>(exp_avg_sq_ptrs.data_ptr()), static_cast<int>(tables.size()), c.elem,
      static_cast<int>(rows.size(1)), static_cast<const int64_t*>(row_base.data_ptr()),
      rowwise ? CUEMBED_ROWWISE_ADAM : CUEMBED_ADAM, Ptr(ids), c.idx, Ptr(rows), ids.numel(), c.num_rows, c.count_word,
      c.words64, c.last_id, static_cast<float>(lr), c.lr_word, static_cast<float>(bias_factor), bias_word,
      static_cast<float>(beta1), static_cast<float>(1.0 - beta1), static_cast<float>(beta2),
      static_cast<float>(1.0 - beta2), static_cast<float>(eps), static_cast<float>(weight_decay), CurrentStream(rows));
}

// Extension (cuembed::PackRowsByOwner): the rank's compressed gradient into the fixed slots of the all-to-all.
void cuembed_exchange_pack_op(const at::Tensor& ids, const at::Tensor& rows, const c10::optional<at::Tensor>& count,
                              const at::Tensor& cuts, const int64_t slot_capacity, const int64_t input_capacity,
                              const int64_t num_categories, at::Tensor send_ids, at::Tensor send_rows,
                              at::Tensor range_starts, at::Tensor flag) {
  CheckGpu(ids, "ids");
  CheckGpu(rows, "rows");
  CheckGpu(cuts, "cuts");
  CheckGpu(send_ids, "send_ids");
  CheckGpu(send_rows, "send_rows");
  CheckGpu(range_starts, "range_starts");
  CheckGpu(flag, "flag");
  const int idx = IndexCode(ids, "ids");
  const int elem = ElemCode(rows, "rows");
  TORCH_CHECK(rows.dim() == 2 && ids.dim() == 1 && rows.size(0) == ids.numel() && ids.is_contiguous() && rows.is_contiguous(),
              "cuembed_pyt: rows must be a contiguous [n, width] tensor with one contiguous id per row");
  const int64_t world = cuts.numel() - 1;
  TORCH_CHECK(world >= 1 && world <= 1024 && cuts.scalar_type() == at::kLong && cuts.is_contiguous(),
              "cuembed_pyt: cuts must be world + 1 contiguous int64 words (world <= 1024)");
  TORCH_CHECK(slot_capacity >= 1, "cuembed_pyt: slot_capacity must be at least one row");
  TORCH_CHECK(send_ids.scalar_type() == at::kLong && send_ids.is_contiguous() && send_ids.numel() == world * slot_capacity,
              "cuembed_pyt: send_ids must be world * slot_capacity contiguous int64 words");
  TORCH_CHECK(send_rows.scalar_type() == rows.scalar_type() && send_rows.is_contiguous() &&
                  send_rows.numel() == world * slot_capacity * rows.size(1),
              "cuembed_pyt: send_rows must be a contiguous [world * slot_capacity, width] tensor of rows' dtype");
  TORCH_CHECK(range_starts.scalar_type() == at::kLong && range_starts.is_contiguous() && range_starts.numel() >= world + 1,
              "cuembed_pyt: range_starts must hold world + 1 contiguous int64 words");
  TORCH_CHECK(flag.scalar_type() == at::kLong && flag.numel() >= 1 && flag.is_contiguous(),
              "cuembed_pyt: flag must be a contiguous int64 word");
  const at::DeviceGuard guard(rows.device());
  at::Tensor cnt;
  if (count.has_value() && count->defined()) {
    CheckGpu(*count, "count");
    TORCH_CHECK(count->numel() >= 1, "cuembed_pyt: count must hold one word");
    // (one word, read by the kernel: a count of the other integer type is converted here, one tiny launch)
    cnt = count->scalar_type() == ids.scalar_type() ? count->contiguous() : count->to(ids.scalar_type());
  }
  ::cuembed_exchange_pack_rows(Ptr(ids), idx, Ptr(rows), elem, ids.numel(), static_cast<int>(rows.size(1)), Ptr(cnt),
                               static_cast<const int64_t*>(cuts.data_ptr()), static_cast<int>(world), slot_capacity,
                               input_capacity, num_categories, static_cast<int64_t*>(send_ids.data_ptr()),
                               send_rows.data_ptr(), static_cast<int64_t*>(range_starts.data_ptr()),
                               static_cast<int64_t*>(flag.data_ptr()), CurrentStream(rows));
}

// Extension: the owner's fixed-capacity merge -- TransposeFixedHotness (+ remap) of the received ids, EmbeddingBackward
// with a device-side row count and pad_to_capacity into out_ids[capacity + 1] / out_rows[capacity + 1, width],
// cuembed::FinishOwnerPiece -- as one op.  ids >= num_categories are padding and dropped.  `tail`: capacity + 2 words
// (the ids, the count, the flag word), `count`: one word; either may be absent.
void cuembed_exchange_merge_op(const at::Tensor& ids, const at::Tensor& rows, const int64_t num_categories,
                               const int64_t pad_lo, const int64_t pad_len, at::Tensor out_ids, at::Tensor out_rows,
                               const c10::optional<at::Tensor>& tail, at::Tensor flag,
                               const c10::optional<at::Tensor>& count) {
  CheckGpu(ids, "ids");
  CheckGpu(rows, "rows");
  CheckGpu(out_ids, "out_ids");
  CheckGpu(out_rows, "out_rows");
  CheckGpu(flag, "flag");
  const int elem = ElemCode(rows, "rows");
  const int64_t nnz = ids.numel();
  TORCH_CHECK(ids.scalar_type() == at::kLong && ids.is_contiguous() && nnz >= 1 && nnz <= INT32_MAX,
              "cuembed_pyt: ids must be 1 .. 2^31 - 1 contiguous int64 words");
  TORCH_CHECK(rows.dim() == 2 && rows.size(0) == nnz && rows.is_contiguous(),
              "cuembed_pyt: rows must be a contiguous [n, width] tensor with one id per row");
  const int64_t width = rows.size(1);
  const int64_t capacity = out_ids.numel() - 1;
  TORCH_CHECK(capacity >= 1 && capacity < INT32_MAX && out_ids.scalar_type() == at::kLong && out_ids.is_contiguous(),
              "cuembed_pyt: out_ids must be capacity + 1 contiguous int64 words");
  TORCH_CHECK(out_rows.scalar_type() == rows.scalar_type() && out_rows.is_contiguous() && out_rows.dim() == 2 &&
                  out_rows.size(0) == capacity + 1 && out_rows.size(1) == width,
              "cuembed_pyt: out_rows must be a contiguous [capacity + 1, width] tensor of rows' dtype");
  TORCH_CHECK(flag.scalar_type() == at::kLong && flag.numel() >= 1 && flag.is_contiguous(),
              "cuembed_pyt: flag must be a contiguous int64 word");
  TORCH_CHECK(pad_len >= 1, "cuembed_pyt: pad_len must be at least 1");
  int64_t* tail_ptr = nullptr;
  if (tail.has_value() && tail->defined()) {
    CheckGpu(*tail, "tail");
    TORCH_CHECK(tail->scalar_type() == at::kLong && tail->is_contiguous() && tail->numel() == capacity + 2,
                "cuembed_pyt: tail must be capacity + 2 contiguous int64 words");
    tail_ptr = static_cast<int64_t*>(tail->data_ptr());
  }
  int64_t* count_ptr = nullptr;
  if (count.has_value() && count->defined()) {
    CheckGpu(*count, "count");
    TORCH_CHECK(count->scalar_type() == at::kLong && count->numel() >= 1 && count->is_contiguous(),
                "cuembed_pyt: count must be a contiguous int64 word");
    count_ptr = static_cast<int64_t*>(count->data_ptr());
  }
  CheckRowAlignment("rows / out_rows", width, rows.element_size(), {Ptr(rows), out_rows.data_ptr()}, true);
  const at::DeviceGuard guard(rows.device());
  const cuembed_stream_t stream = CurrentStream(rows);
  at::Tensor t_idx = at::empty_like(ids), t_pos = at::empty_like(ids), remap = at::empty_like(ids);
  size_t lwork = 0;
  const int bits = IndexBits(num_categories + 1);   // the padding id num_categories is a key too
  ::cuembed_transpose_fixed_hotness_remapped(nullptr, nullptr, static_cast<int>(nnz), 1, CUEMBED_I64, CUEMBED_F32, nullptr,
                                             nullptr, nullptr, nullptr, nullptr, &lwork, bits, 1, nullptr);
  at::Tensor work = at::empty({static_cast<int64_t>(lwork > 0 ? lwork : 1)}, ids.options().dtype(at::kByte));
  ::cuembed_transpose_fixed_hotness_remapped(Ptr(ids), nullptr, static_cast<int>(nnz), 1, CUEMBED_I64, CUEMBED_F32,
                                             MutPtr(t_idx), MutPtr(t_pos), nullptr, MutPtr(remap),
                                             static_cast<char*>(work.data_ptr()), &lwork, bits, 1, stream);
  // capacity + 1 rows: the run of the padding ids needs a row too; too many distinct ids -> the kernels write nothing
  ::cuembed_embedding_backward_bounded(Ptr(rows), elem, static_cast<int>(width), -1, static_cast<int>(nnz), Ptr(t_idx),
                                       Ptr(t_pos), Ptr(remap), CUEMBED_I64, nullptr, /*skip_grad_init=*/0,
                                       out_rows.data_ptr(), out_ids.data_ptr(), 1, nullptr,
                                       static_cast<int>(capacity + 1), nullptr, /*pad_to_capacity=*/1, stream);
  ::cuembed_exchange_finish_piece(static_cast<const int64_t*>(t_idx.data_ptr()),
                                  static_cast<const int64_t*>(remap.data_ptr()), nnz, capacity, num_categories, pad_lo,
                                  pad_len, static_cast<int64_t*>(out_ids.data_ptr()), out_rows.data_ptr(), elem,
                                  static_cast<int>(width), tail_ptr, static_cast<int64_t*>(flag.data_ptr()), count_ptr,
                                  stream);
}

// grad_kind: see GradKind.
at::Tensor cuemb_embedding_autograd_op(const at::Tensor& params, const at::Tensor& indices, const at::Tensor& offsets,
                                    const at::Tensor& weights, const int64_t grad_kind, const int64_t row_loads,
                                    const at::Tensor& sample_order, const at::Tensor& row_loads_device) {
  TORCH_CHECK(grad_kind >= kGradDense && grad_kind <= kGradSparsePadded, "cuembed_pyt: unknown grad_kind");
  return CuEmbEmbeddingNode::apply(params, indices, offsets,
                                   weights.defined() ? c10::optional<at::Tensor>(weights) : c10::nullopt, grad_kind,
                                   row_loads,
                                   sample_order.defined() ? c10::optional<at::Tensor>(sample_order) : c10::nullopt,
                                   row_loads_device.defined() ? c10::optional<at::Tensor>(row_loads_device) : c10::nullopt);
}

// ---- 8-bit row-wise quantized tables (extension; inference only).  The format is torch's own fused layout
// (quantized::embedding_bag_byte_prepack): uint8 [rows, W + 8], codes, fp32 scale, fp32 bias. -------------------------

int OutCode(const at::ScalarType t, const char* what) {
  TORCH_CHECK(t == at::kFloat || t == at::kHalf, "cuembed_pyt: ", what, " must be float32 or float16");
  return t == at::kFloat ? CUEMBED_F32 : CUEMBED_F16;
}

int64_t QuantizedWidth(const at::Tensor& qtable) {
  CheckGpu(qtable, "qtable");
  TORCH_CHECK(qtable.scalar_type() == at::kByte && qtable.dim() == 2 && qtable.is_contiguous(),
              "cuembed_pyt: qtable must be a contiguous 2-D uint8 tensor [rows, width + 8]");
  const int64_t width = qtable.size(1) - 8;
  TORCH_CHECK(width > 0 && width % 4 == 0, "cuembed_pyt: row size must be a multiple of 4 bytes");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(qtable.data_ptr()) % 4 == 0, "cuembed_pyt: qtable must be 4-byte aligned");
  return width;
}

// ... and what DequantizeRows / PlanQuantizedForward would abort on: more than 1,024 lanes of QuantizedCodesPerLane codes
void CheckQuantizedLanes(const at::Tensor& qtable, const int64_t width) {
  const int64_t codes = (width % 8 == 0 && reinterpret_cast<uintptr_t>(qtable.data_ptr()) % 8 == 0) ? 8 : 4;
  TORCH_CHECK(width / codes <= 1024, "cuembed_pyt: qtable: a row of ", width, " codes needs ", width / codes, " lanes of ",
              codes, " bytes, more than 1024; align the table to 8 bytes");
}

at::Tensor quantize_rows_op(const at::Tensor& table) {
  CheckGpu(table, "table");
  const int elem = ElemCode(table, "table");
  TORCH_CHECK(table.dim() == 2 && table.size(1) > 0 && table.size(1) % 4 == 0,
              "cuembed_pyt: table must be [rows, width] with a width that is a multiple of 4");
  const at::DeviceGuard guard(table.device());
  const at::Tensor t = table.contiguous();
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, "cuembed_pyt: table must be 16-byte aligned");
  at::Tensor out = at::empty({t.size(0), t.size(1) + 8}, t.options().dtype(at::kByte));
  if (t.size(0) > 0)
    ::cuembed_quantize_rows(Ptr(t), elem, static_cast<int>(t.size(1)), t.size(0), MutPtr(out), CurrentStream(t));
  return out;
}

at::Tensor dequantize_rows_op(const at::Tensor& qtable, const c10::optional<at::Tensor>& ids, const at::ScalarType dtype) {
  const int64_t width = QuantizedWidth(qtable);
  CheckQuantizedLanes(qtable, width);
  const int out_code = OutCode(dtype, "dtype");
  const at::DeviceGuard guard(qtable.device());
  at::Tensor i;
  int idx = CUEMBED_I32;
  std::vector<int64_t> shape{qtable.size(0), width};
  if (ids.has_value() && ids->defined()) {
    CheckGpu(*ids, "ids");
    idx = IndexCode(*ids, "ids");
    i = ids->contiguous();
    shape = i.sizes().vec();
    shape.push_back(width);
  }
  at::Tensor out = at::empty(shape, qtable.options().dtype(dtype));
  const int64_t n = i.defined() ? i.numel() : qtable.size(0);
  if (n > 0)
    ::cuembed_dequantize_rows(Ptr(qtable), static_cast<int>(width), Ptr(i), idx, n, MutPtr(out), out_code,
                              CurrentStream(qtable));
  return out;
}

// offsets given: CSR (batch + 1 entries); absent: fixed hotness, indices is [batch, hotness].
at::Tensor cuemb_embedding_quantized_op(const at::Tensor& qtable, const at::Tensor& indices,
                                        const c10::optional<at::Tensor>& offsets, const c10::optional<at::Tensor>& weights,
                                        const std::string& mode, const at::ScalarType out_dtype, const int64_t row_loads,
                                        const c10::optional<at::Tensor>& sample_order,
                                        const c10::optional<at::Tensor>& row_loads_device) {
  const int64_t width = QuantizedWidth(qtable);
  CheckQuantizedLanes(qtable, width);
  const int out_code = OutCode(out_dtype, "out_dtype");
  CheckGpu(indices, "indices");
  const int idx = IndexCode(indices, "indices");
  const bool csr = offsets.has_value() && offsets->defined();
  const int m = Mode(mode, !csr);
  TORCH_CHECK(row_loads >= -1 && row_loads <= 1, "cuembed_pyt: row_loads must be -1, 0 or 1");
  const at::DeviceGuard guard(qtable.device());
  const at::Tensor i = indices.contiguous();
  at::Tensor o, w, order, decision;
  int off = CUEMBED_I32;
  int64_t batch = 0, hot = 0;
  if (csr) {
    CheckGpu(*offsets, "offsets");
    off = IndexCode(*offsets, "offsets");
    o = offsets->contiguous();
    batch = o.numel() - 1;
    TORCH_CHECK(batch >= 0, "cuembed_pyt: offsets must hold batch_size + 1 entries");
  } else {
    TORCH_CHECK(i.dim() == 2 && i.size(1) > 0, "cuembed_pyt: without offsets, indices must be [batch, hotness]");
    batch = i.size(0);
    hot = i.size(1);
  }
  if (weights.has_value() && weights->defined()) {
    CheckGpu(*weights, "weights");
    TORCH_CHECK(m != CUEMBED_CONCAT, "cuembed_pyt: concat does not take weights");
    TORCH_CHECK(weights->scalar_type() == out_dtype, "cuembed_pyt: weights must have the output's dtype");
    TORCH_CHECK(weights->numel() >= i.numel(), "cuembed_pyt: weights must have one entry per index");
    w = weights->contiguous();
  }
  if (sample_order.has_value() && sample_order->defined()) {
    order = *sample_order;
    TORCH_CHECK(csr && order.is_cuda() && order.scalar_type() == at::kInt && order.numel() == batch && order.is_contiguous(),
                "cuembed_pyt: sample_order (CSR only) must be a contiguous int32 permutation of the samples on the GPU");
  }
  if (row_loads_device.has_value() && row_loads_device->defined()) {
    decision = *row_loads_device;
    TORCH_CHECK(decision.is_cuda() && decision.scalar_type() == at::kInt && decision.numel() >= 4 && decision.is_contiguous(),
                "cuembed_pyt: row_loads_device must be the contiguous 4-word int32 tensor of cuembed_decide_row_loads");
  }
  at::Tensor out = m == CUEMBED_CONCAT ? at::empty({batch, hot, width}, qtable.options().dtype(out_dtype))
                                       : at::empty({batch, width}, qtable.options().dtype(out_dtype));
  if (batch > 0)
    ::cuembed_embedding_forward_quantized(Ptr(qtable), static_cast<int>(width), Ptr(i), idx, Ptr(o), off, Ptr(w),
                                          static_cast<int>(batch), static_cast<int>(hot), m, MutPtr(out), out_code,
                                          static_cast<int>(row_loads), static_cast<const int32_t*>(Ptr(order)),
                                          static_cast<const uint32_t*>(Ptr(decision)), CurrentStream(qtable));
  return out;
}

// ---- a GROUP of tables pooled in one launch (extension; forward only: no autograd formula).  `tables` keeps the
// tensors (and gives the host copy of their base pointers, which the library reads for the access width); `table_ptrs`
// is the caller's int64 device tensor of the same pointers, built once (cuembed_amd.TableGroup), which the kernel reads.
// offsets given: CSR, num_tables * batch + 1 entries; absent: fixed hotness, indices is [num_tables, batch, hotness].
// Returns [batch, num_tables, width].

struct GroupedCall {
  std::vector<const void*> host_ptrs;
  at::Tensor i, o, w, order;
  int idx = CUEMBED_I32, off = CUEMBED_I32;
  int64_t batch = 0, hot = 0;
};

// The tables of a group and the device tensor of their pointers.  one_width: a same-width group; else any widths, every
// row a multiple of 4 bytes.  Returns the host copy of the base pointers.
std::vector<const void*> CheckGroupTables(const at::TensorList tables, const at::Tensor& table_ptrs, const bool one_width) {
  std::vector<const void*> host_ptrs;
  const int64_t num_tables = static_cast<int64_t>(tables.size());
  TORCH_CHECK(num_tables >= 1, "cuembed_pyt: a group needs at least one table");
  for (const at::Tensor& t : tables) {
    CheckGpu(t, "tables");
    TORCH_CHECK(t.dim() == 2 && t.is_contiguous() && t.scalar_type() == tables[0].scalar_type() &&
                    t.device() == tables[0].device() &&
                    (one_width ? t.size(1) == tables[0].size(1) : t.size(1) > 0 && (t.size(1) * t.element_size()) % 4 == 0),
                one_width
                    ? "cuembed_pyt: the tables of a group must be contiguous [rows, width] of one dtype, width and device"
                    : "cuembed_pyt: the tables of a mixed-width group must be contiguous [rows, width] of one dtype and "
                      "device, every row a multiple of 4 bytes");
    TORCH_CHECK(!(at::GradMode::is_enabled() && t.requires_grad()),
                "cuembed_pyt: a table requires grad: the grouped forward is forward only");
    host_ptrs.push_back(t.data_ptr());
  }
  TORCH_CHECK(table_ptrs.is_cuda() && table_ptrs.device() == tables[0].device() && table_ptrs.scalar_type() == at::kLong &&
                  table_ptrs.is_contiguous() && table_ptrs.numel() == num_tables,
              "cuembed_pyt: table_ptrs must be the contiguous int64 tensor of the tables' data pointers on their device");
  return host_ptrs;
}

// The batch of a grouped call -- indices / offsets / weights / sample_order -- into `c`: CSR xor fixed hotness, the batch
// size, and the contiguous tensors.
void CheckGroupedBatch(GroupedCall* c, const int64_t num_tables, const at::Tensor& indices,
                       const c10::optional<at::Tensor>& offsets, const c10::optional<at::Tensor>& weights,
                       const at::ScalarType weight_type, const int64_t row_loads,
                       const c10::optional<at::Tensor>& sample_order) {
  CheckGpu(indices, "indices");
  c->idx = IndexCode(indices, "indices");
  TORCH_CHECK(row_loads >= -1 && row_loads <= 1, "cuembed_pyt: row_loads must be -1, 0 or 1");
  c->i = indices.contiguous();
  const bool csr = offsets.has_value() && offsets->defined();
  if (csr) {
    CheckGpu(*offsets, "offsets");
    c->off = IndexCode(*offsets, "offsets");
    c->o = offsets->contiguous();
    TORCH_CHECK(c->o.numel() >= 1 && (c->o.numel() - 1) % num_tables == 0,
                "cuembed_pyt: offsets must hold num_tables * batch_size + 1 entries");
    c->batch = (c->o.numel() - 1) / num_tables;
  } else {
    TORCH_CHECK(c->i.dim() == 3 && c->i.size(0) == num_tables && c->i.size(2) > 0,
                "cuembed_pyt: without offsets, indices must be [num_tables, batch, hotness]");
    c->batch = c->i.size(1);
    c->hot = c->i.size(2);
  }
  TORCH_CHECK(num_tables * c->batch <= INT32_MAX, "cuembed_pyt: num_tables * batch_size must fit a 32-bit int");
  if (weights.has_value() && weights->defined()) {
    CheckGpu(*weights, "weights");
    TORCH_CHECK(weights->scalar_type() == weight_type, "cuembed_pyt: weights have the wrong dtype");
    TORCH_CHECK(weights->numel() >= c->i.numel(), "cuembed_pyt: weights must have one entry per index");
    c->w = weights->contiguous();
  }
  if (sample_order.has_value() && sample_order->defined()) {
    c->order = *sample_order;
    TORCH_CHECK(csr && c->order.is_cuda() && c->order.scalar_type() == at::kInt &&
                    c->order.numel() == num_tables * c->batch && c->order.is_contiguous(),
                "cuembed_pyt: sample_order (CSR only) must be a contiguous int32 permutation of the bags on the GPU");
  }
}

// Both, for a same-width group.
GroupedCall CheckGroupedCall(const at::TensorList tables, const at::Tensor& table_ptrs, const at::Tensor& indices,
                             const c10::optional<at::Tensor>& offsets, const c10::optional<at::Tensor>& weights,
                             const at::ScalarType weight_type, const int64_t row_loads,
                             const c10::optional<at::Tensor>& sample_order) {
  GroupedCall c;
  c.host_ptrs = CheckGroupTables(tables, table_ptrs, true);
  CheckGroupedBatch(&c, static_cast<int64_t>(tables.size()), indices, offsets, weights, weight_type, row_loads,
                    sample_order);
  return c;
}

int GroupedMode(const std::string& mode) {
  TORCH_CHECK(mode == "sum" || mode == "mean", "cuembed_pyt: mode must be 'sum' or 'mean'");
  return mode == "sum" ? CUEMBED_SUM : CUEMBED_MEAN;
}

at::Tensor cuemb_embedding_grouped_op(const at::TensorList tables, const at::Tensor& table_ptrs, const at::Tensor& indices,
                                      const c10::optional<at::Tensor>& offsets, const c10::optional<at::Tensor>& weights,
                                      const std::string& mode, const int64_t row_loads,
                                      const c10::optional<at::Tensor>& sample_order) {
  const int m = GroupedMode(mode);
  TORCH_CHECK(!tables.empty(), "cuembed_pyt: a group needs at least one table");
  const int elem = ElemCode(tables[0], "tables");
  const at::DeviceGuard guard(tables[0].device());
  const GroupedCall c =
      CheckGroupedCall(tables, table_ptrs, indices, offsets, weights, tables[0].scalar_type(), row_loads, sample_order);
  const int64_t num_tables = static_cast<int64_t>(tables.size()), width = tables[0].size(1);
  at::Tensor out = at::empty({c.batch, num_tables, width}, tables[0].options());
  uintptr_t bits = 0;
  for (const void* p : c.host_ptrs) bits |= reinterpret_cast<uintptr_t>(p);
  CheckRowAlignment("tables", width, tables[0].element_size(), {reinterpret_cast<const void*>(bits), Ptr(out)}, true);
  if (c.batch > 0)
    ::cuembed_embedding_forward_grouped(c.host_ptrs.data(), static_cast<const void* const*>(table_ptrs.data_ptr()),
                                        static_cast<int>(num_tables), elem, static_cast<int>(width), Ptr(c.i), c.idx,
                                        Ptr(c.o), c.off, Ptr(c.w), static_cast<int>(c.batch), static_cast<int>(c.hot), m,
                                        MutPtr(out), static_cast<int>(row_loads),
                                        static_cast<const int32_t*>(Ptr(c.order)), CurrentStream(out));
  return out;
}

at::Tensor cuemb_embedding_quantized_grouped_op(const at::TensorList qtables, const at::Tensor& table_ptrs,
                                                const at::Tensor& indices, const c10::optional<at::Tensor>& offsets,
                                                const c10::optional<at::Tensor>& weights, const std::string& mode,
                                                const at::ScalarType out_dtype, const int64_t row_loads,
                                                const c10::optional<at::Tensor>& sample_order) {
  const int m = GroupedMode(mode);
  TORCH_CHECK(!qtables.empty(), "cuembed_pyt: a group needs at least one table");
  const int out_code = OutCode(out_dtype, "out_dtype");
  int64_t width = 0;
  uintptr_t bits = 0;
  for (const at::Tensor& t : qtables) {
    width = QuantizedWidth(t);
    bits |= reinterpret_cast<uintptr_t>(t.data_ptr());
  }
  TORCH_CHECK(width / ((width % 8 == 0 && bits % 8 == 0) ? 8 : 4) <= 1024,
              "cuembed_pyt: qtables: a row of ", width, " codes needs more than 1024 lanes; align the tables to 8 bytes");
  const at::DeviceGuard guard(qtables[0].device());
  const GroupedCall c = CheckGroupedCall(qtables, table_ptrs, indices, offsets, weights, out_dtype, row_loads, sample_order);
  const int64_t num_tables = static_cast<int64_t>(qtables.size());
  at::Tensor out = at::empty({c.batch, num_tables, width}, qtables[0].options().dtype(out_dtype));
  if (c.batch > 0)
    ::cuembed_embedding_forward_quantized_grouped(
        c.host_ptrs.data(), static_cast<const void* const*>(table_ptrs.data_ptr()), static_cast<int>(num_tables),
        static_cast<int>(width), Ptr(c.i), c.idx, Ptr(c.o), c.off, Ptr(c.w), static_cast<int>(c.batch),
        static_cast<int>(c.hot), m, MutPtr(out), out_code, static_cast<int>(row_loads),
        static_cast<const int32_t*>(Ptr(c.order)), CurrentStream(out));
  return out;
}

// ---- a group of tables of DIFFERENT widths pooled in one launch (extension; forward only: no autograd formula).
// tables / table_ptrs / idx / offsets / weights as in cuemb_embedding_grouped, except that the widths may differ (plain
// tables only).  `descriptor` is the caller's int32 device tensor of (num_tables + 1) * 4 words, filled on the host by
// cuembed_fill_mixed_group_descriptor for this batch and `lane_bytes` and copied to the device once
// (cuembed_amd.MixedTableGroup.descriptor); lane_bytes is checked here against the pointers, the words cannot be.
// Returns [batch, sum of the widths]: the per-table results concatenated on dim 1.
at::Tensor cuemb_embedding_mixed_group_op(const at::TensorList tables, const at::Tensor& table_ptrs,
                                          const at::Tensor& descriptor, const int64_t lane_bytes, const at::Tensor& indices,
                                          const c10::optional<at::Tensor>& offsets,
                                          const c10::optional<at::Tensor>& weights, const std::string& mode,
                                          const int64_t row_loads) {
  const int m = GroupedMode(mode);
  const int64_t num_tables = static_cast<int64_t>(tables.size());
  TORCH_CHECK(num_tables >= 1, "cuembed_pyt: a group needs at least one table");
  const int elem = ElemCode(tables[0], "tables");
  const at::DeviceGuard guard(tables[0].device());
  GroupedCall c;
  c.host_ptrs = CheckGroupTables(tables, table_ptrs, false);
  std::vector<int> widths;
  int64_t dim = 0;
  uintptr_t bits = 0;
  for (const at::Tensor& t : tables) {
    widths.push_back(static_cast<int>(t.size(1)));
    dim += t.size(1);
    bits |= reinterpret_cast<uintptr_t>(t.data_ptr());
  }
  TORCH_CHECK(dim <= INT32_MAX, "cuembed_pyt: the widths must sum to at most 2^31 - 1");
  TORCH_CHECK(bits % 4 == 0, "cuembed_pyt: every table must be 4-byte aligned");
  TORCH_CHECK(descriptor.is_cuda() && descriptor.device() == tables[0].device() && descriptor.scalar_type() == at::kInt &&
                  descriptor.is_contiguous() && descriptor.numel() == (num_tables + 1) * 4,
              "cuembed_pyt: descriptor must be the contiguous int32 tensor of (num_tables + 1) * 4 words on the tables' "
              "device");
  CheckGroupedBatch(&c, num_tables, indices, offsets, weights, tables[0].scalar_type(), row_loads, c10::nullopt);
  const int idx = c.idx, off = c.off;
  const int64_t batch = c.batch, hot = c.hot;
  const at::Tensor &i = c.i, &o = c.o, &w = c.w;
  at::Tensor out = at::empty({batch, dim}, tables[0].options());
  int shape[7];
  ::cuembed_mixed_group_launch_shape(widths.data(), static_cast<int>(num_tables), elem, idx, static_cast<int>(batch),
                                     static_cast<int>(hot), w.defined() ? 1 : 0,
                                     static_cast<size_t>(bits | reinterpret_cast<uintptr_t>(out.data_ptr())), shape);
  TORCH_CHECK(lane_bytes == shape[0] * tables[0].element_size(), "cuembed_pyt: the descriptor was filled for lanes of ",
              lane_bytes, " bytes, these tables and this result take ", shape[0] * tables[0].element_size());
  if (batch > 0)
    ::cuembed_embedding_forward_mixed_group(c.host_ptrs.data(), static_cast<const void* const*>(table_ptrs.data_ptr()),
                                            widths.data(), descriptor.data_ptr(), static_cast<int>(num_tables), elem,
                                            Ptr(i), idx, Ptr(o), off, Ptr(w), static_cast<int>(batch),
                                            static_cast<int>(hot), m, MutPtr(out), static_cast<int>(row_loads),
                                            CurrentStream(out));
  return out;
}

// ---- the backward of a group: keys + sample ids in front of the single-table pipeline, table cuts behind it ----------
// idx / offsets as in cuemb_embedding_grouped; row_base = the int64 device tensor of num_tables + 1 exclusive prefix sums
// of the tables' row counts (cuembed_amd.TableGroup.row_base_device).  narrow: int32 results (the caller knows that the
// group has fewer than 2^31 rows), else int64.  Returns (keys, sample_ids), nnz entries each.
std::tuple<at::Tensor, at::Tensor> cuembed_grouped_backward_keys_op(const at::Tensor& indices,
                                                                    const c10::optional<at::Tensor>& offsets,
                                                                    const at::Tensor& row_base, const int64_t num_tables,
                                                                    const int64_t batch, const int64_t num_hots,
                                                                    const bool narrow) {
  CheckGpu(indices, "indices");
  CheckGpu(row_base, "row_base");
  const int idx = IndexCode(indices, "indices");
  TORCH_CHECK(num_tables >= 1 && batch >= 0 && num_tables * batch <= INT32_MAX,
              "cuembed_pyt: num_tables >= 1, batch >= 0 and num_tables * batch must fit a 32-bit int");
  TORCH_CHECK(row_base.scalar_type() == at::kLong && row_base.is_contiguous() && row_base.numel() == num_tables + 1 &&
                  row_base.device() == indices.device(),
              "cuembed_pyt: row_base must be the contiguous int64 tensor of num_tables + 1 row offsets on the indices' device");
  const at::DeviceGuard guard(indices.device());
  const at::Tensor i = indices.contiguous();
  const int64_t nnz = i.numel();
  TORCH_CHECK(nnz <= INT32_MAX, "cuembed_pyt: nnz must fit an int");
  at::Tensor o;
  int off = CUEMBED_I32;
  if (offsets.has_value() && offsets->defined()) {
    CheckGpu(*offsets, "offsets");
    off = IndexCode(*offsets, "offsets");
    o = offsets->contiguous();
    TORCH_CHECK(num_hots == 0 && o.numel() == num_tables * batch + 1,
                "cuembed_pyt: CSR: num_hots = 0 and offsets of num_tables * batch + 1 entries");
  } else {
    TORCH_CHECK(num_hots > 0 && nnz == num_tables * batch * num_hots,
                "cuembed_pyt: fixed hotness: num_hots > 0 and num_tables * batch * num_hots indices");
  }
  const at::TensorOptions options = i.options().dtype(narrow ? at::kInt : at::kLong);
  at::Tensor keys = at::empty({nnz}, options), sample_ids = at::empty({nnz}, options);
  if (nnz > 0)
    ::cuembed_grouped_backward_keys(Ptr(i), idx, Ptr(o), off, static_cast<const int64_t*>(row_base.data_ptr()),
                                    static_cast<int>(num_tables), static_cast<int>(batch), static_cast<int>(num_hots), nnz,
                                    MutPtr(keys), MutPtr(sample_ids), narrow ? CUEMBED_I32 : CUEMBED_I64, CurrentStream(i));
  return std::make_tuple(keys, sample_ids);
}

// ids: the ascending global ids of a group's compressed gradient; count_word: one device word, the entry count (int32 /
// int64) or, with last_id = true, the last id (ids' dtype; count = last id + 1).  Returns the int64 cuts[num_tables + 1].
at::Tensor cuembed_grouped_table_cuts_op(const at::Tensor& ids, const at::Tensor& count_word, const at::Tensor& row_base,
                                         const bool last_id) {
  CheckGpu(ids, "ids");
  CheckGpu(count_word, "count_word");
  CheckGpu(row_base, "row_base");
  const int idx = IndexCode(ids, "ids");
  const int word = IndexCode(count_word, "count_word");
  TORCH_CHECK(count_word.numel() == 1 && count_word.device() == ids.device(),
              "cuembed_pyt: count_word must be one word on the ids' device");
  TORCH_CHECK(!last_id || count_word.scalar_type() == ids.scalar_type(), "cuembed_pyt: a last id has the ids' dtype");
  TORCH_CHECK(row_base.scalar_type() == at::kLong && row_base.is_contiguous() && row_base.dim() == 1 &&
                  row_base.numel() >= 2 && row_base.device() == ids.device(),
              "cuembed_pyt: row_base must be the contiguous int64 tensor of num_tables + 1 row offsets on the ids' device");
  const at::DeviceGuard guard(ids.device());
  const at::Tensor i = ids.contiguous();
  at::Tensor cuts = at::empty({row_base.numel()}, row_base.options());
  ::cuembed_grouped_table_cuts(Ptr(i), idx, i.numel(), 0, last_id ? nullptr : Ptr(count_word), word == CUEMBED_I64 ? 1 : 0,
                               last_id ? Ptr(count_word) : nullptr, static_cast<const int64_t*>(row_base.data_ptr()),
                               static_cast<int>(row_base.numel() - 1), static_cast<int64_t*>(cuts.data_ptr()),
                               CurrentStream(i));
  return cuts;
}

// ---- a group beyond sum pooling with table gradients: the per-lookup weight gradient and the mean's scale ---------
// tables / table_ptrs / idx / offsets as in cuemb_embedding_grouped; y_grad [batch, num_tables, width] of the tables'
// dtype.  Returns the gradient of a weighted SUM-forward with respect to the weights, in the shape of idx.
at::Tensor cuembed_grouped_weight_grad_op(const at::TensorList tables, const at::Tensor& table_ptrs,
                                          const at::Tensor& indices, const c10::optional<at::Tensor>& offsets,
                                          const at::Tensor& y_grad) {
  TORCH_CHECK(!tables.empty(), "cuembed_pyt: a group needs at least one table");
  const int elem = ElemCode(tables[0], "tables");
  const at::DeviceGuard guard(tables[0].device());
  const GroupedCall c =
      CheckGroupedCall(tables, table_ptrs, indices, offsets, c10::nullopt, tables[0].scalar_type(), -1, c10::nullopt);
  const int64_t num_tables = static_cast<int64_t>(tables.size()), width = tables[0].size(1);
  CheckGpu(y_grad, "y_grad");
  TORCH_CHECK(y_grad.scalar_type() == tables[0].scalar_type() && y_grad.dim() == 3 && y_grad.size(0) == c.batch &&
                  y_grad.size(1) == num_tables && y_grad.size(2) == width && y_grad.device() == tables[0].device(),
              "cuembed_pyt: y_grad must be [batch, num_tables, width] of the tables' dtype on their device");
  const at::Tensor g = y_grad.contiguous();
  uintptr_t bits = 0;
  for (const void* p : c.host_ptrs) bits |= reinterpret_cast<uintptr_t>(p);
  CheckRowAlignment("tables / y_grad", width, tables[0].element_size(), {reinterpret_cast<const void*>(bits), Ptr(g)}, true);
  at::Tensor out = at::empty(c.i.sizes(), tables[0].options());
  if (c.batch > 0 && c.i.numel() > 0)
    ::cuembed_embedding_weight_grad_grouped(c.host_ptrs.data(), static_cast<const void* const*>(table_ptrs.data_ptr()),
                                            static_cast<int>(num_tables), elem, static_cast<int>(width), Ptr(c.i), c.idx,
                                            Ptr(c.o), c.off, Ptr(g), static_cast<int>(c.batch), static_cast<int>(c.hot),
                                            MutPtr(out), CurrentStream(out));
  return out;
}

// The batch of a mean scale: the batch size is y_grad's, so only the offsets (CSR, hotness = 0) or the hotness, and the
// weights (one per lookup, of the dtype and on the device of `like`, the contiguous y_grad) are left to check.
struct MeanScaleBatch {
  at::Tensor o, w;
  int off = CUEMBED_I32;
};

MeanScaleBatch CheckMeanScaleBatch(const c10::optional<at::Tensor>& offsets, const c10::optional<at::Tensor>& weights,
                                   const int64_t num_tables, const int64_t batch, const int64_t hotness,
                                   const at::Tensor& like) {
  MeanScaleBatch b;
  int64_t nnz = num_tables * batch * hotness;
  if (offsets.has_value() && offsets->defined()) {
    CheckGpu(*offsets, "offsets");
    b.off = IndexCode(*offsets, "offsets");
    b.o = offsets->contiguous();
    TORCH_CHECK(hotness == 0 && b.o.numel() == num_tables * batch + 1 && b.o.device() == like.device(),
                "cuembed_pyt: CSR: hotness = 0 and offsets of num_tables * batch + 1 entries on y_grad's device");
    nnz = -1;   // (known on the device only)
  } else {
    TORCH_CHECK(hotness > 0, "cuembed_pyt: fixed hotness: hotness > 0");
  }
  if (weights.has_value() && weights->defined()) {
    CheckGpu(*weights, "weights");
    TORCH_CHECK(weights->scalar_type() == like.scalar_type() && weights->device() == like.device() &&
                    (nnz < 0 || weights->numel() >= nnz),
                "cuembed_pyt: weights must have one entry per lookup, of y_grad's dtype, on its device");
    b.w = weights->contiguous();
  }
  return b;
}

// y_grad [batch, num_tables, width] of a MEAN-pooled group times each bag's mean factor: the y_grad of the equivalent
// sum-pooled group (a new tensor).  offsets given: CSR, num_tables * batch + 1 entries, hotness = 0; absent: every bag
// has `hotness` lookups.  weights: one per lookup, of y_grad's dtype (the mean is then over the weights).
at::Tensor cuembed_grouped_mean_scale_op(const at::Tensor& y_grad, const c10::optional<at::Tensor>& offsets,
                                         const c10::optional<at::Tensor>& weights, const int64_t num_tables,
                                         const int64_t hotness) {
  CheckGpu(y_grad, "y_grad");
  const int elem = ElemCode(y_grad, "y_grad");
  TORCH_CHECK(num_tables >= 1 && y_grad.dim() == 3 && y_grad.size(1) == num_tables,
              "cuembed_pyt: y_grad must be [batch, num_tables, width]");
  const int64_t batch = y_grad.size(0), width = y_grad.size(2);
  TORCH_CHECK(num_tables * batch <= INT32_MAX, "cuembed_pyt: num_tables * batch must fit a 32-bit int");
  const at::DeviceGuard guard(y_grad.device());
  const at::Tensor g = y_grad.contiguous();
  const MeanScaleBatch b = CheckMeanScaleBatch(offsets, weights, num_tables, batch, hotness, g);
  at::Tensor out = at::empty_like(g);
  CheckRowAlignment("y_grad", width, g.element_size(), {Ptr(g), Ptr(out)}, true);
  if (batch > 0 && width > 0)
    ::cuembed_grouped_mean_scale(Ptr(g), elem, static_cast<int>(width), Ptr(b.o), b.off, Ptr(b.w),
                                 static_cast<int>(num_tables),
                                 static_cast<int>(batch), static_cast<int>(hotness), MutPtr(out), CurrentStream(g));
  return out;
}

// ---- the backward of a group of tables of DIFFERENT widths: the scatter-add for all widths and the mean's scale ---------
// What both ops check of the group: widths (host ints) and table_columns, the int32 [num_tables, 2] device tensor of
// (c_t, W_t).  It MUST be cuembed_amd.MixedTableGroup.table_columns_device of the group the widths belong to (c_t the
// exclusive prefix sum of the widths): its place, dtype and size are checked here, its CONTENTS are on the device and are
// not -- the kernels address y_grad and pick their lanes from them.  Returns D.
static int64_t CheckMixedColumns(const at::IntArrayRef widths, const at::Tensor& table_columns, const at::Tensor& y_grad,
                                 std::vector<int>* widths_out, int64_t* max_width) {
  const int64_t num_tables = static_cast<int64_t>(widths.size());
  TORCH_CHECK(num_tables >= 1, "cuembed_pyt: a group needs at least one table");
  int64_t dim = 0;
  *max_width = 0;
  for (const int64_t w : widths) {
    TORCH_CHECK(w > 0 && (w * y_grad.element_size()) % 4 == 0, "cuembed_pyt: every row must be a multiple of 4 bytes");
    dim += w;
    TORCH_CHECK(dim <= INT32_MAX, "cuembed_pyt: the widths must sum to at most 2^31 - 1");
    if (w > *max_width) *max_width = w;
    widths_out->push_back(static_cast<int>(w));
  }
  TORCH_CHECK(table_columns.is_cuda() && table_columns.device() == y_grad.device() &&
                  table_columns.scalar_type() == at::kInt && table_columns.is_contiguous() &&
                  table_columns.numel() == 2 * num_tables,
              "cuembed_pyt: table_columns must be the contiguous int32 [num_tables, 2] tensor of (column base, width) on "
              "y_grad's device");
  TORCH_CHECK(y_grad.dim() == 2 && y_grad.size(1) == dim, "cuembed_pyt: y_grad must be [batch, sum of the widths]");
  return dim;
}

// y_grad [batch, D]; the sorted lookups of all tables as cuembed_transpose_* gives them for cuembed_grouped_backward_keys'
// keys and sample ids, with the remapped ids.  Returns (rows [capacity, W_max], ids [capacity], overflow int32 [1]):
// the compressed gradient padded to the widest table -- entry k in rows[k, :W_t], the columns past W_t unspecified --,
// its ascending global row ids, and a word that is 1 when the device-side count (remap[-1] + 1) exceeded `capacity` and
// nothing was written.  Entries at and past the count hold nothing.
std::tuple<at::Tensor, at::Tensor, at::Tensor> cuembed_embedding_backward_mixed_group_op(
    const at::Tensor& y_grad, const at::IntArrayRef widths, const at::Tensor& table_columns,
    const at::Tensor& transpose_indices, const at::Tensor& transpose_sample_ids,
    const at::Tensor& transpose_remapped_indices, const c10::optional<at::Tensor>& transpose_weights,
    const int64_t capacity) {
  CheckGpu(y_grad, "y_grad");
  const int elem = ElemCode(y_grad, "y_grad");
  const at::DeviceGuard guard(y_grad.device());
  std::vector<int> w_host;
  int64_t max_width = 0;
  const int64_t dim = CheckMixedColumns(widths, table_columns, y_grad, &w_host, &max_width);
  const int64_t num_tables = static_cast<int64_t>(widths.size()), batch = y_grad.size(0);
  TORCH_CHECK(num_tables * batch <= INT32_MAX, "cuembed_pyt: num_tables * batch must fit a 32-bit int");
  TORCH_CHECK(capacity >= 0, "cuembed_pyt: capacity must not be negative");
  CheckGpu(transpose_indices, "transpose_indices");
  const int idx = IndexCode(transpose_indices, "transpose_indices");
  const int64_t nnz = transpose_indices.numel();
  TORCH_CHECK(nnz <= INT32_MAX, "cuembed_pyt: nnz must fit an int");
  for (const at::Tensor* t : {&transpose_sample_ids, &transpose_remapped_indices})
    TORCH_CHECK(t->is_cuda() && t->device() == y_grad.device() && t->scalar_type() == transpose_indices.scalar_type() &&
                    t->numel() == nnz,
                "cuembed_pyt: the sample ids and the remapped ids must match transpose_indices");
  const at::Tensor g = y_grad.contiguous(), ti = transpose_indices.contiguous(), ts = transpose_sample_ids.contiguous(),
                   tr = transpose_remapped_indices.contiguous();
  at::Tensor tw;
  if (transpose_weights.has_value() && transpose_weights->defined() && transpose_weights->numel() > 0) {
    CheckGpu(*transpose_weights, "transpose_weights");
    TORCH_CHECK(transpose_weights->scalar_type() == g.scalar_type() && transpose_weights->numel() >= nnz,
                "cuembed_pyt: transpose_weights must have one entry per lookup, of y_grad's dtype");
    tw = transpose_weights->contiguous();
  }
  at::Tensor rows = at::empty({capacity, max_width}, g.options());
  at::Tensor ids = at::empty({capacity}, ti.options());
  at::Tensor overflow = at::zeros({1}, g.options().dtype(at::kInt));
  if (nnz == 0) return std::make_tuple(rows, ids, overflow);
  if (capacity == 0) {
    overflow.fill_(1);
    return std::make_tuple(rows, ids, overflow);
  }
  // the launch's lane is the library's to decide: the C ABI is asked with both bases OR-ed.  (The forward's shape function
  // at batch 0 is the lane rule and nothing else; the backward's would abort, not raise, on the limit checked next.)
  const uintptr_t bits = reinterpret_cast<uintptr_t>(g.data_ptr()) | reinterpret_cast<uintptr_t>(rows.data_ptr());
  TORCH_CHECK(bits % 4 == 0, "cuembed_pyt: y_grad must be 4-byte aligned");
  int shape[7];
  ::cuembed_mixed_group_launch_shape(w_host.data(), static_cast<int>(num_tables), elem, CUEMBED_I32, 0, 0, 0,
                                     static_cast<size_t>(bits), shape);
  const int64_t lane_elems = shape[0];
  TORCH_CHECK(max_width / lane_elems <= 1024, "cuembed_pyt: the widest table is more than 1024 lanes");
  TORCH_CHECK(batch * (dim / lane_elems) < (int64_t{1} << 31),
              "cuembed_pyt: batch * sum of the widths / elements per lane must stay below 2^31");
  ::cuembed_embedding_backward_mixed_group(Ptr(g), elem, w_host.data(), table_columns.data_ptr(),
                                           static_cast<int>(num_tables), static_cast<int>(batch), nnz, Ptr(ti), Ptr(ts),
                                           Ptr(tr), idx, Ptr(tw), MutPtr(rows), MutPtr(ids), capacity,
                                           static_cast<uint32_t*>(overflow.data_ptr()), CurrentStream(g));
  return std::make_tuple(rows, ids, overflow);
}

// y_grad [batch, D] of a MEAN-pooled mixed-width group times each bag's mean factor (a new tensor); offsets / weights /
// hotness as in cuembed_grouped_mean_scale.
at::Tensor cuembed_mixed_group_mean_scale_op(const at::Tensor& y_grad, const at::IntArrayRef widths,
                                             const at::Tensor& table_columns, const c10::optional<at::Tensor>& offsets,
                                             const c10::optional<at::Tensor>& weights, const int64_t hotness) {
  CheckGpu(y_grad, "y_grad");
  const int elem = ElemCode(y_grad, "y_grad");
  const at::DeviceGuard guard(y_grad.device());
  std::vector<int> w_host;
  int64_t max_width = 0;
  CheckMixedColumns(widths, table_columns, y_grad, &w_host, &max_width);
  const int64_t num_tables = static_cast<int64_t>(widths.size()), batch = y_grad.size(0);
  TORCH_CHECK(num_tables * batch <= INT32_MAX, "cuembed_pyt: num_tables * batch must fit a 32-bit int");
  const at::Tensor g = y_grad.contiguous();
  const MeanScaleBatch b = CheckMeanScaleBatch(offsets, weights, num_tables, batch, hotness, g);
  at::Tensor out = at::empty_like(g);
  if (batch > 0)
    ::cuembed_mixed_group_mean_scale(Ptr(g), elem, w_host.data(), table_columns.data_ptr(), Ptr(b.o), b.off, Ptr(b.w),
                                     static_cast<int>(num_tables), static_cast<int>(batch), static_cast<int>(hotness),
                                     MutPtr(out), CurrentStream(g));
  return out;
}

// Extension (cuembed::CheckIndices): is this batch safe to hand to the row-addressing ops?  No table is read and nothing
// is read back.  row_base: the int64 device tensor of num_tables + 1 entries of a group, or undefined and ONE table of
// num_rows rows.  CSR: offsets of num_tables * batch + 1 entries, num_hots = 0; fixed hotness: no offsets, num_hots > 0.
// Returns (report int64[4], repaired indices, repaired offsets); without `repair` -- and for the offsets of a
// fixed-hotness batch -- the latter are tensors of 0 entries.
std::tuple<at::Tensor, at::Tensor, at::Tensor> cuembed_check_indices_op(
    const at::Tensor& indices, const c10::optional<at::Tensor>& offsets, const c10::optional<at::Tensor>& row_base,
    const int64_t num_rows, const int64_t num_tables, const int64_t batch, const int64_t num_hots, const bool repair) {
  CheckGpu(indices, "indices");
  const int idx = IndexCode(indices, "indices");
  const bool grouped = row_base.has_value() && row_base->defined();
  TORCH_CHECK(num_tables >= 1 && num_tables <= 1023, "cuembed_pyt: 1 <= num_tables <= 1023");
  if (grouped) {
    CheckGpu(*row_base, "row_base");
    TORCH_CHECK(row_base->scalar_type() == at::kLong && row_base->numel() == num_tables + 1 && row_base->is_contiguous() &&
                    row_base->device() == indices.device(),
                "cuembed_pyt: row_base must be the contiguous int64 tensor of num_tables + 1 entries on indices' device");
  } else {
    TORCH_CHECK(num_tables == 1 && num_rows >= 1, "cuembed_pyt: without row_base: one table of num_rows >= 1 rows");
  }
  TORCH_CHECK(batch >= 0 && num_tables * batch <= INT32_MAX, "cuembed_pyt: num_tables * batch must fit a 32-bit int");
  const at::DeviceGuard guard(indices.device());
  const at::Tensor i = indices.contiguous();
  const int64_t nnz = i.numel();
  TORCH_CHECK(nnz <= (int64_t{1} << 38), "cuembed_pyt: at most 2^38 lookups per call");
  at::Tensor o;
  int off = CUEMBED_I32;
  if (offsets.has_value() && offsets->defined()) {
    CheckGpu(*offsets, "offsets");
    off = IndexCode(*offsets, "offsets");
    o = offsets->contiguous();
    TORCH_CHECK(num_hots == 0 && o.numel() == num_tables * batch + 1 && o.device() == i.device(),
                "cuembed_pyt: CSR: num_hots = 0 and offsets of num_tables * batch + 1 entries on indices' device");
    TORCH_CHECK(off == CUEMBED_I64 || nnz <= INT32_MAX, "cuembed_pyt: int32 offsets cannot address that many lookups");
  } else {
    TORCH_CHECK(num_hots > 0 && nnz == num_tables * batch * num_hots,
                "cuembed_pyt: fixed hotness: num_hots > 0 and indices of num_tables * batch * num_hots entries");
  }
  at::Tensor report = at::empty({4}, i.options().dtype(at::kLong));
  at::Tensor i_out = repair ? at::empty_like(i) : at::empty({0}, i.options());
  at::Tensor o_out = repair && o.defined() ? at::empty_like(o) : at::empty({0}, o.defined() ? o.options() : i.options());
  size_t lwork = 0;
  const int64_t* base = grouped ? static_cast<const int64_t*>(row_base->data_ptr()) : nullptr;
  ::cuembed_check_indices(nullptr, idx, nullptr, off, nnz, base, num_rows, static_cast<int>(num_tables),
                          static_cast<int>(batch), static_cast<int>(num_hots), nullptr, nullptr, nullptr, nullptr, &lwork,
                          nullptr);
  at::Tensor work = at::empty({static_cast<int64_t>(lwork > 0 ? lwork : 8)}, i.options().dtype(at::kByte));
  ::cuembed_check_indices(Ptr(i), idx, Ptr(o), off, nnz, base, num_rows, static_cast<int>(num_tables),
                          static_cast<int>(batch), static_cast<int>(num_hots), static_cast<int64_t*>(report.data_ptr()),
                          repair ? i_out.data_ptr() : nullptr, repair && o.defined() ? o_out.data_ptr() : nullptr,
                          static_cast<char*>(work.data_ptr()), &lwork, CurrentStream(i));
  return {report, i_out, o_out};
}

}  // namespace

TORCH_LIBRARY(cuembed_pyt, m) {
  // the reference's schemas, verbatim (examples/pytorch/cuembed_embedding.cu:169-183)
  m.def("cuembed_extract_row_ids_from_csr(Tensor offsets, int nnz) ->Tensor");
  m.def("cuembed_transpose(Tensor rows, Tensor cols, Tensor weights) -> (Tensor, Tensor, Tensor)");
  m.def("cuembed_embedding_forward(Tensor params, Tensor indices, Tensor offsets, Tensor weights, str mode) -> Tensor");
  m.def(
      "cuembed_embedding_backward(Tensor y_grad, int num_categories, Tensor transpose_indices, Tensor "
      "transpose_sample_ids, Tensor transpose_weights) -> Tensor");
  // this library's extensions
  m.def("cuembed_extract_row_ids_from_offsets(Tensor offsets, int nnz) -> Tensor");
  m.def("cuembed_transpose_bounded(Tensor rows, Tensor cols, Tensor weights, int num_categories) -> (Tensor, Tensor, Tensor)");
  m.def(
      "cuembed_transpose_sample_ids(Tensor sample_ids, Tensor indices, Tensor weights, int num_categories) -> "
      "(Tensor, Tensor, Tensor)");
  m.def(
      "cuembed_transpose_fixed_hotness(Tensor indices, Tensor weights, int num_categories, bool compressed) -> "
      "(Tensor, Tensor, Tensor, Tensor)");
  m.def(
      "cuembed_transpose_sample_blocks(Tensor sample_ids, Tensor indices, Tensor weights, int num_categories, int "
      "sample_blocks) -> (Tensor, Tensor, Tensor)");
  m.def("cuembed_compute_compressed_grad_indices(Tensor transpose_indices) -> Tensor");
  m.def(
      "cuembed_embedding_backward_compressed(Tensor y_grad, int num_unique, Tensor transpose_indices, Tensor "
      "transpose_sample_ids, Tensor transpose_remapped_indices, Tensor transpose_weights) -> (Tensor, Tensor)");
  m.def("cuembed_embedding_forward_fixed(Tensor params, Tensor indices, Tensor weights, str mode) -> Tensor");
  m.def("cuembed_embedding_weight_grad(Tensor params, Tensor indices, Tensor offsets, Tensor y_grad) -> Tensor");
  // forward + backward of cuemb_embedding as one native autograd node (see CuEmbEmbeddingNode)
  m.def(
      "cuemb_embedding_step(Tensor params, Tensor indices, Tensor offsets, Tensor? weights, int grad_kind, int row_loads, "
      "Tensor? sample_order, Tensor? row_loads_device) -> Tensor");
  m.def(
      "cuembed_embedding_forward_hinted(Tensor params, Tensor indices, Tensor offsets, Tensor? weights, str mode, int "
      "row_loads, Tensor? sample_order, Tensor? row_loads_device) -> Tensor");
  m.def("cuembed_decide_row_loads(Tensor indices, int table_bytes, Tensor(a!) decision) -> ()");
  m.def("cuembed_bag_order_by_length(Tensor offsets, int max_length) -> Tensor");
  m.def(
      "cuembed_exchange_pack(Tensor ids, Tensor rows, Tensor? count, Tensor cuts, int slot_capacity, int input_capacity, "
      "int num_categories, Tensor(a!) send_ids, Tensor(b!) send_rows, Tensor(c!) range_starts, Tensor(d!) flag) -> ()");
  m.def(
      "cuembed_exchange_merge(Tensor ids, Tensor rows, int num_categories, int pad_lo, int pad_len, Tensor(a!) out_ids, "
      "Tensor(b!) out_rows, Tensor(c!)? tail, Tensor(d!) flag, Tensor(e!)? count) -> ()");
  m.def(
      "cuembed_sparse_row_update_(Tensor(a!) table, Tensor(b!)? state, Tensor ids, Tensor rows, str rule, float lr, "
      "float eps, Tensor? lr_device, int count, Tensor? counts, Tensor? last_id, int piece_rows, bool "
      "stochastic_rounding=False, int seed=0, int step=0, Tensor? step_device=None) -> ()");
  m.def(
      "cuembed_sparse_row_adam_(Tensor(a!) table, Tensor(b!) exp_avg, Tensor(c!) exp_avg_sq, Tensor ids, Tensor rows, bool "
      "rowwise, float lr, float bias_factor, float beta1, float beta2, float eps, float weight_decay, Tensor? lr_device, "
      "Tensor? bias_factor_device, int count, Tensor? counts, Tensor? last_id, int piece_rows, bool "
      "stochastic_rounding=False, int seed=0, int step=0, Tensor? step_device=None) -> ()");
  // the same steps on a group of separate table tensors, in one launch each
  m.def(
      "cuembed_sparse_row_update_grouped(Tensor(a!)[] tables, Tensor table_ptrs, Tensor(b!)[] states, Tensor? state_ptrs, "
      "Tensor row_base, Tensor ids, Tensor rows, str rule, float lr, float eps, Tensor? lr_device, int count, Tensor? "
      "count_word, Tensor? last_id, bool stochastic_rounding=False, Tensor? seeds=None, int step=0, Tensor? "
      "step_device=None) -> ()");
  m.def(
      "cuembed_sparse_row_adam_grouped(Tensor(a!)[] tables, Tensor table_ptrs, Tensor(b!)[] exp_avg, Tensor exp_avg_ptrs, "
      "Tensor(c!)[] exp_avg_sq, Tensor exp_avg_sq_ptrs, Tensor row_base, Tensor ids, Tensor rows, bool rowwise, float lr, "
      "float bias_factor, float beta1, float beta2, float eps, float weight_decay, Tensor? lr_device, Tensor? "
      "bias_factor_device, int count, Tensor? count_word, Tensor? last_id, bool stochastic_rounding=False, Tensor? "
      "seeds=None, int step=0, Tensor? step_device=None) -> ()");
  // 8-bit row-wise quantized tables (torch's fused layout), inference only
  m.def("quantize_rows(Tensor table) -> Tensor");
  m.def("dequantize_rows(Tensor qtable, Tensor? ids, ScalarType dtype) -> Tensor");
  m.def(
      "cuemb_embedding_quantized(Tensor qtable, Tensor indices, Tensor? offsets, Tensor? weights, str mode, ScalarType "
      "out_dtype, int row_loads, Tensor? sample_order, Tensor? row_loads_device) -> Tensor");
  // a group of tables of one width and dtype pooled in one launch -> [batch, num_tables, width]; forward only
  m.def(
      "cuemb_embedding_grouped(Tensor[] tables, Tensor table_ptrs, Tensor idx, Tensor? offsets, Tensor? weights, str mode, "
      "int row_loads=-1, Tensor? sample_order=None) -> Tensor");
  m.def(
      "cuemb_embedding_quantized_grouped(Tensor[] qtables, Tensor table_ptrs, Tensor idx, Tensor? offsets, Tensor? weights, "
      "str mode, ScalarType out_dtype, int row_loads=-1, Tensor? sample_order=None) -> Tensor");
  // a group of plain tables of different widths pooled in one launch -> [batch, sum of widths]; forward only
  m.def(
      "cuemb_embedding_mixed_group(Tensor[] tables, Tensor table_ptrs, Tensor descriptor, int lane_bytes, Tensor idx, "
      "Tensor? offsets, Tensor? weights, str mode, int row_loads=-1) -> Tensor");
  // the backward of a group: the keys in front of the single-table pipeline, the table boundaries behind it
  m.def(
      "cuembed_grouped_backward_keys(Tensor idx, Tensor? offsets, Tensor row_base, int num_tables, int batch, int "
      "num_hots, bool narrow) -> (Tensor, Tensor)");
  m.def("cuembed_grouped_table_cuts(Tensor ids, Tensor count_word, Tensor row_base, bool last_id=False) -> Tensor");
  // a group beyond sum pooling with table gradients: the per-lookup weight gradient, the scale of a mean's y_grad
  m.def("cuembed_grouped_weight_grad(Tensor[] tables, Tensor table_ptrs, Tensor idx, Tensor? offsets, Tensor y_grad) -> Tensor");
  m.def("cuembed_grouped_mean_scale(Tensor y_grad, Tensor? offsets, Tensor? weights, int num_tables, int hotness) -> Tensor");
  // the backward of a mixed-width group: the scatter-add for all widths -> (padded rows, ids, overflow word); the mean's scale
  m.def(
      "cuembed_embedding_backward_mixed_group(Tensor y_grad, int[] widths, Tensor table_columns, Tensor transpose_indices, "
      "Tensor transpose_sample_ids, Tensor transpose_remapped_indices, Tensor? transpose_weights, int capacity) -> "
      "(Tensor, Tensor, Tensor)");
  m.def(
      "cuembed_mixed_group_mean_scale(Tensor y_grad, int[] widths, Tensor table_columns, Tensor? offsets, Tensor? weights, "
      "int hotness) -> Tensor");
  // the device-side index check in front of the row-addressing ops: (report, repaired indices, repaired offsets)
  m.def(
      "cuembed_check_indices(Tensor indices, Tensor? offsets, Tensor? row_base, int num_rows, int num_tables, int batch, "
      "int num_hots, bool repair=False) -> (Tensor, Tensor, Tensor)");
}

TORCH_LIBRARY_IMPL(cuembed_pyt, Autograd, m) {
  m.impl("cuemb_embedding_step", [](const at::Tensor& params, const at::Tensor& indices, const at::Tensor& offsets,
                                    const c10::optional<at::Tensor>& weights, int64_t grad_kind, int64_t row_loads,
                                    const c10::optional<at::Tensor>& sample_order,
                                    const c10::optional<at::Tensor>& row_loads_device) {
    return cuemb_embedding_autograd_op(params, indices, offsets, weights.has_value() ? *weights : at::Tensor(), grad_kind,
                                       row_loads, sample_order.has_value() ? *sample_order : at::Tensor(),
                                       row_loads_device.has_value() ? *row_loads_device : at::Tensor());
  });
}

TORCH_LIBRARY_IMPL(cuembed_pyt, CUDA, m) {  // HIP tensors use the CUDA dispatch key on PyTorch-ROCm
  m.impl("cuembed_extract_row_ids_from_csr", cuembed_extract_row_ids_from_csr_op);
  m.impl("cuembed_transpose", cuembed_transpose_op);
  m.impl("cuembed_embedding_forward", cuembed_embedding_forward_op);
  m.impl("cuembed_embedding_backward", cuembed_embedding_backward_op);
  m.impl("cuembed_extract_row_ids_from_offsets", cuembed_extract_row_ids_from_offsets_op);
  m.impl("cuembed_transpose_bounded", cuembed_transpose_bounded_op);
  m.impl("cuembed_transpose_sample_ids", cuembed_transpose_sample_ids_op);
  m.impl("cuembed_transpose_sample_blocks", cuembed_transpose_sample_blocks_op);
  m.impl("cuembed_transpose_fixed_hotness", cuembed_transpose_fixed_hotness_op);
  m.impl("cuembed_compute_compressed_grad_indices", cuembed_compute_compressed_grad_indices_op);
  m.impl("cuembed_embedding_backward_compressed", cuembed_embedding_backward_compressed_op);
  m.impl("cuembed_embedding_forward_fixed", cuembed_embedding_forward_fixed_op);
  m.impl("cuembed_embedding_weight_grad", cuembed_embedding_weight_grad_op);
  m.impl("cuembed_embedding_forward_hinted", cuembed_embedding_forward_hinted_op);
  m.impl("cuembed_bag_order_by_length", cuembed_bag_order_by_length_op);
  m.impl("cuembed_decide_row_loads", cuembed_decide_row_loads_op);
  m.impl("cuembed_exchange_pack", cuembed_exchange_pack_op);
  m.impl("cuembed_exchange_merge", cuembed_exchange_merge_op);
  m.impl("cuembed_sparse_row_update_", cuembed_sparse_row_update_op);
  m.impl("cuembed_sparse_row_adam_", cuembed_sparse_row_adam_op);
  m.impl("cuembed_sparse_row_update_grouped", cuembed_sparse_row_update_grouped_op);
  m.impl("cuembed_sparse_row_adam_grouped", cuembed_sparse_row_adam_grouped_op);
  m.impl("quantize_rows", quantize_rows_op);
  m.impl("dequantize_rows", dequantize_rows_op);
  m.impl("cuemb_embedding_quantized", cuemb_embedding_quantized_op);
  m.impl("cuemb_embedding_grouped", cuemb_embedding_grouped_op);
  m.impl("cuemb_embedding_quantized_grouped", cuemb_embedding_quantized_grouped_op);
  m.impl("cuemb_embedding_mixed_group", cuemb_embedding_mixed_group_op);
  m.impl("cuembed_grouped_backward_keys", cuembed_grouped_backward_keys_op);
  m.impl("cuembed_grouped_table_cuts", cuembed_grouped_table_cuts_op);
  m.impl("cuembed_grouped_weight_grad", cuembed_grouped_weight_grad_op);
  m.impl("cuembed_grouped_mean_scale", cuembed_grouped_mean_scale_op);
  m.impl("cuembed_embedding_backward_mixed_group", cuembed_embedding_backward_mixed_group_op);
  m.impl("cuembed_mixed_group_mean_scale", cuembed_mixed_group_mean_scale_op);
  m.impl("cuembed_check_indices", cuembed_check_indices_op);
}
