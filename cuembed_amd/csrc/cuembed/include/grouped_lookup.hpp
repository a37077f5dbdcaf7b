// MI355X (gfx950 / CDNA4) forward on a GROUP of embedding tables in one launch -- header-only host API (an extension:
// the reference's entry points take one table).
//
//   EmbeddingForwardGrouped            EmbeddingForward (sum / mean) on T tables of one width and element type
//   EmbeddingForwardQuantizedGrouped   EmbeddingForwardQuantized (sum / mean) on T fused 8-bit tables of one width
//
// Layout (grouped_gather_kernels.hpp): bag g = t * B + b belongs to table t and sample b; CSR has one indices[nnz], one
// offsets[T * B + 1] and optional weights[nnz]; fixed hotness has indices[T, B, H]; the result is out[B, T, W],
// contiguous -- torch.stack of T single-table results on dim 1, with the same bits.
//
// The caller builds TWO copies of the table base pointers once: one in host memory, which the library reads to choose the
// access width (one misaligned table narrows the whole group), and one in device memory, which the kernel reads.  The
// library never reads device memory on the host, copies nothing per call and allocates nothing; the call is asynchronous
// on `stream` (last argument) and CUEMBED_ASSERTs (print and abort) on misuse, like every other entry point.
//
// Forward only, sum and mean only, fp32 accumulation in lookup order.  Of ForwardOptions, row_loads (one host value for
// the group) and sample_order (a permutation of the T * B bags: BagOrderByLength on the combined offsets) are honoured
// as scheduling hints that change no bit; row_loads_device must be null (the decision is per table and nothing carries
// T decisions); reduction_order is not consulted (there is one order: the wide-load and split kernels are not taken).
// A group of mixed WIDTHS is EmbeddingForwardMixedGroup (mixed_group_lookup.hpp: plain tables, no sample_order); groups of
// mixed element types are the caller's job: one group per type.
#ifndef CUEMBED_INCLUDE_GROUPED_LOOKUP_HPP_
#define CUEMBED_INCLUDE_GROUPED_LOOKUP_HPP_

#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>
#include <type_traits>

#include "cuembed/include/cuembed_assert.hpp"
#include "cuembed/include/device_shape.hpp"
#include "cuembed/include/embedding_lookup.hpp"
#include "cuembed/include/grouped_gather_kernels.hpp"
#include "cuembed/include/quantized_lookup.hpp"

namespace cuembed {

namespace detail {

//! All table bases of a group OR-ed into one address: what SplitRow and QuantizedForwardCodesPerLane look at (the low
//! bits), so that the least aligned table decides for the group.
inline const void* GroupAlignmentBits(const void* const* tables_host, const int num_tables) {
  uintptr_t bits = 0;
  for (int t = 0; t < num_tables; ++t) {
    CUEMBED_ASSERT(tables_host[t] != nullptr);
    bits |= reinterpret_cast<uintptr_t>(tables_host[t]);
  }
  return reinterpret_cast<const void*>(bits);
}

//! T * B, asserted to fit an int.
inline int GroupedBatch(const int num_tables, const int batch_per_table) {
  CUEMBED_ASSERT(num_tables >= 1 && batch_per_table >= 0);
  const int64_t batch = static_cast<int64_t>(num_tables) * batch_per_table;
  CUEMBED_ASSERT(batch <= INT_MAX);
  return static_cast<int>(batch);
}

//! The argument contract both grouped entry points share.
template <typename OffsetT>
inline void CheckGroupedCall(const void* tables_host, const void* tables_device, const OffsetT* offsets,
                             const int num_hots, const CombineMode mode, const ForwardOptions& options) {
  CUEMBED_ASSERT(tables_host != nullptr && tables_device != nullptr);
  CUEMBED_ASSERT(mode == CombineMode::kSum || mode == CombineMode::kMean);
  CUEMBED_ASSERT((offsets != nullptr && num_hots == 0) || (offsets == nullptr && num_hots > 0));
  CUEMBED_ASSERT(options.sample_order == nullptr || offsets != nullptr);
  CUEMBED_ASSERT(options.row_loads_device == nullptr);
}

template <typename ElemT, typename IndexT, typename OffsetT, int N>
inline void LaunchGatherReduceGrouped(const ElemT* const* tables, const int batch_per_table, const int num_tables,
                                      const int width, const IndexT* indices, const OffsetT* offsets,
                                      const ElemT* weights, const int batch, const int num_hots, const bool is_mean,
                                      ElemT* out, const ForwardLaunch& f, hipStream_t stream,
                                      const ForwardOptions& options) {
  const bool stream_rows = options.row_loads == RowLoadPolicy::kStreaming;
  const dim3 block(f.split.lanes_per_row, f.split.rows_per_block, 1);
  const dim3 grid(f.grid, 1, 1);
  WithIndexSource(f.staged, f.split.lanes_per_row, weights != nullptr, [&](auto w, auto source) {
    GatherReduceGroupedKernel<ElemT, IndexT, OffsetT, N, decltype(w)::value, decltype(source)::value>
        <<<grid, block, f.stage_bytes, stream>>>(tables, batch_per_table, num_tables, width, batch, indices, offsets,
                                                 num_hots, weights, is_mean, out, stream_rows,
                                                 offsets != nullptr ? options.sample_order : nullptr);
  });
}

template <typename OutT, typename IndexT, typename OffsetT, int N>
inline void LaunchGatherReduceQuantizedGrouped(const uint8_t* const* tables, const int batch_per_table,
                                               const int num_tables, const int width, const IndexT* indices,
                                               const OffsetT* offsets, const OutT* weights, const int batch,
                                               const int num_hots, const bool is_mean, OutT* out,
                                               const QuantizedForwardLaunch& f, hipStream_t stream,
                                               const ForwardOptions& options) {
  const bool stream_rows = options.row_loads == RowLoadPolicy::kStreaming;
  const dim3 block(f.lanes_per_row, f.rows_per_block, 1);
  const dim3 grid(f.grid, 1, 1);
  WithIndexSource(f.staged, f.lanes_per_row, weights != nullptr, [&](auto w, auto source) {
    GatherReduceQuantizedGroupedKernel<OutT, IndexT, OffsetT, N, decltype(w)::value, decltype(source)::value>
        <<<grid, block, f.stage_bytes, stream>>>(tables, batch_per_table, num_tables, width, batch, indices, offsets,
                                                 num_hots, weights, is_mean, out, stream_rows,
                                                 offsets != nullptr ? options.sample_order : nullptr);
  });
}

}  // namespace detail

/**
 * @brief EmbeddingForward (sum / mean) on a group of `num_tables` tables of one element type and width, in one launch:
 * ret[b, t, :] = combine_j weights[.] * tables[t][indices[.], :] over the lookups of bag t * batch_per_table + b.
 * Bit-identical to num_tables calls of EmbeddingForward (fp32 accumulation) stacked on dimension 1.
 *
 * @tparam InputT   table element type (float, __half or __hip_bfloat16)
 * @tparam OutputT  result element type (must equal InputT)
 *
 * @param tables_host      [num_tables] table base pointers, in HOST memory (read here, for the access width)
 * @param tables_device    the same pointers in DEVICE memory (read by the kernel)
 * @param num_tables       T >= 1
 * @param embed_width      elements per row of every table (row bytes a multiple of 4)
 * @param indices          CSR: [nnz]; fixed hotness: [T, B, num_hots]; ids of table t are rows of tables[t]
 * @param offsets          CSR: [T * B + 1], or nullptr
 * @param weights          per-lookup weights in the tables' type (same layout as indices) or nullptr
 * @param batch_per_table  B; T * B <= INT_MAX
 * @param num_hots         fixed hotness (the same for every table), 0 for CSR
 * @param mode             kSum or kMean
 * @param ret              [B, T, embed_width], contiguous
 */
template <typename InputT, typename OutputT, typename IndexT, typename OffsetT>
void EmbeddingForwardGrouped(const InputT* const* tables_host,
                             const InputT* const* tables_device,
                             const int num_tables,
                             const int embed_width,
                             const IndexT* indices,
                             const OffsetT* offsets,
                             const GetElemT<InputT>* weights,
                             const int batch_per_table,
                             const int num_hots,
                             const CombineMode mode,
                             OutputT* ret,
                             const hipStream_t stream,
                             const ForwardOptions& options) {
  static_assert(std::is_same<InputT, OutputT>::value, "EmbeddingForwardGrouped: OutputT must equal InputT");
  using HostElemT = GetElemT<InputT>;
  static_assert(std::is_same<HostElemT, float>::value || std::is_same<HostElemT, __half>::value ||
                    std::is_same<HostElemT, __hip_bfloat16>::value,
                "EmbeddingForwardGrouped: table elements must be float, __half or __hip_bfloat16");
  using ElemT = detail::DeviceElemT<HostElemT>;
  detail::CheckGroupedCall(tables_host, tables_device, offsets, num_hots, mode, options);
  const int batch = detail::GroupedBatch(num_tables, batch_per_table);
  if (batch <= 0) return;
  const void* bits = detail::GroupAlignmentBits(reinterpret_cast<const void* const*>(tables_host), num_tables);
  const detail::ForwardLaunch f = detail::PlanForward<ElemT, IndexT>(embed_width, bits, ret, batch, num_hots,
                                                                     offsets != nullptr, weights != nullptr, false);
  const ElemT* const* tables = reinterpret_cast<const ElemT* const*>(tables_device);
  const ElemT* w = reinterpret_cast<const ElemT*>(weights);
  ElemT* out = reinterpret_cast<ElemT*>(ret);
  const bool is_mean = mode == CombineMode::kMean;
  constexpr int kMaxN = 16 / static_cast<int>(sizeof(ElemT));
  if (f.split.elems_per_lane == kMaxN)
    detail::LaunchGatherReduceGrouped<ElemT, IndexT, OffsetT, kMaxN>(
        tables, batch_per_table, num_tables, embed_width, indices, offsets, w, batch, num_hots, is_mean, out, f, stream,
        options);
  else if (f.split.elems_per_lane == kMaxN / 2)
    detail::LaunchGatherReduceGrouped<ElemT, IndexT, OffsetT, kMaxN / 2>(
        tables, batch_per_table, num_tables, embed_width, indices, offsets, w, batch, num_hots, is_mean, out, f, stream,
        options);
  else
    detail::LaunchGatherReduceGrouped<ElemT, IndexT, OffsetT, kMaxN / 4>(
        tables, batch_per_table, num_tables, embed_width, indices, offsets, w, batch, num_hots, is_mean, out, f, stream,
        options);
}

//! ... with the process-wide default options (DefaultForwardOptions()).
template <typename InputT, typename OutputT, typename IndexT, typename OffsetT>
void EmbeddingForwardGrouped(const InputT* const* tables_host,
                             const InputT* const* tables_device,
                             const int num_tables,
                             const int embed_width,
                             const IndexT* indices,
                             const OffsetT* offsets,
                             const GetElemT<InputT>* weights,
                             const int batch_per_table,
                             const int num_hots,
                             const CombineMode mode,
                             OutputT* ret,
                             const hipStream_t stream = 0) {
  EmbeddingForwardGrouped<InputT, OutputT, IndexT, OffsetT>(tables_host, tables_device, num_tables, embed_width, indices,
                                                            offsets, weights, batch_per_table, num_hots, mode, ret,
                                                            stream, DefaultForwardOptions());
}

/**
 * @brief EmbeddingForwardQuantized (sum / mean) on a group of `num_tables` fused 8-bit tables of one width, in one
 * launch.  Same layout as EmbeddingForwardGrouped; `weights` are in the output's type; bit-identical to num_tables
 * calls of EmbeddingForwardQuantized stacked on dimension 1.
 *
 * @tparam OutputT float or __half
 * @param tables_host / tables_device  [num_tables] bases of fused tables [rows_t x (embed_width + 8)] bytes, 4-byte aligned
 * @param ret                          [B, T, embed_width], 16-byte aligned
 */
template <typename OutputT, typename IndexT, typename OffsetT>
void EmbeddingForwardQuantizedGrouped(const uint8_t* const* tables_host,
                                      const uint8_t* const* tables_device,
                                      const int num_tables,
                                      const int embed_width,
                                      const IndexT* indices,
                                      const OffsetT* offsets,
                                      const OutputT* weights,
                                      const int batch_per_table,
                                      const int num_hots,
                                      const CombineMode mode,
                                      OutputT* ret,
                                      const hipStream_t stream,
                                      const ForwardOptions& options) {
  using OutT = detail::DeviceElemT<OutputT>;
  static_assert(std::is_same<OutputT, float>::value || std::is_same<OutputT, __half>::value,
                "EmbeddingForwardQuantizedGrouped: output must be float or __half");
  detail::CheckGroupedCall(tables_host, tables_device, offsets, num_hots, mode, options);
  const int batch = detail::GroupedBatch(num_tables, batch_per_table);
  if (batch <= 0) return;
  const void* bits = detail::GroupAlignmentBits(reinterpret_cast<const void* const*>(tables_host), num_tables);
  const int codes = detail::QuantizedForwardCodesPerLane(embed_width, bits);
  CUEMBED_ASSERT(reinterpret_cast<uintptr_t>(ret) % 16 == 0);
  const detail::QuantizedForwardLaunch f =
      detail::PlanQuantizedForward(embed_width, codes, batch, num_hots, offsets != nullptr, weights != nullptr,
                                   sizeof(IndexT), sizeof(OutT), detail::CurrentDeviceShape());
  const OutT* w = reinterpret_cast<const OutT*>(weights);
  OutT* out = reinterpret_cast<OutT*>(ret);
  const bool is_mean = mode == CombineMode::kMean;
  if (codes == 16)
    detail::LaunchGatherReduceQuantizedGrouped<OutT, IndexT, OffsetT, 16>(
        tables_device, batch_per_table, num_tables, embed_width, indices, offsets, w, batch, num_hots, is_mean, out, f,
        stream, options);
  else if (codes == 8)
    detail::LaunchGatherReduceQuantizedGrouped<OutT, IndexT, OffsetT, 8>(
        tables_device, batch_per_table, num_tables, embed_width, indices, offsets, w, batch, num_hots, is_mean, out, f,
        stream, options);
  else
    detail::LaunchGatherReduceQuantizedGrouped<OutT, IndexT, OffsetT, 4>(
        tables_device, batch_per_table, num_tables, embed_width, indices, offsets, w, batch, num_hots, is_mean, out, f,
        stream, options);
}

//! ... with the process-wide default options (DefaultForwardOptions()).
template <typename OutputT, typename IndexT, typename OffsetT>
void EmbeddingForwardQuantizedGrouped(const uint8_t* const* tables_host,
                                      const uint8_t* const* tables_device,
                                      const int num_tables,
                                      const int embed_width,
                                      const IndexT* indices,
                                      const OffsetT* offsets,
                                      const OutputT* weights,
                                      const int batch_per_table,
                                      const int num_hots,
                                      const CombineMode mode,
                                      OutputT* ret,
                                      const hipStream_t stream = 0) {
  EmbeddingForwardQuantizedGrouped<OutputT, IndexT, OffsetT>(tables_host, tables_device, num_tables, embed_width, indices,
                                                             offsets, weights, batch_per_table, num_hots, mode, ret,
                                                             stream, DefaultForwardOptions());
}

}  // namespace cuembed

#endif  // CUEMBED_INCLUDE_GROUPED_LOOKUP_HPP_
