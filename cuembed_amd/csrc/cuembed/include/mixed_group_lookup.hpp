// MI355X (gfx950 / CDNA4) forward on a group of embedding tables of DIFFERENT widths in one launch -- header-only host
// API (an extension: the reference's entry points take one table; grouped_lookup.hpp is the same-width group).
//
//   EmbeddingForwardMixedGroup   EmbeddingForward (sum / mean) on T plain tables of one element type, any widths
//   MixedGroupDescriptorBytes    size of the per-(group, B) device descriptor
//   FillMixedGroupDescriptor     fills a HOST copy of it (host arithmetic only; the caller copies it to the device, once)
//   MixedGroupLaneBytes          the access width the call will take for these pointers and widths
//
// Layout (mixed_group_gather_kernels.hpp): the input is the same-width group's -- bag g = t * B + b, CSR indices[nnz] /
// offsets[T * B + 1] / optional weights[nnz], or fixed hotness indices[T, B, H] --; the result is out[B, D], D = sum W_t,
// bag (t, b) at columns [c_t, c_t + W_t) of row b: torch.cat of T single-table results on dim 1, with the same bits.
//
// The caller builds, once: the table base pointers twice (host copy: read here for the access width; device copy: read
// by the kernel), the widths on the host, and per (group, B, lane bytes) the device descriptor.  The descriptor depends
// on the lane bytes, and those on the alignment of the tables AND of the result: the widest of 16 / 8 / 4 bytes that
// every table base, the ret base, D * sizeof, every c_t * sizeof and every W_t * sizeof allow (the least aligned one
// decides for the launch).  A caller whose `ret` changes alignment between calls keeps one descriptor per lane width;
// handing the call a descriptor filled for another lane width, B or block size is a contract violation the library
// cannot see (it never reads device memory on the host).
//
// The library copies nothing per call and allocates nothing; the call is asynchronous on `stream`, one kernel node in a
// captured graph, and CUEMBED_ASSERTs (print and abort) on misuse.  Forward only, sum and mean only, fp32 accumulation
// in lookup order.  Of ForwardOptions, row_loads (one host value for the group) is honoured; row_loads_device and
// sample_order must be null (refused, not ignored); reduction_order is not consulted.
// Limits: T * B <= INT_MAX, D <= INT_MAX, workgroups = sum_t ceil(B / spb_t) <= INT_MAX.  The workgroup prefix is read
// from device memory, not staged in LDS: there is no limit on T beyond those.
#ifndef CUEMBED_INCLUDE_MIXED_GROUP_LOOKUP_HPP_
#define CUEMBED_INCLUDE_MIXED_GROUP_LOOKUP_HPP_

#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>
#include <type_traits>

#include "cuembed/include/cuembed_assert.hpp"
#include "cuembed/include/embedding_lookup.hpp"
#include "cuembed/include/group_host_plan.hpp"
#include "cuembed/include/grouped_lookup.hpp"
#include "cuembed/include/mixed_group_gather_kernels.hpp"

namespace cuembed {

namespace detail {

//! What one pass over the widths gives: the grid, the widest workgroup in bags (for the LDS staging) and D.
struct MixedGroupPlan {
  int grid;        //!< sum_t ceil(B / spb_t)
  int max_slots;   //!< max_t spb_t
  int out_width;   //!< D
};

//! The launch arithmetic of a mixed group, and -- with `entries` non-null -- its descriptor.  Host only.
inline MixedGroupPlan PlanMixedGroup(const int* widths_host, const int num_tables, const int elem_bytes,
                                     const int lane_bytes, const int batch_per_table, const int block_threads,
                                     MixedGroupEntry* entries) {
  CUEMBED_ASSERT(widths_host != nullptr && num_tables >= 1 && batch_per_table >= 0);
  CUEMBED_ASSERT(elem_bytes == 2 || elem_bytes == 4);
  CUEMBED_ASSERT(lane_bytes == 16 || lane_bytes == 8 || lane_bytes == 4);
  CUEMBED_ASSERT(block_threads >= 64 && block_threads <= kMaxBlockThreads && block_threads % 64 == 0);
  CUEMBED_ASSERT(static_cast<int64_t>(num_tables) * batch_per_table <= INT_MAX);
  const int n = lane_bytes / elem_bytes;
  int64_t column = 0, blocks = 0;
  MixedGroupPlan plan{0, 0, 0};
  for (int t = 0; t < num_tables; ++t) {
    const int width = widths_host[t];
    CUEMBED_ASSERT(width > 0);
    CUEMBED_ASSERT((static_cast<int64_t>(width) * elem_bytes) % lane_bytes == 0);
    CUEMBED_ASSERT((column * elem_bytes) % lane_bytes == 0);
    const int row_lanes = width / n;
    const int lanes = row_lanes < block_threads ? row_lanes : block_threads;
    const int slots = block_threads / lanes;
    if (entries != nullptr) entries[t] = MixedGroupEntry{width, static_cast<int32_t>(column), lanes, static_cast<int32_t>(blocks)};
    if (slots > plan.max_slots) plan.max_slots = slots;
    column += width;
    blocks += (static_cast<int64_t>(batch_per_table) + slots - 1) / slots;
    CUEMBED_ASSERT(column <= INT_MAX && blocks <= INT_MAX);
  }
  CUEMBED_ASSERT((column * elem_bytes) % lane_bytes == 0);
  if (entries != nullptr) entries[num_tables] = MixedGroupEntry{0, static_cast<int32_t>(column), 0, static_cast<int32_t>(blocks)};
  plan.grid = static_cast<int>(blocks);
  plan.out_width = static_cast<int>(column);
  return plan;
}

//! Dynamic LDS of the staged kernel: fixed hotness whose widest workgroup's indices (+ weights) fit the staging budget of
//! the single-table plan.  0: the indices are read where they lie (CSR, or a share past kMaxStageBytes).
inline size_t MixedGroupStageBytes(const MixedGroupPlan& plan, const bool is_csr, const int num_hots,
                                   const size_t index_bytes, const size_t weight_bytes) {
  if (is_csr || num_hots <= 0) return 0;
  const size_t bytes = static_cast<size_t>(plan.max_slots) * num_hots * (index_bytes + weight_bytes);
  return bytes <= static_cast<size_t>(kMaxStageBytes) ? bytes : 0;
}

template <typename ElemT, typename IndexT, typename OffsetT, int N>
inline void LaunchGatherReduceMixedGroup(const ElemT* const* tables, const MixedGroupEntry* descriptor,
                                         const int num_tables, const int batch_per_table, const IndexT* indices,
                                         const OffsetT* offsets, const ElemT* weights, const int num_hots,
                                         const bool is_mean, ElemT* out, const MixedGroupPlan& plan, hipStream_t stream,
                                         const ForwardOptions& options) {
  const bool stream_rows = options.row_loads == RowLoadPolicy::kStreaming;
  const dim3 block(kMixedGroupBlockThreads, 1, 1);
  const dim3 grid(plan.grid, 1, 1);
  const size_t stage_bytes = MixedGroupStageBytes(plan, offsets != nullptr, num_hots, sizeof(IndexT),
                                                  weights != nullptr ? sizeof(ElemT) : 0);
  const bool staged = stage_bytes > 0;
  const auto launch = [&](auto w) {
    constexpr bool kW = decltype(w)::value;
    if (staged)   // (the staged kernel reads no offsets: one instantiation for both offset types)
      GatherReduceMixedGroupKernel<ElemT, IndexT, int32_t, N, kW, true><<<grid, block, stage_bytes, stream>>>(
          tables, descriptor, num_tables, batch_per_table, indices, static_cast<const int32_t*>(nullptr), num_hots, weights,
          is_mean, out,
          plan.out_width, stream_rows);
    else
      GatherReduceMixedGroupKernel<ElemT, IndexT, OffsetT, N, kW, false><<<grid, block, 0, stream>>>(
          tables, descriptor, num_tables, batch_per_table, indices, offsets, num_hots, weights, is_mean, out,
          plan.out_width, stream_rows);
  };
  if (weights != nullptr) launch(std::true_type{});
  else launch(std::false_type{});
}

}  // namespace detail

//! Bytes of the device descriptor of a mixed group of `num_tables` tables (num_tables + 1 entries of 16 bytes).
inline size_t MixedGroupDescriptorBytes(const int num_tables) {
  CUEMBED_ASSERT(num_tables >= 1);
  return (static_cast<size_t>(num_tables) + 1) * sizeof(detail::MixedGroupEntry);
}

//! The block size EmbeddingForwardMixedGroup launches with: what FillMixedGroupDescriptor must be given.
constexpr int kMixedGroupBlockThreads = detail::kMixedGroupBlockThreads;

/**
 * @brief The access width (16, 8 or 4 bytes per lane) EmbeddingForwardMixedGroup takes for this group and result:
 * the widest that every table base, `ret`, D * elem_bytes, every c_t * elem_bytes and every W_t * elem_bytes allow.
 * `tables_host` and `ret` may be null (aligned buffers).  Host arithmetic only.
 */
inline int MixedGroupLaneBytes(const void* const* tables_host, const int* widths_host, const int num_tables,
                               const int elem_bytes, const void* ret) {
  uintptr_t bits = reinterpret_cast<uintptr_t>(ret);
  if (tables_host != nullptr)
    bits |= reinterpret_cast<uintptr_t>(detail::GroupAlignmentBits(tables_host, num_tables));
  return detail::MixedGroupLaneBytesOfBits(bits, widths_host, num_tables, elem_bytes);
}

/**
 * @brief Fills the HOST buffer `host_blob` (MixedGroupDescriptorBytes(num_tables) bytes, 4-byte aligned) with the
 * words the kernel reads per table: width, column base c_t, lanes per bag L_t = min(W_t * elem_bytes / lane_bytes,
 * block_threads) and the workgroup prefix for this batch_per_table (spb_t = block_threads / L_t bags per workgroup);
 * entry num_tables closes the prefixes with D and the grid.  Host arithmetic only: the caller copies the buffer to the
 * device, once per (group, batch_per_table, lane_bytes).  Returns the grid = sum_t ceil(batch_per_table / spb_t).
 *
 * @param lane_bytes     MixedGroupLaneBytes(...) of the call the descriptor is for
 * @param block_threads  kMixedGroupBlockThreads for EmbeddingForwardMixedGroup
 */
inline int FillMixedGroupDescriptor(const int* widths_host, const int num_tables, const int elem_bytes,
                                    const int lane_bytes, const int batch_per_table, const int block_threads,
                                    void* host_blob) {
  CUEMBED_ASSERT(host_blob != nullptr && reinterpret_cast<uintptr_t>(host_blob) % 4 == 0);
  return detail::PlanMixedGroup(widths_host, num_tables, elem_bytes, lane_bytes, batch_per_table, block_threads,
                                static_cast<detail::MixedGroupEntry*>(host_blob))
      .grid;
}

/**
 * @brief EmbeddingForward (sum / mean) on a group of `num_tables` plain tables of one element type and ANY widths, in
 * one launch: ret[b, c_t : c_t + W_t] = combine_j weights[.] * tables[t][indices[.], :] over the lookups of bag
 * t * batch_per_table + b.  Bit-identical to num_tables calls of EmbeddingForward (fp32 accumulation) concatenated on
 * dimension 1.
 *
 * @tparam InputT   table element type (float, __half or __hip_bfloat16)
 * @tparam OutputT  result element type (must equal InputT)
 *
 * @param tables_host        [num_tables] table base pointers, in HOST memory (read here, for the access width)
 * @param tables_device      the same pointers in DEVICE memory (read by the kernel)
 * @param widths_host        [num_tables] elements per row of each table, in HOST memory (row bytes a multiple of 4)
 * @param descriptor_device  FillMixedGroupDescriptor(widths_host, num_tables, sizeof(InputT), MixedGroupLaneBytes(
 *                           tables_host, widths_host, num_tables, sizeof(InputT), ret), batch_per_table,
 *                           kMixedGroupBlockThreads, .) copied to DEVICE memory, 4-byte aligned
 * @param num_tables         T >= 1
 * @param indices            CSR: [nnz]; fixed hotness: [T, B, num_hots]; ids of table t are rows of tables[t]
 * @param offsets            CSR: [T * B + 1], or nullptr
 * @param weights            per-lookup weights in the tables' type (same layout as indices) or nullptr
 * @param batch_per_table    B; T * B <= INT_MAX
 * @param num_hots           fixed hotness (the same for every table), 0 for CSR
 * @param mode               kSum or kMean
 * @param ret                [B, D], contiguous, D = sum of widths_host
 */
template <typename InputT, typename OutputT, typename IndexT, typename OffsetT>
void EmbeddingForwardMixedGroup(const InputT* const* tables_host,
                                const InputT* const* tables_device,
                                const int* widths_host,
                                const void* descriptor_device,
                                const int num_tables,
                                const IndexT* indices,
                                const OffsetT* offsets,
                                const GetElemT<InputT>* weights,
                                const int batch_per_table,
                                const int num_hots,
                                const CombineMode mode,
                                OutputT* ret,
                                const hipStream_t stream,
                                const ForwardOptions& options) {
  static_assert(std::is_same<InputT, OutputT>::value, "EmbeddingForwardMixedGroup: OutputT must equal InputT");
  using HostElemT = GetElemT<InputT>;
  static_assert(std::is_same<HostElemT, float>::value || std::is_same<HostElemT, __half>::value ||
                    std::is_same<HostElemT, __hip_bfloat16>::value,
                "EmbeddingForwardMixedGroup: table elements must be float, __half or __hip_bfloat16");
  using ElemT = detail::DeviceElemT<HostElemT>;
  CUEMBED_ASSERT(tables_host != nullptr && tables_device != nullptr && widths_host != nullptr);
  CUEMBED_ASSERT(descriptor_device != nullptr &&
                 reinterpret_cast<uintptr_t>(descriptor_device) % alignof(detail::MixedGroupEntry) == 0);
  CUEMBED_ASSERT(mode == CombineMode::kSum || mode == CombineMode::kMean);
  CUEMBED_ASSERT((offsets != nullptr && num_hots == 0) || (offsets == nullptr && num_hots > 0));
  CUEMBED_ASSERT(options.sample_order == nullptr);      // not taken in this version: refused, not ignored
  CUEMBED_ASSERT(options.row_loads_device == nullptr);
  const int batch = detail::GroupedBatch(num_tables, batch_per_table);
  if (batch <= 0) return;
  CUEMBED_ASSERT(ret != nullptr && indices != nullptr);
  const int lane_bytes = MixedGroupLaneBytes(reinterpret_cast<const void* const*>(tables_host), widths_host, num_tables,
                                             static_cast<int>(sizeof(ElemT)), ret);
  const detail::MixedGroupPlan plan =
      detail::PlanMixedGroup(widths_host, num_tables, static_cast<int>(sizeof(ElemT)), lane_bytes, batch_per_table,
                             detail::kMixedGroupBlockThreads, nullptr);
  const ElemT* const* tables = reinterpret_cast<const ElemT* const*>(tables_device);
  const detail::MixedGroupEntry* descriptor = static_cast<const detail::MixedGroupEntry*>(descriptor_device);
  const ElemT* w = reinterpret_cast<const ElemT*>(weights);
  ElemT* out = reinterpret_cast<ElemT*>(ret);
  const bool is_mean = mode == CombineMode::kMean;
  detail::WithLaneWidth<ElemT>(lane_bytes / static_cast<int>(sizeof(ElemT)), [&](auto n) {
    detail::LaunchGatherReduceMixedGroup<ElemT, IndexT, OffsetT, decltype(n)::value>(
        tables, descriptor, num_tables, batch_per_table, indices, offsets, w, num_hots, is_mean, out, plan, stream,
        options);
  });
}

//! ... with the process-wide default row-load policy (and no other option).
template <typename InputT, typename OutputT, typename IndexT, typename OffsetT>
void EmbeddingForwardMixedGroup(const InputT* const* tables_host,
                                const InputT* const* tables_device,
                                const int* widths_host,
                                const void* descriptor_device,
                                const int num_tables,
                                const IndexT* indices,
                                const OffsetT* offsets,
                                const GetElemT<InputT>* weights,
                                const int batch_per_table,
                                const int num_hots,
                                const CombineMode mode,
                                OutputT* ret,
                                const hipStream_t stream = 0) {
  ForwardOptions options;
  options.row_loads = GetForwardRowLoadPolicy();
  EmbeddingForwardMixedGroup<InputT, OutputT, IndexT, OffsetT>(tables_host, tables_device, widths_host,
                                                               descriptor_device, num_tables, indices, offsets, weights,
                                                               batch_per_table, num_hots, mode, ret, stream, options);
}

}  // namespace cuembed

#endif  // CUEMBED_INCLUDE_MIXED_GROUP_LOOKUP_HPP_
