// MI355X (gfx950 / CDNA4) forward on a group of fused 8-bit row-wise tables of DIFFERENT widths in one launch --
// header-only host API (an extension: mixed_group_lookup.hpp is the group of plain tables, quantized_lookup.hpp the
// single fused table, grouped_lookup.hpp the same-width group of either).
//
//   EmbeddingForwardQuantizedMixedGroup   EmbeddingForwardQuantized (sum / mean) on T fused tables of any widths
//   QuantizedMixedGroupCodesPerLane       N, the codes of one lane (16, 8 or 4), for these pointers and widths
//   FillQuantizedMixedGroupDescriptor     fills a HOST copy of the per-(group, B, N) descriptor
//                                         (MixedGroupDescriptorBytes(T) bytes, as the plain group's)
//
// Layout (quantized_mixed_group_gather_kernels.hpp): the input is the mixed group's -- bag g = t * B + b, CSR indices[nnz]
// / offsets[T * B + 1] / optional weights[nnz], or fixed hotness indices[T, B, H]; table t is [rows_t, W_t + 8] bytes
// (W_t codes, fp32 scale, fp32 bias); the result is out[B, D] of OutputT, D = sum W_t, bag (t, b) at columns [c_t, c_t +
// W_t) of row b: the results of T calls of EmbeddingForwardQuantized concatenated on dimension 1, with the same bits.
//
// N is one value for the launch, the single-table rules (QuantizedCodesPerLane, QuantizedForwardCodesPerLane) applied to
// every table: 16 when every W_t is a multiple of 16 and every base 8-byte aligned, 8 when every W_t is a multiple of 8
// and every base 8-byte aligned, else 4 (every W_t a multiple of 4 and every base 4-byte aligned: required).  Unlike the
// single-table call a row may need more lanes than a workgroup has -- the kernel loops over its columns -- so the width
// never narrows 16 to 8.  `ret` is 16-byte aligned (asserted, as EmbeddingForwardQuantized does) and so never narrows N
// either: every c_t and D are multiples of N.
//
// The conventions of EmbeddingForwardMixedGroup hold: the caller builds the pointer arrays (host and device copy), the
// widths on the host and the device descriptor once; the library copies nothing per call and allocates nothing; the call
// is asynchronous on `stream`, one kernel node in a captured graph, and CUEMBED_ASSERTs on misuse.  Of ForwardOptions,
// row_loads (one host value for the group) is honoured; row_loads_device and sample_order must be null (refused, not
// ignored); there is no concat.  Limits: T * B <= INT_MAX, D <= INT_MAX, workgroups <= INT_MAX.
#ifndef CUEMBED_INCLUDE_QUANTIZED_MIXED_GROUP_LOOKUP_HPP_
#define CUEMBED_INCLUDE_QUANTIZED_MIXED_GROUP_LOOKUP_HPP_

#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "cuembed/include/cuembed_assert.hpp"
#include "cuembed/include/mixed_group_lookup.hpp"
#include "cuembed/include/quantized_lookup.hpp"
#include "cuembed/include/quantized_mixed_group_gather_kernels.hpp"

namespace cuembed {

namespace detail {

//! N for tables whose base pointers OR to `bits`: the single-table rule on every width, the narrowest one wins.
inline int QuantizedMixedGroupCodesPerLaneOfBits(const uintptr_t bits, const int* widths_host, const int num_tables) {
  CUEMBED_ASSERT(widths_host != nullptr && num_tables >= 1);
  const void* base = reinterpret_cast<const void*>(bits);
  int n = 16;
  for (int t = 0; t < num_tables; ++t) {
    const int codes = QuantizedCodesPerLane(widths_host[t], base);   // 8 or 4; asserts W_t % 4 and the 4-byte alignment
    const int of_table = (codes == 8 && widths_host[t] % 16 == 0) ? 16 : codes;
    if (of_table < n) n = of_table;
  }
  return n;
}

template <typename OutT, typename IndexT, typename OffsetT, int N>
inline void LaunchGatherReduceQuantizedMixedGroup(const uint8_t* const* tables, const MixedGroupEntry* descriptor,
                                                  const int num_tables, const int batch_per_table, const IndexT* indices,
                                                  const OffsetT* offsets, const OutT* weights, const int num_hots,
                                                  const bool is_mean, OutT* out, const MixedGroupPlan& plan,
                                                  hipStream_t stream, const ForwardOptions& options) {
  const bool stream_rows = options.row_loads == RowLoadPolicy::kStreaming;
  const dim3 block(kMixedGroupBlockThreads, 1, 1);
  const dim3 grid(plan.grid, 1, 1);
  const size_t stage_bytes = MixedGroupStageBytes(plan, offsets != nullptr, num_hots, sizeof(IndexT),
                                                  weights != nullptr ? sizeof(OutT) : 0);
  const bool staged = stage_bytes > 0;
  const auto launch = [&](auto w) {
    constexpr bool kW = decltype(w)::value;
    if (staged)   // (the staged kernel reads no offsets: one instantiation for both offset types)
      GatherReduceQuantizedMixedGroupKernel<OutT, IndexT, int32_t, N, kW, true><<<grid, block, stage_bytes, stream>>>(
          tables, descriptor, num_tables, batch_per_table, indices, static_cast<const int32_t*>(nullptr), num_hots, weights,
          is_mean, out, plan.out_width, stream_rows);
    else
      GatherReduceQuantizedMixedGroupKernel<OutT, IndexT, OffsetT, N, kW, false><<<grid, block, 0, stream>>>(
          tables, descriptor, num_tables, batch_per_table, indices, offsets, num_hots, weights, is_mean, out,
          plan.out_width, stream_rows);
  };
  if (weights != nullptr) launch(std::true_type{});
  else launch(std::false_type{});
}

}  // namespace detail

/**
 * @brief N, the codes one lane of EmbeddingForwardQuantizedMixedGroup pools (16, 8 or 4), for these tables.
 * `tables_host` may be null (aligned buffers).  Host arithmetic only.
 */
inline int QuantizedMixedGroupCodesPerLane(const void* const* tables_host, const int* widths_host, const int num_tables) {
  uintptr_t bits = 0;
  if (tables_host != nullptr) bits = reinterpret_cast<uintptr_t>(detail::GroupAlignmentBits(tables_host, num_tables));
  return detail::QuantizedMixedGroupCodesPerLaneOfBits(bits, widths_host, num_tables);
}

/**
 * @brief FillMixedGroupDescriptor for fused tables: entry t < num_tables of `host_blob` (MixedGroupDescriptorBytes(
 * num_tables) bytes, 4-byte aligned) is {W_t, c_t, L_t = min(W_t / codes_per_lane, block_threads), first workgroup};
 * entry num_tables is {0, D, 0, grid}.  Host arithmetic only.  Returns the grid.
 *
 * @param codes_per_lane  QuantizedMixedGroupCodesPerLane(...) of the call the descriptor is for
 * @param block_threads   kMixedGroupBlockThreads for EmbeddingForwardQuantizedMixedGroup
 */
inline int FillQuantizedMixedGroupDescriptor(const int* widths_host, const int num_tables, const int codes_per_lane,
                                             const int batch_per_table, const int block_threads, void* host_blob) {
  CUEMBED_ASSERT(host_blob != nullptr && reinterpret_cast<uintptr_t>(host_blob) % 4 == 0);
  CUEMBED_ASSERT(codes_per_lane == 16 || codes_per_lane == 8 || codes_per_lane == 4);
  return detail::PlanMixedGroupLanes(widths_host, num_tables, codes_per_lane, batch_per_table, block_threads,
                                     static_cast<detail::MixedGroupEntry*>(host_blob))
      .grid;
}

/**
 * @brief EmbeddingForwardQuantized (sum / mean) on a group of `num_tables` fused 8-bit tables of ANY widths, in one
 * launch: ret[b, c_t : c_t + W_t] = combine_j weights[.] * value(tables[t][indices[.], :]) over the lookups of bag
 * t * batch_per_table + b.  Bit-identical to num_tables calls of EmbeddingForwardQuantized concatenated on dimension 1.
 *
 * @tparam OutputT  result and weight element type: float or __half
 *
 * @param tables_host        [num_tables] table base pointers, in HOST memory (read here, for N)
 * @param tables_device      the same pointers in DEVICE memory (read by the kernel)
 * @param widths_host        [num_tables] codes per row W_t (a row is W_t + 8 bytes), in HOST memory, multiples of 4
 * @param descriptor_device  FillQuantizedMixedGroupDescriptor(widths_host, num_tables, QuantizedMixedGroupCodesPerLane(
 *                           tables_host, widths_host, num_tables), batch_per_table, kMixedGroupBlockThreads, .) copied
 *                           to DEVICE memory, 4-byte aligned
 * @param indices            CSR: [nnz]; fixed hotness: [T, B, num_hots]; ids of table t are rows of tables[t]
 * @param offsets            CSR: [T * B + 1], or nullptr
 * @param weights            per-lookup weights in OutputT (same layout as indices) or nullptr
 * @param batch_per_table    B; T * B <= INT_MAX
 * @param num_hots           fixed hotness (the same for every table), 0 for CSR
 * @param mode               kSum or kMean
 * @param ret                [B, D], contiguous, 16-byte aligned, D = sum of widths_host
 */
template <typename OutputT, typename IndexT, typename OffsetT>
void EmbeddingForwardQuantizedMixedGroup(const uint8_t* const* tables_host,
                                         const uint8_t* const* tables_device,
                                         const int* widths_host,
                                         const void* descriptor_device,
                                         const int num_tables,
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
                "EmbeddingForwardQuantizedMixedGroup: output must be float or __half");
  CUEMBED_ASSERT(tables_host != nullptr && tables_device != nullptr && widths_host != nullptr);
  CUEMBED_ASSERT(descriptor_device != nullptr &&
                 reinterpret_cast<uintptr_t>(descriptor_device) % alignof(detail::MixedGroupEntry) == 0);
  CUEMBED_ASSERT(mode == CombineMode::kSum || mode == CombineMode::kMean);   // (no concat on a group)
  CUEMBED_ASSERT((offsets != nullptr && num_hots == 0) || (offsets == nullptr && num_hots > 0));
  CUEMBED_ASSERT(options.sample_order == nullptr);      // not taken in this version: refused, not ignored
  CUEMBED_ASSERT(options.row_loads_device == nullptr);
  const int batch = detail::GroupedBatch(num_tables, batch_per_table);
  if (batch <= 0) return;
  CUEMBED_ASSERT(ret != nullptr && indices != nullptr);
  CUEMBED_ASSERT(reinterpret_cast<uintptr_t>(ret) % 16 == 0);
  const int codes = QuantizedMixedGroupCodesPerLane(reinterpret_cast<const void* const*>(tables_host), widths_host,
                                                    num_tables);
  const detail::MixedGroupPlan plan = detail::PlanMixedGroupLanes(widths_host, num_tables, codes, batch_per_table,
                                                                  detail::kMixedGroupBlockThreads, nullptr);
  // the store unit min(16, N * sizeof(OutT)) divides every ret + (b * D + c_t + column) * sizeof(OutT): see the kernel
  CUEMBED_ASSERT(plan.out_width % codes == 0);
  const detail::MixedGroupEntry* descriptor = static_cast<const detail::MixedGroupEntry*>(descriptor_device);
  const OutT* w = reinterpret_cast<const OutT*>(weights);
  OutT* out = reinterpret_cast<OutT*>(ret);
  const bool is_mean = mode == CombineMode::kMean;
  const auto launch = [&](auto n) {
    detail::LaunchGatherReduceQuantizedMixedGroup<OutT, IndexT, OffsetT, decltype(n)::value>(
        tables_device, descriptor, num_tables, batch_per_table, indices, offsets, w, num_hots, is_mean, out, plan, stream,
        options);
  };
  if (codes == 16) launch(std::integral_constant<int, 16>{});
  else if (codes == 8) launch(std::integral_constant<int, 8>{});
  else launch(std::integral_constant<int, 4>{});
}

//! ... with the process-wide default row-load policy (and no other option).
template <typename OutputT, typename IndexT, typename OffsetT>
void EmbeddingForwardQuantizedMixedGroup(const uint8_t* const* tables_host,
                                         const uint8_t* const* tables_device,
                                         const int* widths_host,
                                         const void* descriptor_device,
                                         const int num_tables,
                                         const IndexT* indices,
                                         const OffsetT* offsets,
                                         const OutputT* weights,
                                         const int batch_per_table,
                                         const int num_hots,
                                         const CombineMode mode,
                                         OutputT* ret,
                                         const hipStream_t stream = 0) {
  ForwardOptions options;
  options.row_loads = GetForwardRowLoadPolicy();
  EmbeddingForwardQuantizedMixedGroup<OutputT, IndexT, OffsetT>(tables_host, tables_device, widths_host,
                                                                descriptor_device, num_tables, indices, offsets, weights,
                                                                batch_per_table, num_hots, mode, ret, stream, options);
}

}  // namespace cuembed

#endif  // CUEMBED_INCLUDE_QUANTIZED_MIXED_GROUP_LOOKUP_HPP_
