// MI355X (gfx950 / CDNA4) forward on a group of fused 4-bit row-wise tables of DIFFERENT widths in one launch --
// header-only host API (an extension: quantized_mixed_group_lookup.hpp is the group of fused 8-bit tables,
// quantized_4bit_lookup.hpp the single fused 4-bit table).
//
//   EmbeddingForwardQuantized4BitMixedGroup   EmbeddingForwardQuantized4Bit (sum / mean) on T fused tables of any widths
//   Quantized4BitMixedGroupCodesPerLane       N, the codes of one lane (32, 16 or 8), for these pointers and widths
//   FillQuantized4BitMixedGroupDescriptor     fills a HOST copy of the per-(group, B, N) descriptor
//                                             (MixedGroupDescriptorBytes(T) bytes, as every mixed group's)
//
// Layout (quantized_4bit_mixed_group_gather_kernels.hpp): the input is the mixed group's -- bag g = t * B + b, CSR
// indices[nnz] / offsets[T * B + 1] / optional weights[nnz], or fixed hotness indices[T, B, H]; table t is [rows_t,
// W_t / 2 + 4] bytes (two codes a byte, fp16 scale, fp16 bias), W_t % 8 == 0; the result is out[B, D] of OutputT, D = sum
// W_t, bag (t, b) at columns [c_t, c_t + W_t) of row b: the results of T calls of EmbeddingForwardQuantized4Bit
// concatenated on dimension 1, with the same bits.
//
// N is one value for the launch: the largest of 32, 16 and 8 that divides every W_t.  A lane's N / 2 bytes of codes are
// one load that needs 4-byte alignment only, which the row pitch gives when the base has it: every base must be 4-byte
// aligned (asserted) and alignment never narrows N.  Unlike the single-table call a row may need more lanes than a
// workgroup has -- the kernel loops over its columns -- so a wide row never narrows N either (W = 8,224 takes N = 32
// here, 16 there).  `ret` is 16-byte aligned (asserted): every c_t and D are multiples of N.
//
// The conventions of EmbeddingForwardQuantizedMixedGroup hold: the caller builds the pointer arrays (host and device
// copy), the widths on the host and the device descriptor once; the library copies nothing per call and allocates
// nothing; the call is asynchronous on `stream`, one kernel node in a captured graph, and CUEMBED_ASSERTs on misuse.  Of
// ForwardOptions, row_loads (one host value for the group) is honoured; row_loads_device and sample_order must be null
// (refused, not ignored); there is no concat.  Limits: T * B <= INT_MAX, D <= INT_MAX, workgroups <= INT_MAX.
#ifndef CUEMBED_INCLUDE_QUANTIZED_4BIT_MIXED_GROUP_LOOKUP_HPP_
#define CUEMBED_INCLUDE_QUANTIZED_4BIT_MIXED_GROUP_LOOKUP_HPP_

#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "cuembed/include/cuembed_assert.hpp"
#include "cuembed/include/mixed_group_lookup.hpp"
#include "cuembed/include/quantized_4bit_lookup.hpp"
#include "cuembed/include/quantized_4bit_mixed_group_gather_kernels.hpp"

namespace cuembed {

namespace detail {

//! N for tables whose base pointers OR to `bits`: the format's checks on every table (W_t % 8 == 0, a 4-byte aligned
//! base), then the widest lane that divides every width.
inline int Quantized4BitMixedGroupCodesPerLaneOfBits(const uintptr_t bits, const int* widths_host, const int num_tables) {
  CUEMBED_ASSERT(widths_host != nullptr && num_tables >= 1);
  int n = 32;
  for (int t = 0; t < num_tables; ++t) {
    CheckQuantized4BitTable(widths_host[t], reinterpret_cast<const void*>(bits));
    while (widths_host[t] % n != 0) n /= 2;   // (stops at 8 at the latest: W_t % 8 == 0)
  }
  return n;
}

template <typename OutT, typename IndexT, typename OffsetT, int N>
inline void LaunchGatherReduceQuantized4BitMixedGroup(const uint8_t* const* tables, const MixedGroupEntry* descriptor,
                                                      const int num_tables, const int batch_per_table,
                                                      const IndexT* indices, const OffsetT* offsets, const OutT* weights,
                                                      const int num_hots, const bool is_mean, OutT* out,
                                                      const MixedGroupPlan& plan, hipStream_t stream,
                                                      const ForwardOptions& options) {
  const bool stream_rows = options.row_loads == RowLoadPolicy::kStreaming;
  const dim3 block(kMixedGroupBlockThreads, 1, 1);
  const dim3 grid(plan.grid, 1, 1);
  const size_t stage_bytes = MixedGroupStageBytes(plan, offsets != nullptr, num_hots, sizeof(IndexT),
                                                  weights != nullptr ? sizeof(OutT) : 0);
  const bool staged = stage_bytes > 0;
  const auto launch = [&](auto w) {
    constexpr bool kW = decltype(w)::value;
    if (staged)   // (the staged kernel reads no offsets: one instantiation for both offset types)
      GatherReduceQuantized4BitMixedGroupKernel<OutT, IndexT, int32_t, N, kW, true><<<grid, block, stage_bytes, stream>>>(
          tables, descriptor, num_tables, batch_per_table, indices, static_cast<const int32_t*>(nullptr), num_hots, weights,
          is_mean, out, plan.out_width, stream_rows);
    else
      GatherReduceQuantized4BitMixedGroupKernel<OutT, IndexT, OffsetT, N, kW, false><<<grid, block, 0, stream>>>(
          tables, descriptor, num_tables, batch_per_table, indices, offsets, num_hots, weights, is_mean, out,
          plan.out_width, stream_rows);
  };
  if (weights != nullptr) launch(std::true_type{});
  else launch(std::false_type{});
}

}  // namespace detail

/**
 * @brief N, the codes one lane of EmbeddingForwardQuantized4BitMixedGroup pools (32, 16 or 8), for these tables: the
 * largest that divides every width.  `tables_host` may be null (aligned buffers); a base that is not 4-byte aligned or
 * a width that is not a multiple of 8 aborts.  Host arithmetic only.
 */
inline int Quantized4BitMixedGroupCodesPerLane(const void* const* tables_host, const int* widths_host,
                                               const int num_tables) {
  uintptr_t bits = 0;
  if (tables_host != nullptr) bits = reinterpret_cast<uintptr_t>(detail::GroupAlignmentBits(tables_host, num_tables));
  return detail::Quantized4BitMixedGroupCodesPerLaneOfBits(bits, widths_host, num_tables);
}

/**
 * @brief FillQuantizedMixedGroupDescriptor for fused 4-bit tables: entry t < num_tables of `host_blob`
 * (MixedGroupDescriptorBytes(num_tables) bytes, 4-byte aligned) is {W_t, c_t, L_t = min(W_t / codes_per_lane,
 * block_threads), first workgroup}; entry num_tables is {0, D, 0, grid}.  Host arithmetic only.  Returns the grid.
 *
 * @param codes_per_lane  Quantized4BitMixedGroupCodesPerLane(...) of the call the descriptor is for
 * @param block_threads   kMixedGroupBlockThreads for EmbeddingForwardQuantized4BitMixedGroup
 */
inline int FillQuantized4BitMixedGroupDescriptor(const int* widths_host, const int num_tables, const int codes_per_lane,
                                                 const int batch_per_table, const int block_threads, void* host_blob) {
  CUEMBED_ASSERT(host_blob != nullptr && reinterpret_cast<uintptr_t>(host_blob) % 4 == 0);
  CUEMBED_ASSERT(codes_per_lane == 32 || codes_per_lane == 16 || codes_per_lane == 8);
  return detail::PlanMixedGroupLanes(widths_host, num_tables, codes_per_lane, batch_per_table, block_threads,
                                     static_cast<detail::MixedGroupEntry*>(host_blob))
      .grid;
}

/**
 * @brief EmbeddingForwardQuantized4Bit (sum / mean) on a group of `num_tables` fused 4-bit tables of ANY widths, in one
 * launch: ret[b, c_t : c_t + W_t] = combine_j weights[.] * value(tables[t][indices[.], :]) over the lookups of bag
 * t * batch_per_table + b.  Bit-identical to num_tables calls of EmbeddingForwardQuantized4Bit concatenated on
 * dimension 1.
 *
 * @tparam OutputT  result and weight element type: float or __half
 *
 * @param tables_host        [num_tables] table base pointers, 4-byte aligned, in HOST memory (read here, checked)
 * @param tables_device      the same pointers in DEVICE memory (read by the kernel)
 * @param widths_host        [num_tables] values per row W_t (a row is W_t / 2 + 4 bytes), in HOST memory, multiples of 8
 * @param descriptor_device  FillQuantized4BitMixedGroupDescriptor(widths_host, num_tables,
 *                           Quantized4BitMixedGroupCodesPerLane(tables_host, widths_host, num_tables), batch_per_table,
 *                           kMixedGroupBlockThreads, .) copied to DEVICE memory, 4-byte aligned
 * @param indices            CSR: [nnz]; fixed hotness: [T, B, num_hots]; ids of table t are rows of tables[t]
 * @param offsets            CSR: [T * B + 1], or nullptr
 * @param weights            per-lookup weights in OutputT (same layout as indices) or nullptr
 * @param batch_per_table    B; T * B <= INT_MAX
 * @param num_hots           fixed hotness (the same for every table), 0 for CSR
 * @param mode               kSum or kMean
 * @param ret                [B, D], contiguous, 16-byte aligned, D = sum of widths_host
 */
template <typename OutputT, typename IndexT, typename OffsetT>
void EmbeddingForwardQuantized4BitMixedGroup(const uint8_t* const* tables_host,
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
                "EmbeddingForwardQuantized4BitMixedGroup: output must be float or __half");
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
  const int codes = Quantized4BitMixedGroupCodesPerLane(reinterpret_cast<const void* const*>(tables_host), widths_host,
                                                        num_tables);
  const detail::MixedGroupPlan plan = detail::PlanMixedGroupLanes(widths_host, num_tables, codes, batch_per_table,
                                                                  detail::kMixedGroupBlockThreads, nullptr);
  // N elements of OutT are at least 16 bytes: every ret + (b * D + c_t + column) * sizeof(OutT) is 16-byte aligned
  CUEMBED_ASSERT(plan.out_width % codes == 0);
  const detail::MixedGroupEntry* descriptor = static_cast<const detail::MixedGroupEntry*>(descriptor_device);
  const OutT* w = reinterpret_cast<const OutT*>(weights);
  OutT* out = reinterpret_cast<OutT*>(ret);
  const bool is_mean = mode == CombineMode::kMean;
  const auto launch = [&](auto n) {
    detail::LaunchGatherReduceQuantized4BitMixedGroup<OutT, IndexT, OffsetT, decltype(n)::value>(
        tables_device, descriptor, num_tables, batch_per_table, indices, offsets, w, num_hots, is_mean, out, plan, stream,
        options);
  };
  if (codes == 32) launch(std::integral_constant<int, 32>{});
  else if (codes == 16) launch(std::integral_constant<int, 16>{});
  else launch(std::integral_constant<int, 8>{});
}

//! ... with the process-wide default row-load policy (and no other option).
template <typename OutputT, typename IndexT, typename OffsetT>
void EmbeddingForwardQuantized4BitMixedGroup(const uint8_t* const* tables_host,
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
  EmbeddingForwardQuantized4BitMixedGroup<OutputT, IndexT, OffsetT>(tables_host, tables_device, widths_host,
                                                                    descriptor_device, num_tables, indices, offsets,
                                                                    weights, batch_per_table, num_hots, mode, ret, stream,
                                                                    options);
}

}  // namespace cuembed

#endif  // CUEMBED_INCLUDE_QUANTIZED_4BIT_MIXED_GROUP_LOOKUP_HPP_
