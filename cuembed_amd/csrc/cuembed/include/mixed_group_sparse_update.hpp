// MI355X (gfx950 / CDNA4) sparse optimizer step on a group of tables of DIFFERENT widths, in one launch -- header-only
// host API (an extension: the reference ends at the gradient and takes one table).
//
//   cuembed::SparseRowUpdateMixedGroup<ElemT, IndexT>(tables_host, tables_device, state_host, state_device, widths_host,
//                                                     widths_device, num_tables, row_base_device, max_width, ids, rows,
//                                                     total_entries, options, stream)
//   cuembed::SparseRowAdamMixedGroup<ElemT, IndexT>(tables_host, tables_device, exp_avg_host, exp_avg_device,
//                                                   exp_avg_sq_host, exp_avg_sq_device, widths_host, widths_device,
//                                                   num_tables, row_base_device, max_width, ids, rows, total_entries,
//                                                   options, stream)
//
// consume the compressed gradient of a mixed-width group exactly as EmbeddingBackwardMixedGroup leaves it
// (mixed_group_backward.hpp: `ids` ascending GLOBAL rows of the tables laid end to end, `rows` [total_entries, max_width]
// with entry k's gradient in rows[k, :W_t] and the columns from W_t on unspecified) and update the named rows of T
// separate tensors of T widths, and of their T (or 2 T) state tensors, in place.  Per-element state is fp32 [rows_t, W_t]
// with its own pitch W_t, row-wise state fp32 [rows_t].  The padded columns are never read.
//
// As in SparseRowUpdateGrouped the caller builds the pointer arrays TWICE, once: in host memory, which the library reads
// to choose the lane width, and in device memory, which the kernel reads; the widths likewise.  ONE lane width serves
// the launch, by the mixed group's rule (PlanMixedGroupColumns): the widest of 16 / 8 / 4 bytes that every W_t *
// sizeof(ElemT), every table base, `rows` and -- for rules with per-element state -- every such state base allow
// (max_width is one of the widths, so the gradient pitch is covered).  Nothing is allocated, copied or read back and the
// host never waits: the call can be captured.  Misuse CUEMBED_ASSERTs (prints and aborts).
//
// The tables and all state tensors have the bits of T single-table steps (SparseRowUpdate / SparseRowAdam), each run at
// width W_t with the group's lane width: a row's arithmetic depends on that row alone, and the one ordered quantity, the
// row-wise rules' sum of g^2, is summed in the order (W_t, N) fix -- per-lane sums in slice order, then the butterfly
// over PlanUpdate's group for W_t / N lanes (mixed_group_update_kernels.hpp).
//
// Not taken, each refused: stochastic rounding, counts[pieces], tables behind the row cache (there is no placed variant),
// a ragged gradient layout, quantized or mixed-dtype groups.
#ifndef CUEMBED_INCLUDE_MIXED_GROUP_SPARSE_UPDATE_HPP_
#define CUEMBED_INCLUDE_MIXED_GROUP_SPARSE_UPDATE_HPP_

#include "cuembed/include/group_host_plan.hpp"
#include "cuembed/include/grouped_sparse_update.hpp"
#include "cuembed/include/mixed_group_update_kernels.hpp"

namespace cuembed {

namespace detail {

//! The lane bytes of a mixed-width step: PlanMixedGroupColumns over the widths and `bits` (every table base and `rows`
//! OR-ed), narrowed as in UpdateLaneBytes until every per-element state base (`state_bits`, OR-ed; 0 = none) is aligned
//! to the fp32 packs a lane moves.  Host only.
inline int MixedGroupUpdateLaneBytes(const int* widths_host, const int num_tables, const int elem_bytes,
                                     const uintptr_t bits, const uintptr_t state_bits) {
  int bytes = MixedGroupLaneBytesOfBits(bits, widths_host, num_tables, elem_bytes);
  const auto state_align = [&](int b) { const int n = b / elem_bytes; return 4 * (n < 4 ? n : 4); };
  while (bytes > 4 && state_bits % state_align(bytes) != 0) bytes /= 2;
  CUEMBED_ASSERT(state_bits % state_align(bytes) == 0);
  return bytes;
}

//! The grid of a mixed-width step (pure host arithmetic), in workgroups of kUpdateBlockThreads -- four wavefronts, one
//! tile of 64 entries each per turn: PlanUpdate's grid for such tiles, as many workgroups as there are tiles to give every
//! wavefront one, at most what the device holds at once; the rest is the grid stride.
inline unsigned PlanMixedGroupUpdate(const int64_t total_entries, const DeviceShape& dev) {
  const int64_t per_block = static_cast<int64_t>(kMixedUpdateWave) * kMixedUpdateWaves;
  const int64_t needed = (total_entries + per_block - 1) / per_block;
  const int64_t resident = static_cast<int64_t>(dev.compute_units) * (dev.lanes_per_cu / kUpdateBlockThreads);
  return static_cast<unsigned>(needed < resident ? (needed < 1 ? 1 : needed) : resident);
}

//! What a pass does on a table of `lanes_per_row` = W_t / N lanes: the lanes an entry takes (PlanUpdate's group, or the
//! whole wavefront for a wider row) and the entries a pass serves.
inline void MixedGroupPassOf(const int lanes_per_row, int* lanes_per_entry, int* entries_per_pass) {
  int group = 1;
  while (group < lanes_per_row && group < kMixedUpdateWave) group *= 2;
  *lanes_per_entry = group;
  *entries_per_pass = lanes_per_row > kMixedUpdateWave ? 1 : kMixedUpdateWave / group;
}

//! The checks both mixed steps share after CheckGroupedStep's, and the lane bytes (0: nothing to do).
template <typename ElemT>
inline int CheckMixedGroupStep(SparseStepOptions& o, const void* const* tables_host, const void* tables_device,
                               const int* widths_host, const int* widths_device, const int num_tables,
                               const int64_t* row_base_device, const int max_width, const void* ids, const void* rows,
                               const int64_t total_entries, const float* const* state_host,
                               const float* const* state2_host) {
  CUEMBED_ASSERT(!o.stochastic_rounding && "a mixed-width group's optimizer step rounds to nearest: no stochastic rounding");
  const bool work = CheckGroupedStep(o, tables_host, tables_device, num_tables, row_base_device, ids, rows, total_entries,
                                     nullptr);
  CUEMBED_ASSERT(widths_host != nullptr && widths_device != nullptr);
  uintptr_t bits = reinterpret_cast<uintptr_t>(rows);
  for (int t = 0; t < num_tables; ++t) bits |= reinterpret_cast<uintptr_t>(tables_host[t]);
  uintptr_t state_bits = 0;
  for (int t = 0; t < num_tables; ++t) {
    if (state_host != nullptr) state_bits |= reinterpret_cast<uintptr_t>(state_host[t]);
    if (state2_host != nullptr) state_bits |= reinterpret_cast<uintptr_t>(state2_host[t]);
  }
  const int elem_bytes = static_cast<int>(sizeof(ElemT));
  const MixedGroupColumns columns = PlanMixedGroupColumns(widths_host, num_tables, elem_bytes, bits);
  CUEMBED_ASSERT(columns.max_width == max_width && "max_width, the gradient pitch, is the widest table's width");
  if (!work) return 0;
  return MixedGroupUpdateLaneBytes(widths_host, num_tables, elem_bytes, bits, state_bits);
}

//! From the lane bytes to N = 16 / 8 / 4 bytes of ElemT per lane, as an integral constant.
template <typename ElemT, typename WithT>
inline void DispatchMixedLane(const int bytes, const WithT& with_n) {
  constexpr int kMaxN = 16 / static_cast<int>(sizeof(ElemT));
  if (bytes == 16) with_n(Int<kMaxN>());
  else if (bytes == 8) with_n(Int<kMaxN / 2>());
  else with_n(Int<kMaxN / 4>());
}

}  // namespace detail

/**
 * @brief SparseRowUpdate on a group of `num_tables` separate tables of one element type and DIFFERENT widths, in one
 * launch: for every valid entry k, with t the last table with row_base[t] <= ids[k] and r = ids[k] - row_base[t],
 * tables[t][r, :W_t] and the state of row r of table t are updated in place from rows[k, :W_t] by options.rule.  Rows
 * that no valid entry names are neither read nor written; rows[k, W_t:] is never read.
 *
 * @param tables_host / tables_device  [num_tables] table bases, in HOST memory (read here, for the lane width) and in
 *                                     DEVICE memory (read by the kernel)
 * @param state_host / state_device    [num_tables] bases of the fp32 state tensors: both nullptr for kSgd; [rows_t, W_t]
 *                                     each for kAdagrad (host copy required); [rows_t] each for kRowwiseAdagrad (host
 *                                     copy not read)
 * @param widths_host / widths_device  [num_tables] ints, W_t in elements, in HOST and in DEVICE memory
 * @param num_tables       T, 1 <= T <= detail::kGroupedMaxTables
 * @param row_base_device  [num_tables + 1] int64 in DEVICE memory: the exclusive prefix sum of the tables' row counts
 * @param max_width        the widest W_t: the pitch of `rows` in elements
 * @param ids              [total_entries] global rows, valid entries distinct and inside [0, row_base[num_tables])
 * @param rows             [total_entries, max_width] gradient rows, of the tables' type
 * @param options          rule, lr, eps and ONE count source (num_rows, counts -- one word --, or last_id); pieces must be
 *                         1; a count below zero or above total_entries applies nothing; stochastic_rounding aborts
 */
template <typename ElemT, typename IndexT>
void SparseRowUpdateMixedGroup(const ElemT* const* tables_host,
                               ElemT* const* tables_device,
                               const float* const* state_host,
                               float* const* state_device,
                               const int* widths_host,
                               const int* widths_device,
                               const int num_tables,
                               const int64_t* row_base_device,
                               const int max_width,
                               const IndexT* ids,
                               const ElemT* rows,
                               const int64_t total_entries,
                               const SparseUpdateOptions& options,
                               const hipStream_t stream = 0) {
  static_assert(std::is_same<ElemT, float>::value || std::is_same<ElemT, __half>::value ||
                    std::is_same<ElemT, __hip_bfloat16>::value,
                "SparseRowUpdateMixedGroup: tables must be float, __half or __hip_bfloat16");
  static_assert(std::is_same<IndexT, int32_t>::value || std::is_same<IndexT, int64_t>::value,
                "SparseRowUpdateMixedGroup: ids must be int32_t or int64_t");
  using DevT = detail::DeviceElemT<ElemT>;
  SparseUpdateOptions o = options;
  CUEMBED_ASSERT((o.rule == UpdateRule::kSgd) == (state_device == nullptr));
  const bool per_element = o.rule == UpdateRule::kAdagrad;
  CUEMBED_ASSERT(!per_element || state_host != nullptr);
  const int bytes = detail::CheckMixedGroupStep<DevT>(
      o, reinterpret_cast<const void* const*>(tables_host), tables_device, widths_host, widths_device, num_tables,
      row_base_device, max_width, ids, rows, total_entries, per_element ? state_host : nullptr, nullptr);
  if (bytes == 0) return;
  const detail::MixedGroupTables g = {reinterpret_cast<const void* const*>(tables_device),
                                      const_cast<const float* const*>(state_device), nullptr, row_base_device,
                                      widths_device, num_tables};
  const detail::UpdateCounts counts = detail::CountsOf(o);
  const dim3 grid(detail::PlanMixedGroupUpdate(total_entries, detail::CurrentDeviceShape()));
  const dim3 block(detail::kUpdateBlockThreads);
  const size_t lds = detail::MixedGroupUpdateLdsBytes(num_tables, o.rule == UpdateRule::kSgd ? 0 : 1);
  detail::DispatchMixedLane<DevT>(bytes, [&](auto n) {
    detail::DispatchRule(o.rule, [&](auto rule) {
      constexpr int N = decltype(n)::value;
      constexpr UpdateRule kRule = decltype(rule)::value;
      detail::SparseRowUpdateMixedGroupKernel<DevT, IndexT, N, kRule, detail::kMixedPassesInFlight<kRule, N>>
          <<<grid, block, lds, stream>>>(ids, reinterpret_cast<const DevT*>(rows), g, max_width, total_entries, counts,
                                         o.lr, o.lr_device, o.eps);
    });
  });
}

/**
 * @brief SparseRowAdam on such a group, in one launch: as SparseRowUpdateMixedGroup, with the two moments of every table
 * in tensors of their own.  options.bias_factor_device (AdamClockAdvance's word) serves the whole group.
 *
 * @param exp_avg_host / exp_avg_device        [num_tables] bases of the fp32 [rows_t, W_t] first moments, in HOST and
 *                                             in DEVICE memory
 * @param exp_avg_sq_host / exp_avg_sq_device  the second moments: fp32 [rows_t, W_t] (kAdam; both copies required) or
 *                                             fp32 [rows_t] (kRowwiseAdam; the host copy is not read)
 */
template <typename ElemT, typename IndexT>
void SparseRowAdamMixedGroup(const ElemT* const* tables_host,
                             ElemT* const* tables_device,
                             const float* const* exp_avg_host,
                             float* const* exp_avg_device,
                             const float* const* exp_avg_sq_host,
                             float* const* exp_avg_sq_device,
                             const int* widths_host,
                             const int* widths_device,
                             const int num_tables,
                             const int64_t* row_base_device,
                             const int max_width,
                             const IndexT* ids,
                             const ElemT* rows,
                             const int64_t total_entries,
                             const SparseAdamOptions& options,
                             const hipStream_t stream = 0) {
  static_assert(std::is_same<ElemT, float>::value || std::is_same<ElemT, __half>::value ||
                    std::is_same<ElemT, __hip_bfloat16>::value,
                "SparseRowAdamMixedGroup: tables must be float, __half or __hip_bfloat16");
  static_assert(std::is_same<IndexT, int32_t>::value || std::is_same<IndexT, int64_t>::value,
                "SparseRowAdamMixedGroup: ids must be int32_t or int64_t");
  using DevT = detail::DeviceElemT<ElemT>;
  SparseAdamOptions o = options;
  detail::CheckAdamOptions(o);
  CUEMBED_ASSERT(exp_avg_host != nullptr && exp_avg_device != nullptr && exp_avg_sq_device != nullptr);
  const bool both = o.rule == AdamRule::kAdam;
  CUEMBED_ASSERT(!both || exp_avg_sq_host != nullptr);
  const int bytes = detail::CheckMixedGroupStep<DevT>(
      o, reinterpret_cast<const void* const*>(tables_host), tables_device, widths_host, widths_device, num_tables,
      row_base_device, max_width, ids, rows, total_entries, exp_avg_host, both ? exp_avg_sq_host : nullptr);
  if (bytes == 0) return;
  const detail::MixedGroupTables g = {reinterpret_cast<const void* const*>(tables_device),
                                      const_cast<const float* const*>(exp_avg_device),
                                      const_cast<const float* const*>(exp_avg_sq_device), row_base_device, widths_device,
                                      num_tables};
  const detail::UpdateCounts counts = detail::CountsOf(o);
  const detail::AdamScalars h = {o.beta1, o.one_minus_beta1, o.beta2, o.one_minus_beta2, o.eps, o.weight_decay};
  const dim3 grid(detail::PlanMixedGroupUpdate(total_entries, detail::CurrentDeviceShape()));
  const dim3 block(detail::kUpdateBlockThreads);
  const size_t lds = detail::MixedGroupUpdateLdsBytes(num_tables, 2);
  detail::DispatchMixedLane<DevT>(bytes, [&](auto n) {
    detail::DispatchRule(o.rule, [&](auto rule) {
      constexpr int N = decltype(n)::value;
      constexpr AdamRule kRule = decltype(rule)::value;
      detail::SparseRowAdamMixedGroupKernel<DevT, IndexT, N, kRule, detail::kMixedPassesInFlight<kRule, N>>
          <<<grid, block, lds, stream>>>(ids, reinterpret_cast<const DevT*>(rows), g, max_width, total_entries, counts,
                                         o.lr, o.lr_device, o.bias_factor, o.bias_factor_device, h);
    });
  });
}

}  // namespace cuembed

#endif  // CUEMBED_INCLUDE_MIXED_GROUP_SPARSE_UPDATE_HPP_
