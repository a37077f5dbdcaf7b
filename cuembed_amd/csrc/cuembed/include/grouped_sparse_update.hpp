// MI355X (gfx950 / CDNA4) sparse optimizer step on a GROUP of separate table tensors, in one launch -- header-only host
// API (an extension: the reference ends at the gradient and takes one table).
//
//   cuembed::SparseRowUpdateGrouped<ElemT, IndexT>(tables_host, tables_device, state_host, state_device, num_tables,
//                                                  row_base_device, embed_width, ids, rows, total_entries, options, stream,
//                                                  seeds_device)
//   cuembed::SparseRowAdamGrouped<ElemT, IndexT>(tables_host, tables_device, exp_avg_host, exp_avg_device,
//                                                exp_avg_sq_host, exp_avg_sq_device, num_tables, row_base_device,
//                                                embed_width, ids, rows, total_entries, options, stream, seeds_device)
//
// consume the compressed gradient of a table group (grouped_backward.hpp: `ids` are GLOBAL rows of the tables laid end to
// end, ascending, `rows` their gradient rows) and update the named rows of T separate tensors and of their T (or 2 T) state
// tensors in place.  The kernel finds each entry's table itself (WalkNamedRows' kGrouped: a binary search over row_base,
// staged in LDS), so the step needs neither the per-table cuts nor T launches, and with the count on the device a whole
// training step on separate tensors can be captured into a HIP graph.
//
// As in EmbeddingForwardGrouped the caller builds the pointer arrays TWICE, once: in host memory, which the library reads
// to choose the access width (GroupAlignmentBits: the least aligned table -- or per-element state tensor -- narrows the
// lanes of the whole group), and in device memory, which the kernel reads.  Nothing is allocated, copied or read back and
// the host never waits; misuse CUEMBED_ASSERTs (prints and aborts) like every other entry point.
//
// Arithmetic, lane groups, entries in flight and launch shape are those of SparseRowUpdate / SparseRowAdam at the same
// lane width: the result has the bits of T single-table calls that run at that lane width.
//
// Stochastic rounding (16-bit tables): options.stochastic_rounding with seeds_device, ONE 64-bit SEED PER TABLE in device
// memory.  The bits of entry k are those of (seeds[t], step, r, column), t the table that owns ids[k] and r = ids[k] -
// row_base[t] its row inside that table; the step is options.rounding_step or the device word options.rounding_step_device,
// one value for the group, and options.rounding_seed is not read.  So the step has the bits of T single-table stochastic
// steps with seed = seeds[t] at the same step, and a table's trajectory depends neither on the group it is in nor on its
// place in it.  (This is NOT the naming of the single-table step on a one-storage group's flat tensor, which names the
// bits by the global row: the two draw different bits.)  There are no default seeds: stochastic_rounding without
// seeds_device, and seeds_device without stochastic_rounding, abort.  Tables behind the row cache are not taken.
#ifndef CUEMBED_INCLUDE_GROUPED_SPARSE_UPDATE_HPP_
#define CUEMBED_INCLUDE_GROUPED_SPARSE_UPDATE_HPP_

#include "cuembed/include/grouped_lookup.hpp"
#include "cuembed/include/sparse_adam.hpp"
#include "cuembed/include/sparse_update.hpp"

namespace cuembed {

namespace detail {

//! The checks both grouped steps share, and the options of the one piece they walk: (false: nothing to do).
inline bool CheckGroupedStep(SparseStepOptions& o, const void* tables_host, const void* tables_device,
                             const int num_tables, const int64_t* row_base_device, const void* ids, const void* rows,
                             const int64_t total_entries, const uint64_t* seeds_device) {
  CUEMBED_ASSERT(total_entries >= 0);
  CUEMBED_ASSERT(o.pieces == 1 && (o.piece_rows == 0 || o.piece_rows == total_entries));   // one piece: the whole array
  o.piece_rows = total_entries;
  CheckCountSource(o);
  CUEMBED_ASSERT(o.stochastic_rounding == (seeds_device != nullptr) &&
                 "stochastic rounding on a grouped step takes one seed per table, and seeds go with stochastic rounding");
  CUEMBED_ASSERT(num_tables >= 1 && num_tables <= kGroupedMaxTables);
  CUEMBED_ASSERT(tables_host != nullptr && tables_device != nullptr && row_base_device != nullptr);
  if (total_entries == 0 || o.num_rows == 0) return false;
  CUEMBED_ASSERT(ids != nullptr && rows != nullptr);
  return true;
}

//! A state tensor's bases OR-ed into one address (GroupAlignmentBits), or nullptr when the rule reads none per element.
inline const float* GroupStateBits(const float* const* state_host, const int num_tables, const bool per_element) {
  if (!per_element) return nullptr;
  CUEMBED_ASSERT(state_host != nullptr);
  return static_cast<const float*>(GroupAlignmentBits(reinterpret_cast<const void* const*>(state_host), num_tables));
}

//! The operands of a grouped step: the pointer arrays in device memory, and what the host copies say about alignment
//! (GroupAlignmentBits of the tables, GroupStateBits of the state tensors).
template <typename ElemT>
inline StepOperands GroupedOperands(const void* table_bits, ElemT* const* tables_device, const float* state_bits,
                                    float* const* state_device, const float* state2_bits, float* const* state2_device,
                                    const int num_tables, const int64_t* row_base_device, const uint64_t* seeds_device) {
  StepOperands p;
  p.table = table_bits, p.state = state_bits, p.state2 = state2_bits;
  p.grouped = {reinterpret_cast<const void* const*>(tables_device), const_cast<const float* const*>(state_device),
               const_cast<const float* const*>(state2_device), row_base_device, num_tables};
  p.seeds = seeds_device;
  return p;
}

}  // namespace detail

/**
 * @brief SparseRowUpdate on a group of `num_tables` separate tables of one element type and width, in one launch: for
 * every valid entry k, with t the table that owns the global row ids[k] (row_base[t] <= ids[k] < row_base[t + 1]) and
 * r = ids[k] - row_base[t], tables[t][r, :] and the state of row r of table t are updated in place from rows[k, :] by
 * options.rule.  Rows that no valid entry names are neither read nor written.
 *
 * @param tables_host      [num_tables] table base pointers, in HOST memory (read here, for the access width)
 * @param tables_device    the same pointers in DEVICE memory (read by the kernel)
 * @param state_host       [num_tables] bases of the state tensors in HOST memory: required for kAdagrad (its fp32
 *                         [rows_t, embed_width] state moves in the lanes of the weights), not read otherwise
 * @param state_device     the same pointers in DEVICE memory: nullptr for kSgd, fp32 [rows_t, embed_width] tensors for
 *                         kAdagrad, fp32 [rows_t] for kRowwiseAdagrad
 * @param num_tables       T, 1 <= T <= detail::kGroupedMaxTables
 * @param row_base_device  [num_tables + 1] int64 in DEVICE memory: the exclusive prefix sum of the tables' row counts
 * @param embed_width      elements per row of every table (row bytes a multiple of 4)
 * @param ids              [total_entries] global rows, valid entries distinct and inside [0, row_base[num_tables])
 * @param rows             [total_entries, embed_width] gradient rows, of the tables' type
 * @param total_entries    the entries `ids` and `rows` have room for
 * @param options          rule, lr, eps and ONE count source (num_rows, counts -- one word --, or last_id);
 *                         piece_rows may stay 0 (it is total_entries), pieces must be 1; a count below zero or above
 *                         total_entries applies nothing; stochastic_rounding (16-bit tables) requires seeds_device
 *                         and reads rounding_step / rounding_step_device, not rounding_seed
 * @param seeds_device     [num_tables] 64-bit seeds in DEVICE memory, one per table, with options.stochastic_rounding;
 *                         nullptr without it
 *
 * kRoundings: which roundings the instantiation carries kernels for (the C ABI splits them over two units).
 */
template <typename ElemT, typename IndexT, UpdateRoundings kRoundings = UpdateRoundings::kBoth>
void SparseRowUpdateGrouped(const ElemT* const* tables_host,
                            ElemT* const* tables_device,
                            const float* const* state_host,
                            float* const* state_device,
                            const int num_tables,
                            const int64_t* row_base_device,
                            const int embed_width,
                            const IndexT* ids,
                            const ElemT* rows,
                            const int64_t total_entries,
                            const SparseUpdateOptions& options,
                            const hipStream_t stream = 0,
                            const uint64_t* seeds_device = nullptr) {
  static_assert(std::is_same<ElemT, float>::value || std::is_same<ElemT, __half>::value ||
                    std::is_same<ElemT, __hip_bfloat16>::value,
                "SparseRowUpdateGrouped: tables must be float, __half or __hip_bfloat16");
  static_assert(std::is_same<IndexT, int32_t>::value || std::is_same<IndexT, int64_t>::value,
                "SparseRowUpdateGrouped: ids must be int32_t or int64_t");
  SparseUpdateOptions o = options;
  const bool work = detail::CheckGroupedStep(o, tables_host, tables_device, num_tables, row_base_device, ids, rows,
                                             total_entries, seeds_device);
  CUEMBED_ASSERT((o.rule == UpdateRule::kSgd) == (state_device == nullptr));
  CUEMBED_ASSERT(!o.stochastic_rounding || (detail::kCanRoundStochastically<ElemT, kRoundings>));
  CUEMBED_ASSERT(o.stochastic_rounding || kRoundings != UpdateRoundings::kStochasticOnly);
  if (!work) return;
  const void* table_bits = detail::GroupAlignmentBits(reinterpret_cast<const void* const*>(tables_host), num_tables);
  const float* state_bits = detail::GroupStateBits(state_host, num_tables, o.rule == UpdateRule::kAdagrad);
  const detail::StepOperands p = detail::GroupedOperands(table_bits, tables_device, state_bits, state_device, nullptr,
                                                         nullptr, num_tables, row_base_device, seeds_device);
  detail::LaunchSparseRowUpdate<detail::StepVariant::kGrouped, kRoundings>(p, embed_width, ids, rows, o, stream);
}

/**
 * @brief SparseRowAdam on a group of `num_tables` separate tables, in one launch: as SparseRowUpdateGrouped, with the two
 * moments of every table in tensors of their own.  options.bias_factor_device (AdamClockAdvance's word) serves the
 * whole group: one clock per group.
 *
 * @param exp_avg_host / exp_avg_device        [num_tables] bases of the fp32 [rows_t, embed_width] first moments, in
 *                                             HOST memory (read here, for the access width) and in DEVICE memory
 * @param exp_avg_sq_host / exp_avg_sq_device  the second moments: fp32 [rows_t, embed_width] (kAdam; both copies
 *                                             required) or fp32 [rows_t] (kRowwiseAdam; the host copy is not read)
 * Everything else, seeds_device and kRoundings included, as SparseRowUpdateGrouped; the hyper-parameters are checked as in
 * SparseRowAdam.
 */
template <typename ElemT, typename IndexT, UpdateRoundings kRoundings = UpdateRoundings::kBoth>
void SparseRowAdamGrouped(const ElemT* const* tables_host,
                          ElemT* const* tables_device,
                          const float* const* exp_avg_host,
                          float* const* exp_avg_device,
                          const float* const* exp_avg_sq_host,
                          float* const* exp_avg_sq_device,
                          const int num_tables,
                          const int64_t* row_base_device,
                          const int embed_width,
                          const IndexT* ids,
                          const ElemT* rows,
                          const int64_t total_entries,
                          const SparseAdamOptions& options,
                          const hipStream_t stream = 0,
                          const uint64_t* seeds_device = nullptr) {
  static_assert(std::is_same<ElemT, float>::value || std::is_same<ElemT, __half>::value ||
                    std::is_same<ElemT, __hip_bfloat16>::value,
                "SparseRowAdamGrouped: tables must be float, __half or __hip_bfloat16");
  static_assert(std::is_same<IndexT, int32_t>::value || std::is_same<IndexT, int64_t>::value,
                "SparseRowAdamGrouped: ids must be int32_t or int64_t");
  SparseAdamOptions o = options;
  const bool work = detail::CheckGroupedStep(o, tables_host, tables_device, num_tables, row_base_device, ids, rows,
                                             total_entries, seeds_device);
  CUEMBED_ASSERT(!o.stochastic_rounding || (detail::kCanRoundStochastically<ElemT, kRoundings>));
  CUEMBED_ASSERT(o.stochastic_rounding || kRoundings != UpdateRoundings::kStochasticOnly);
  detail::CheckAdamOptions(o);
  CUEMBED_ASSERT(exp_avg_device != nullptr && exp_avg_sq_device != nullptr);
  if (!work) return;
  const void* table_bits = detail::GroupAlignmentBits(reinterpret_cast<const void* const*>(tables_host), num_tables);
  const float* exp_avg_bits = detail::GroupStateBits(exp_avg_host, num_tables, true);
  const float* exp_avg_sq_bits = detail::GroupStateBits(exp_avg_sq_host, num_tables, o.rule == AdamRule::kAdam);
  const detail::StepOperands p =
      detail::GroupedOperands(table_bits, tables_device, exp_avg_bits, exp_avg_device, exp_avg_sq_bits, exp_avg_sq_device,
                              num_tables, row_base_device, seeds_device);
  detail::LaunchSparseRowAdam<detail::StepVariant::kGrouped, kRoundings>(p, embed_width, ids, rows, o, stream);
}

}  // namespace cuembed

#endif  // CUEMBED_INCLUDE_GROUPED_SPARSE_UPDATE_HPP_
