// MI355X (gfx950 / CDNA4) sparse optimizer step -- host API (an extension: the reference ends at the gradient).
//
//   cuembed::SparseRowUpdate<ElemT, IndexT>(table, state, embed_width, ids, rows, options, stream)
//   cuembed::SparseRowUpdate<ElemT, IndexT>(table, state, embed_width, ids, rows, options, stream, state_ids)
//   cuembed::SparseRowUpdate<ElemT, IndexT>(table, state, embed_width, ids, rows, options, stream, state_ids, row_names)
//
// consumes the compressed gradient that EmbeddingBackward (or the sparse-gradient exchange) produced -- `ids` naming
// table rows, `rows` their gradient rows -- and updates the named rows of `table` in place.  The number of valid
// entries may live on the device, so a step that ends in this call needs no host read-back.  With `state_ids` the state
// of entry k is addressed by a second id (a table behind the row cache keeps weights and state in two planes); with
// `row_names` the bits of stochastic rounding are named by a third, the table row, which a translated id is not.
#ifndef CUEMBED_INCLUDE_SPARSE_UPDATE_HPP_
#define CUEMBED_INCLUDE_SPARSE_UPDATE_HPP_

#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "cuembed/include/cuembed_assert.hpp"
#include "cuembed/include/device_shape.hpp"
#include "cuembed/include/sparse_update_kernels.hpp"

namespace cuembed {

//! What the options of every sparse step hold (SparseUpdateOptions below, SparseAdamOptions in sparse_adam.hpp): the
//! learning rate, the entries and the source of their count, and the rounding of the store.
struct SparseStepOptions {
  float lr = 0.f;                    //!< learning rate, unless ...
  const float* lr_device = nullptr;  //!< ... one fp32 word on the device holds it (a captured graph follows a schedule)
  //! The entries are `pieces` blocks of `piece_rows` entries; entry j of piece p is valid iff j < count(p).
  int64_t piece_rows = 0;            //!< capacity of one piece (rows of `ids` / `rows` per piece)
  int pieces = 1;
  //! Exactly one source of the counts:
  int64_t num_rows = -1;             //!< >= 0: host-known count (one piece)
  const void* counts = nullptr;      //!< counts[pieces] on the device, int32 or ...
  bool counts_are_int64 = false;     //!< ... int64
  const void* last_id = nullptr;     //!< one IndexT word on the device, count = *last_id + 1 (one piece): the
                                     //!< convention of EmbeddingBackward with num_grad_embedding_rows < 0
  //! Stochastic rounding of the one rounding to the table's type (__half / __hip_bfloat16 tables only; see
  //! stochastic_rounding.hpp).  The bits depend on (rounding_seed, step, table row, column) and on nothing else: give
  //! every call of a run the same seed and its own step.
  bool stochastic_rounding = false;
  uint64_t rounding_seed = 0;
  uint64_t rounding_step = 0;                    //!< the step, unless ...
  const int64_t* rounding_step_device = nullptr; //!< ... one int64 word on the device holds it (advance it on the
                                                 //!< device and a replayed graph draws fresh bits)
};

//! Rule, hyper-parameters and the source of the entry count of one SparseRowUpdate call.
struct SparseUpdateOptions : SparseStepOptions {
  UpdateRule rule = UpdateRule::kSgd;
  float eps = 1e-8f;                 //!< Adagrad rules: added to sqrt(state)
};

//! Which roundings a SparseRowUpdate instantiation carries kernels for.  The header API carries both; the C ABI splits
//! them over two translation units so that they compile side by side.
enum class UpdateRoundings { kBoth, kNearestOnly, kStochasticOnly };

namespace detail {

//! Bytes per lane: the widest of 16 / 8 / 4 that the row size, the three data pointers and the per-element state
//! (Adagrad's accumulator; Adam's first moment and, as `state2`, its second) allow.
template <typename ElemT>
inline int UpdateLaneBytes(const int embed_width, const void* table, const void* rows, const float* state,
                           const bool state_per_element, const float* state2 = nullptr) {
  const size_t row_bytes = static_cast<size_t>(embed_width) * sizeof(ElemT);
  CUEMBED_ASSERT(embed_width > 0);
  CUEMBED_ASSERT(row_bytes % 4 == 0);
  const uintptr_t bits = reinterpret_cast<uintptr_t>(table) | reinterpret_cast<uintptr_t>(rows) | row_bytes;
  CUEMBED_ASSERT(reinterpret_cast<uintptr_t>(table) % 4 == 0 && reinterpret_cast<uintptr_t>(rows) % 4 == 0);
  int bytes = bits % 16 == 0 ? 16 : (bits % 8 == 0 ? 8 : 4);
  if (state_per_element) {
    // a lane's N = bytes / sizeof(ElemT) state elements move as fp32 packs of min(N, 4)
    const auto state_align = [](int b) { const int n = b / static_cast<int>(sizeof(ElemT)); return 4 * (n < 4 ? n : 4); };
    const uintptr_t state_bits = reinterpret_cast<uintptr_t>(state) | reinterpret_cast<uintptr_t>(state2);
    while (bytes > 4 && state_bits % state_align(bytes) != 0) bytes /= 2;
    CUEMBED_ASSERT(state_bits % state_align(bytes) == 0);
  }
  return bytes;
}

//! Launch shape of one update: lanes per entry, slices per lane, grid (pure host arithmetic).
struct UpdateShape {
  int lanes_per_row;  //!< width / N
  int group;          //!< lanes per entry: a power of two <= 64
  int chunks;         //!< 1, kUpdateMaxChunks or 0 (run-time loop)
  unsigned grid;
};

inline UpdateShape PlanUpdate(const int lanes_per_row, const int64_t total_entries, const DeviceShape& dev) {
  UpdateShape s;
  s.lanes_per_row = lanes_per_row;
  s.group = 1;
  while (s.group < lanes_per_row && s.group < 64) s.group *= 2;
  s.chunks = lanes_per_row <= s.group ? 1 : (lanes_per_row <= kUpdateMaxChunks * s.group ? kUpdateMaxChunks : 0);
  const int groups_per_block = kUpdateBlockThreads / s.group;
  const int64_t needed = (total_entries + groups_per_block - 1) / groups_per_block;
  // as many workgroups as the device holds at once (8 per CU at 256 threads); the rest is the grid stride
  const int64_t resident = static_cast<int64_t>(dev.compute_units) * (dev.lanes_per_cu / kUpdateBlockThreads);
  s.grid = static_cast<unsigned>(needed < resident ? (needed < 1 ? 1 : needed) : resident);
  return s;
}

//! Whether an instantiation carries the stochastic kernels of its table type.
template <typename ElemT, UpdateRoundings kRoundings>
constexpr bool kCanRoundStochastically = !std::is_same<ElemT, float>::value && kRoundings != UpdateRoundings::kNearestOnly;

//! The checks that every sparse step makes, in this order: CheckCountSource, its own on the rule and the state, then
//! CheckRoundingAndWork on the rounding and the buffers (false: there is nothing to do).
inline void CheckCountSource(const SparseStepOptions& o) {
  const int sources = (o.num_rows >= 0) + (o.counts != nullptr) + (o.last_id != nullptr);
  CUEMBED_ASSERT(sources == 1);
  CUEMBED_ASSERT(o.pieces >= 1 && o.piece_rows >= 0);
  CUEMBED_ASSERT(o.pieces == 1 || o.counts != nullptr);   // several pieces: counts[pieces] on the device
  if (o.num_rows >= 0) CUEMBED_ASSERT(o.num_rows <= o.piece_rows);
}

template <typename ElemT, UpdateRoundings kRoundings>
inline bool CheckRoundingAndWork(const SparseStepOptions& o, const void* table, const void* ids, const void* rows) {
  CUEMBED_ASSERT(!o.stochastic_rounding || (kCanRoundStochastically<ElemT, kRoundings>));
  CUEMBED_ASSERT(o.stochastic_rounding || kRoundings != UpdateRoundings::kStochasticOnly);
  if (o.piece_rows == 0 || o.num_rows == 0) return false;
  CUEMBED_ASSERT(table != nullptr && ids != nullptr && rows != nullptr);
  return true;
}

inline UpdateCounts CountsOf(const SparseStepOptions& o) {
  UpdateCounts counts;
  counts.host_count = o.num_rows >= 0 ? o.num_rows : -1;
  counts.count_words = o.counts;
  counts.count_words_are_64 = o.counts_are_int64 ? 1 : 0;
  counts.last_id = o.last_id;
  return counts;
}

template <bool kStochastic>
inline UpdateRounding<kStochastic> RoundingOf(const SparseStepOptions& o) {
  UpdateRounding<kStochastic> rounding;
  if constexpr (kStochastic) {
    rounding.seed = o.rounding_seed;
    rounding.step = o.rounding_step;
    rounding.step_word = o.rounding_step_device;
  }
  return rounding;
}

template <int kValue>
using Int = std::integral_constant<int, kValue>;

//! From the options' rounding, the lane bytes and the plan to the instantiation: calls
//! launch(stochastic, n, chunks, shape) with the first three as integral constants -- stochastic rounding or not,
//! N = 16 / 8 / 4 bytes of ElemT per lane, slices per lane (1, kUpdateMaxChunks or 0) -- and the UpdateShape to launch.
template <typename ElemT, UpdateRoundings kRoundings, typename LaunchT>
inline void DispatchUpdate(const int bytes, const int width, const SparseStepOptions& o, const LaunchT& launch) {
  constexpr int kMaxN = 16 / static_cast<int>(sizeof(ElemT));
  const auto with_rounding = [&](auto stochastic) {
    const auto with_n = [&](auto n) {
      const UpdateShape s = PlanUpdate(width / n, o.piece_rows * o.pieces, CurrentDeviceShape());
      if (s.chunks == 1) launch(stochastic, n, Int<1>(), s);
      else if (s.chunks == kUpdateMaxChunks) launch(stochastic, n, Int<kUpdateMaxChunks>(), s);
      else launch(stochastic, n, Int<0>(), s);
    };
    if (bytes == 16) with_n(Int<kMaxN>());
    else if (bytes == 8) with_n(Int<kMaxN / 2>());
    else with_n(Int<kMaxN / 4>());
  };
  if constexpr (kCanRoundStochastically<ElemT, kRoundings>) {
    if (o.stochastic_rounding) return with_rounding(std::true_type());
  }
  if constexpr (kRoundings != UpdateRoundings::kStochasticOnly) with_rounding(std::false_type());
}

//! The variants of a step, by what the caller supplied beyond ids and rows: nothing; ids of their own for the state
//! tensors (round to nearest); those and the table rows that name the bits of stochastic rounding; or a group of
//! separate tables (grouped_sparse_update.hpp), whose stochastic kernels are a fifth variant with a seed per table.
enum class StepVariant { kPlain, kPlaced, kNamed, kGrouped };

//! What the kernels of a step read and write besides ids and rows; a variant reads its own fields.
struct StepOperands {
  //! The tensors of a single-table step (state2: Adam's second moment).  Of a grouped step, what decides the lane bytes
  //! alone: the bases of each tensor list OR-ed into one address (GroupAlignmentBits), nullptr where no state moves in
  //! the lanes of the weights.
  const void* table = nullptr;
  const float* state = nullptr;
  const float* state2 = nullptr;
  const int64_t* state_ids = nullptr;    //!< kPlaced, kNamed: where entry k keeps its state ...
  const int64_t* state2_ids = nullptr;   //!< ... and Adam's second moment
  const int64_t* row_names = nullptr;    //!< kNamed: the table row of entry k
  GroupedTables<true> grouped = {};      //!< kGrouped: the pointer arrays in device memory ...
  const uint64_t* seeds = nullptr;       //!< ... and, with stochastic rounding, a seed per table
};

//! Entries in flight per lane group (WalkNamedRows' kEntries) of the kernel that a variant launches for (rounding, rule,
//! N, kChunks): two when a lane holds one slice per entry, else one.  Every variant takes what its plain sibling takes:
//! the placed Adam kernels, the named ones (profiles/sparse_update_placed_stochastic_kernel_resources.txt) and the
//! grouped ones, of which no instantiation spills with two (profiles/sparse_update_grouped_kernel_resources.txt,
//! profiles/sparse_update_grouped_stochastic_kernel_resources.txt).  A specialisation on (variant, rounding, rule, N) is
//! where a fallback to one would go.  (SparseRowUpdateKernel and its placed and named siblings take no such parameter:
//! they hold the same answer themselves.)
template <StepVariant kVariant, bool kStochastic, auto kRule, int N, int kChunks>
constexpr int kStepEntriesInFlight = kChunks == 1 ? 2 : 1;

//! From options.rule to the instantiation: calls with_rule(rule) with the rule as an integral constant.
template <typename WithRuleT>
inline void DispatchRule(const UpdateRule rule, const WithRuleT& with_rule) {
  switch (rule) {
    case UpdateRule::kSgd: return with_rule(std::integral_constant<UpdateRule, UpdateRule::kSgd>());
    case UpdateRule::kAdagrad: return with_rule(std::integral_constant<UpdateRule, UpdateRule::kAdagrad>());
    case UpdateRule::kRowwiseAdagrad: return with_rule(std::integral_constant<UpdateRule, UpdateRule::kRowwiseAdagrad>());
  }
  CUEMBED_ASSERT(false && "unknown update rule");
}

//! The one launch path of SGD / Adagrad / row-wise Adagrad, for every variant: lane bytes, counts, dispatch on rounding,
//! lane width, slices and rule, and the launch.  The entry points below have made their checks; kRoundings is what the
//! variant may launch of what its caller carries.
template <StepVariant kVariant, UpdateRoundings kRoundings, typename ElemT, typename IndexT>
void LaunchSparseRowUpdate(const StepOperands& p, const int embed_width, const IndexT* ids, const ElemT* rows,
                           const SparseUpdateOptions& o, const hipStream_t stream) {
  using DevT = DeviceElemT<ElemT>;
  const int bytes = UpdateLaneBytes<DevT>(embed_width, p.table, rows, p.state, o.rule == UpdateRule::kAdagrad);
  const UpdateCounts counts = CountsOf(o);
  DevT* t = reinterpret_cast<DevT*>(const_cast<void*>(p.table));
  float* state = const_cast<float*>(p.state);
  const DevT* g = reinterpret_cast<const DevT*>(rows);
  DispatchUpdate<DevT, kRoundings>(bytes, embed_width, o, [&](auto stochastic, auto n, auto chunks, const UpdateShape& s) {
    DispatchRule(o.rule, [&](auto rule) {
      constexpr bool kStochastic = decltype(stochastic)::value;
      constexpr int N = decltype(n)::value, kChunks = decltype(chunks)::value;
      constexpr UpdateRule kRule = decltype(rule)::value;
      const dim3 grid(s.grid), block(kUpdateBlockThreads);
      if constexpr (kVariant == StepVariant::kPlain) {
        SparseRowUpdateKernel<DevT, IndexT, N, kRule, kChunks, kStochastic><<<grid, block, 0, stream>>>(
            ids, g, t, state, embed_width, s.lanes_per_row, s.group, o.piece_rows, o.pieces, counts, o.lr, o.lr_device,
            o.eps, RoundingOf<kStochastic>(o));
      } else if constexpr (kVariant == StepVariant::kPlaced) {
        if constexpr (kRule != UpdateRule::kSgd) {   // (SGD has no state to place: its entry point refuses it)
          SparseRowUpdatePlacedKernel<DevT, IndexT, N, kRule, kChunks><<<grid, block, 0, stream>>>(
              ids, p.state_ids, g, t, state, embed_width, s.lanes_per_row, s.group, o.piece_rows, o.pieces, counts, o.lr,
              o.lr_device, o.eps);
        }
      } else if constexpr (kVariant == StepVariant::kNamed) {
        SparseRowUpdateNamedKernel<DevT, IndexT, N, kRule, kChunks><<<grid, block, 0, stream>>>(
            ids, p.state_ids, p.row_names, g, t, state, embed_width, s.lanes_per_row, s.group, o.piece_rows, o.pieces,
            counts, o.lr, o.lr_device, o.eps, RoundingOf<true>(o));
      } else {
        constexpr int kInFlight = kStepEntriesInFlight<kVariant, kStochastic, kRule, N, kChunks>;
        const size_t lds = sizeof(int64_t) * GroupedLdsWords(p.grouped.num_tables, kRule == UpdateRule::kSgd ? 0 : 1, kStochastic);
        if constexpr (kStochastic) {
          SparseRowUpdateGroupedStochasticKernel<DevT, IndexT, N, kRule, kChunks, kInFlight><<<grid, block, lds, stream>>>(
              ids, g, GroupedSeededTables{p.grouped, p.seeds}, embed_width, s.lanes_per_row, s.group, o.piece_rows,
              o.pieces, counts, o.lr, o.lr_device, o.eps, RoundingOf<true>(o));
        } else {
          SparseRowUpdateGroupedKernel<DevT, IndexT, N, kRule, kChunks, kInFlight><<<grid, block, lds, stream>>>(
              ids, g, p.grouped, embed_width, s.lanes_per_row, s.group, o.piece_rows, o.pieces, counts, o.lr, o.lr_device,
              o.eps);
        }
      }
    });
  });
}

}  // namespace detail

/**
 * @brief Sparse optimizer step: for every valid entry k, table[ids[k], :] and the state of row ids[k] are updated in
 * place from rows[k, :] by options.rule.  Rows that no valid entry names are neither read nor written.
 *
 * All arithmetic is fp32 whatever ElemT is, with exactly one rounding to ElemT at the store: to nearest, or, with
 * options.stochastic_rounding on a __half / __hip_bfloat16 table, up or down with the probability of the value's
 * position between its two neighbours (stochastic_rounding.hpp).  The fp32 arithmetic and the fp32 state are the same
 * either way.
 *
 * The valid entries must name DISTINCT rows, i.e. the gradient must be coalesced: the output of EmbeddingBackward on a
 * fully sorted transpose or on ComputeCompressedGradIndicesBlocked's ids, or a piece of the sparse-gradient exchange.
 * The UNCOALESCED gradient of a sample-blocked transpose (one entry per (block, row)) is not accepted: Adagrad is not
 * linear and two entries on one row would race.  Entries at or past the count are ignored whatever they hold, which
 * is what makes padded buffers safe; a count above piece_rows (the backward then wrote nothing and raised its
 * overflow word) or below zero leaves the table unchanged.
 *
 * @param table  [num_categories, embed_width], updated in place
 * @param state  nullptr (kSgd), fp32 [num_categories, embed_width] (kAdagrad) or fp32 [num_categories]
 *               (kRowwiseAdagrad), updated in place
 * @param ids    [pieces * piece_rows] table rows (values in [0, num_categories) wherever valid)
 * @param rows   [pieces * piece_rows, embed_width] gradient rows, of the table's type
 *
 * Misuse (no or more than one count source, a missing state, a row size that is not a multiple of 4 bytes, stochastic
 * rounding on a float table or in an instantiation without those kernels) aborts with the failed condition, like
 * EmbeddingBackward.
 */
template <typename ElemT, typename IndexT, UpdateRoundings kRoundings = UpdateRoundings::kBoth>
void SparseRowUpdate(ElemT* table,
                     float* state,
                     const int embed_width,
                     const IndexT* ids,
                     const ElemT* rows,
                     const SparseUpdateOptions& options,
                     const hipStream_t stream = 0) {
  static_assert(std::is_same<ElemT, float>::value || std::is_same<ElemT, __half>::value ||
                    std::is_same<ElemT, __hip_bfloat16>::value,
                "SparseRowUpdate: tables must be float, __half or __hip_bfloat16");
  static_assert(std::is_same<IndexT, int32_t>::value || std::is_same<IndexT, int64_t>::value,
                "SparseRowUpdate: ids must be int32_t or int64_t");
  detail::CheckCountSource(options);
  CUEMBED_ASSERT((options.rule == UpdateRule::kSgd) == (state == nullptr));
  if (!detail::CheckRoundingAndWork<ElemT, kRoundings>(options, table, ids, rows)) return;
  detail::StepOperands p;
  p.table = table, p.state = state;
  detail::LaunchSparseRowUpdate<detail::StepVariant::kPlain, kRoundings>(p, embed_width, ids, rows, options, stream);
}

/**
 * @brief The same step with the state in a place of its own: entry k updates table[ids[k], :] as above, but reads and
 * writes its state at row state_ids[k] of `state` -- the per-element accumulator at state[state_ids[k], :] (kAdagrad),
 * the row word at state[state_ids[k]] (kRowwiseAdagrad).  For a table behind the row cache (row_cache.hpp), whose
 * weights and state are cached in two planes: `ids` are the batch's ids translated with the table plane's row offset,
 * `state_ids` the same ids translated with the state plane's, and both reach cached rows through the base pointers of
 * the host tensors.  Same walk, same launch shape, same arithmetic and the same bits as the call above on tensors that
 * hold the same values.  The valid entries must name distinct rows in both id arrays.
 *
 * state_ids == nullptr is the call above.  Otherwise the rule must have a state (not kSgd) and the rounding is to
 * nearest: the bits of stochastic rounding are named by the table row, which a translated id is not -- the overload
 * with `row_names` below carries the table rows next to the placed ids and rounds stochastically.
 */
template <typename ElemT, typename IndexT, UpdateRoundings kRoundings = UpdateRoundings::kBoth>
void SparseRowUpdate(ElemT* table,
                     float* state,
                     const int embed_width,
                     const IndexT* ids,
                     const ElemT* rows,
                     const SparseUpdateOptions& options,
                     const hipStream_t stream,
                     const int64_t* state_ids) {
  if (state_ids == nullptr)
    return SparseRowUpdate<ElemT, IndexT, kRoundings>(table, state, embed_width, ids, rows, options, stream);
  static_assert(kRoundings != UpdateRoundings::kStochasticOnly, "a placed state is updated with round to nearest");
  detail::CheckCountSource(options);
  CUEMBED_ASSERT(options.rule != UpdateRule::kSgd && state != nullptr);
  CUEMBED_ASSERT(!options.stochastic_rounding);
  if (!detail::CheckRoundingAndWork<ElemT, UpdateRoundings::kNearestOnly>(options, table, ids, rows)) return;
  detail::StepOperands p;
  p.table = table, p.state = state, p.state_ids = state_ids;
  detail::LaunchSparseRowUpdate<detail::StepVariant::kPlaced, UpdateRoundings::kNearestOnly>(p, embed_width, ids, rows,
                                                                                              options, stream);
}

namespace detail {
//! The named step itself (row_names != nullptr): the body of the overload below, and what a translation unit that wants
//! the named kernels alone calls.
template <typename ElemT, typename IndexT, UpdateRoundings kRoundings>
void SparseRowUpdateNamed(ElemT* table, float* state, const int embed_width, const IndexT* ids, const ElemT* rows,
                          const SparseUpdateOptions& options, const hipStream_t stream, const int64_t* state_ids,
                          const int64_t* row_names) {
  CUEMBED_ASSERT(row_names != nullptr);
  CheckCountSource(options);
  CUEMBED_ASSERT(options.stochastic_rounding);
  CUEMBED_ASSERT(sizeof(ElemT) == 2);
  if (options.rule == UpdateRule::kSgd) CUEMBED_ASSERT(state == nullptr && state_ids == nullptr);
  else CUEMBED_ASSERT(state != nullptr && state_ids != nullptr);
  if (!CheckRoundingAndWork<ElemT, kRoundings>(options, table, ids, rows)) return;
  if constexpr (kCanRoundStochastically<ElemT, kRoundings>) {
    StepOperands p;
    p.table = table, p.state = state, p.state_ids = state_ids, p.row_names = row_names;
    LaunchSparseRowUpdate<StepVariant::kNamed, UpdateRoundings::kStochasticOnly>(p, embed_width, ids, rows, options, stream);
  }
}
}  // namespace detail

/**
 * @brief The placed step with stochastic rounding: entry k updates table[ids[k], :] and its state at row state_ids[k]
 * as above, and the one rounding to ElemT draws the bits of (seed, step, row_names[k], column).  For a table behind the
 * row cache: `ids` and `state_ids` are translated and name slots, `row_names` are the batch's own ids -- the table rows
 * -- so that a row rounds with the same bits wherever the cache has put it, and the result is bit for bit that of the
 * unplaced stochastic call on tensors that hold the same values.  Lane bytes, plan and dispatch are that call's.
 *
 * row_names == nullptr is the call above (which refuses stochastic rounding with placed ids).  With names,
 * options.stochastic_rounding must be set and ElemT must be a 16-bit type; kSgd takes state == nullptr and
 * state_ids == nullptr (the table plane only), every other rule requires state_ids.  The valid entries must name
 * distinct rows in every id array.  Misuse aborts with the failed condition.
 */
template <typename ElemT, typename IndexT, UpdateRoundings kRoundings = UpdateRoundings::kBoth>
void SparseRowUpdate(ElemT* table,
                     float* state,
                     const int embed_width,
                     const IndexT* ids,
                     const ElemT* rows,
                     const SparseUpdateOptions& options,
                     const hipStream_t stream,
                     const int64_t* state_ids,
                     const int64_t* row_names) {
  if (row_names == nullptr) {
    if constexpr (kRoundings == UpdateRoundings::kStochasticOnly) {
      CUEMBED_ASSERT(state_ids == nullptr);   // (placed ids without names: round to nearest, not in this instantiation)
      return SparseRowUpdate<ElemT, IndexT, kRoundings>(table, state, embed_width, ids, rows, options, stream);
    } else {
      return SparseRowUpdate<ElemT, IndexT, kRoundings>(table, state, embed_width, ids, rows, options, stream, state_ids);
    }
  }
  detail::SparseRowUpdateNamed<ElemT, IndexT, kRoundings>(table, state, embed_width, ids, rows, options, stream, state_ids,
                                                          row_names);
}

}  // namespace cuembed

#endif  // CUEMBED_INCLUDE_SPARSE_UPDATE_HPP_
