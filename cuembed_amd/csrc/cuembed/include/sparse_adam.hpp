// MI355X (gfx950 / CDNA4) sparse optimizer step, the Adam family -- host API (an extension: the reference ends at the
// gradient).
//
//   cuembed::SparseRowAdam<ElemT, IndexT>(table, exp_avg, exp_avg_sq, embed_width, ids, rows, options, stream)
//   cuembed::SparseRowAdam<ElemT, IndexT>(table, exp_avg, exp_avg_sq, embed_width, ids, rows, options, stream,
//                                         exp_avg_ids, exp_avg_sq_ids)
//   cuembed::SparseRowAdam<ElemT, IndexT>(table, exp_avg, exp_avg_sq, embed_width, ids, rows, options, stream,
//                                         exp_avg_ids, exp_avg_sq_ids, row_names)
//   cuembed::AdamClockAdvance(powers, bias_factor, beta1, beta2, stream)
//
// SparseRowAdam consumes the compressed gradient like SparseRowUpdate (sparse_update.hpp) and keeps two fp32 moments per
// named row; with exp_avg_ids / exp_avg_sq_ids the moments of entry k are addressed by ids of their own (a table behind
// the row cache keeps weights and moments in three planes), and with row_names the bits of stochastic rounding are named
// by the table rows that the translated ids no longer are; AdamClockAdvance keeps the bias factor of the step in a device word, so that a captured step needs the host
// for neither the entry count nor the step number.
#ifndef CUEMBED_INCLUDE_SPARSE_ADAM_HPP_
#define CUEMBED_INCLUDE_SPARSE_ADAM_HPP_

#include "cuembed/include/sparse_adam_kernels.hpp"
#include "cuembed/include/sparse_update.hpp"

namespace cuembed {

//! Rule, hyper-parameters and (SparseStepOptions) learning rate, entries, count source and rounding of one SparseRowAdam call.
struct SparseAdamOptions : SparseStepOptions {
  AdamRule rule = AdamRule::kAdam;
  float bias_factor = 1.f;                    //!< c = sqrt(1 - beta2^t) / (1 - beta1^t) of step t (1: no correction), unless ...
  const float* bias_factor_device = nullptr;  //!< ... one fp32 word on the device holds it (AdamClockAdvance writes it)
  //! The kernel multiplies with these fp32 values as they are: form 1 - beta in double and round it once.
  float beta1 = 0.9f, one_minus_beta1 = 0.1f;
  float beta2 = 0.999f, one_minus_beta2 = 0.001f;
  float eps = 1e-8f;                          //!< added to sqrt(v)
  float weight_decay = 0.f;                   //!< decoupled (AdamW): w <- w - (lr * weight_decay) * w on the named rows; 0: off
};

namespace detail {

//! The checks of the hyper-parameters, and of the moments of a single-table step that has work.
inline void CheckAdamOptions(const SparseAdamOptions& options) {
  CUEMBED_ASSERT(options.beta1 >= 0.f && options.beta1 < 1.f && options.beta2 >= 0.f && options.beta2 < 1.f);
  CUEMBED_ASSERT(options.eps >= 0.f && options.weight_decay >= 0.f);
}

inline void CheckMoments(const float* exp_avg, const float* exp_avg_sq) {
  CUEMBED_ASSERT(exp_avg != nullptr && exp_avg_sq != nullptr);
  CUEMBED_ASSERT(reinterpret_cast<uintptr_t>(exp_avg_sq) % 4 == 0);
}

//! From options.rule to the instantiation: calls with_rule(rule) with the rule as an integral constant.
template <typename WithRuleT>
inline void DispatchRule(const AdamRule rule, const WithRuleT& with_rule) {
  switch (rule) {
    case AdamRule::kAdam: return with_rule(std::integral_constant<AdamRule, AdamRule::kAdam>());
    case AdamRule::kRowwiseAdam: return with_rule(std::integral_constant<AdamRule, AdamRule::kRowwiseAdam>());
  }
  CUEMBED_ASSERT(false && "unknown Adam rule");
}

//! The one launch path of Adam / row-wise Adam, for every variant (as LaunchSparseRowUpdate; p.state = exp_avg,
//! p.state2 = exp_avg_sq): lane bytes, counts, scalars, dispatch and the launch.
template <StepVariant kVariant, UpdateRoundings kRoundings, typename ElemT, typename IndexT>
void LaunchSparseRowAdam(const StepOperands& p, const int embed_width, const IndexT* ids, const ElemT* rows,
                         const SparseAdamOptions& o, const hipStream_t stream) {
  using DevT = DeviceElemT<ElemT>;
  const int bytes = UpdateLaneBytes<DevT>(embed_width, p.table, rows, p.state, true,
                                          o.rule == AdamRule::kAdam ? p.state2 : nullptr);
  const UpdateCounts counts = CountsOf(o);
  const AdamScalars h = {o.beta1, o.one_minus_beta1, o.beta2, o.one_minus_beta2, o.eps, o.weight_decay};
  DevT* t = reinterpret_cast<DevT*>(const_cast<void*>(p.table));
  float* m = const_cast<float*>(p.state);
  float* v = const_cast<float*>(p.state2);
  const DevT* g = reinterpret_cast<const DevT*>(rows);
  DispatchUpdate<DevT, kRoundings>(bytes, embed_width, o, [&](auto stochastic, auto n, auto chunks, const UpdateShape& s) {
    DispatchRule(o.rule, [&](auto rule) {
      constexpr bool kStochastic = decltype(stochastic)::value;
      constexpr int N = decltype(n)::value, kChunks = decltype(chunks)::value;
      constexpr AdamRule kRule = decltype(rule)::value;
      constexpr int kInFlight = kStepEntriesInFlight<kVariant, kStochastic, kRule, N, kChunks>;
      const dim3 grid(s.grid), block(kUpdateBlockThreads);
      if constexpr (kVariant == StepVariant::kPlain) {
        SparseRowAdamKernel<DevT, IndexT, N, kRule, kChunks, kInFlight, kStochastic><<<grid, block, 0, stream>>>(
            ids, g, t, m, v, embed_width, s.lanes_per_row, s.group, o.piece_rows, o.pieces, counts, o.lr, o.lr_device,
            o.bias_factor, o.bias_factor_device, h, RoundingOf<kStochastic>(o));
      } else if constexpr (kVariant == StepVariant::kPlaced) {
        SparseRowAdamPlacedKernel<DevT, IndexT, N, kRule, kChunks, kInFlight><<<grid, block, 0, stream>>>(
            ids, p.state_ids, p.state2_ids, g, t, m, v, embed_width, s.lanes_per_row, s.group, o.piece_rows, o.pieces,
            counts, o.lr, o.lr_device, o.bias_factor, o.bias_factor_device, h);
      } else if constexpr (kVariant == StepVariant::kNamed) {
        SparseRowAdamNamedKernel<DevT, IndexT, N, kRule, kChunks, kInFlight><<<grid, block, 0, stream>>>(
            ids, p.state_ids, p.state2_ids, p.row_names, g, t, m, v, embed_width, s.lanes_per_row, s.group, o.piece_rows,
            o.pieces, counts, o.lr, o.lr_device, o.bias_factor, o.bias_factor_device, h, RoundingOf<true>(o));
      } else {
        const size_t lds = sizeof(int64_t) * GroupedLdsWords(p.grouped.num_tables, 2, kStochastic);
        if constexpr (kStochastic) {
          SparseRowAdamGroupedStochasticKernel<DevT, IndexT, N, kRule, kChunks, kInFlight><<<grid, block, lds, stream>>>(
              ids, g, GroupedSeededTables{p.grouped, p.seeds}, embed_width, s.lanes_per_row, s.group, o.piece_rows,
              o.pieces, counts, o.lr, o.lr_device, o.bias_factor, o.bias_factor_device, h, RoundingOf<true>(o));
        } else {
          SparseRowAdamGroupedKernel<DevT, IndexT, N, kRule, kChunks, kInFlight><<<grid, block, lds, stream>>>(
              ids, g, p.grouped, embed_width, s.lanes_per_row, s.group, o.piece_rows, o.pieces, counts, o.lr, o.lr_device,
              o.bias_factor, o.bias_factor_device, h);
        }
      }
    });
  });
}

}  // namespace detail

/**
 * @brief Sparse Adam step: for every valid entry k, table[ids[k], :] and the moments of row ids[k] are updated in place
 * from rows[k, :] by options.rule (AdamRule).  Rows that no valid entry names are neither read nor written: their
 * moments do not decay (torch.optim.SparseAdam's behaviour).
 *
 * All arithmetic is fp32 whatever ElemT is, one unfused operation per step, with exactly one rounding to ElemT at the
 * store (to nearest, or stochastically: see SparseRowUpdate).  The bias correction goes into the step size, lr * c with
 * c = options.bias_factor (or the device word), and eps is added to sqrt(v): torch.optim.SparseAdam's formula.
 *
 * The valid entries must name DISTINCT rows (a coalesced gradient); entries at or past the count are ignored whatever
 * they hold; a count above piece_rows or below zero leaves the table and the moments unchanged.
 *
 * @param table       [num_categories, embed_width], updated in place
 * @param exp_avg     fp32 [num_categories, embed_width], updated in place
 * @param exp_avg_sq  fp32 [num_categories, embed_width] (kAdam) or fp32 [num_categories] (kRowwiseAdam), updated in place
 * @param ids         [pieces * piece_rows] table rows (values in [0, num_categories) wherever valid)
 * @param rows        [pieces * piece_rows, embed_width] gradient rows, of the table's type
 *
 * Misuse (no or more than one count source, a missing moment, betas outside [0, 1), a negative eps or weight decay, a
 * row size that is not a multiple of 4 bytes, stochastic rounding on a float table or in an instantiation without
 * those kernels) aborts with the failed condition, like SparseRowUpdate.
 */
template <typename ElemT, typename IndexT, UpdateRoundings kRoundings = UpdateRoundings::kBoth>
void SparseRowAdam(ElemT* table,
                   float* exp_avg,
                   float* exp_avg_sq,
                   const int embed_width,
                   const IndexT* ids,
                   const ElemT* rows,
                   const SparseAdamOptions& options,
                   const hipStream_t stream = 0) {
  static_assert(std::is_same<ElemT, float>::value || std::is_same<ElemT, __half>::value ||
                    std::is_same<ElemT, __hip_bfloat16>::value,
                "SparseRowAdam: tables must be float, __half or __hip_bfloat16");
  static_assert(std::is_same<IndexT, int32_t>::value || std::is_same<IndexT, int64_t>::value,
                "SparseRowAdam: ids must be int32_t or int64_t");
  detail::CheckCountSource(options);
  detail::CheckAdamOptions(options);
  if (!detail::CheckRoundingAndWork<ElemT, kRoundings>(options, table, ids, rows)) return;
  detail::CheckMoments(exp_avg, exp_avg_sq);
  detail::StepOperands p;
  p.table = table, p.state = exp_avg, p.state2 = exp_avg_sq;
  detail::LaunchSparseRowAdam<detail::StepVariant::kPlain, kRoundings>(p, embed_width, ids, rows, options, stream);
}

/**
 * @brief The same step with the moments in places of their own: entry k updates table[ids[k], :] as above, but reads
 * and writes its first moment at row exp_avg_ids[k] of `exp_avg` and its second at row exp_avg_sq_ids[k] of `exp_avg_sq`
 * (kAdam: a row of embed_width elements; kRowwiseAdam: the row's one word).  For a table behind the row cache
 * (row_cache.hpp) whose weights and moments are cached in three planes: `ids`, `exp_avg_ids` and `exp_avg_sq_ids` are the
 * batch's ids translated with the three planes' row offsets (TranslateIndicesForRowCachePlanes), and each reaches cached
 * rows through the base pointer of its host tensor.  The two moments need an id each: they are separate allocations,
 * so their planes' row offsets differ, and row-wise their row sizes do.  Lane bytes, launch shape and dispatch are those
 * of the call above: the same walk, the same arithmetic and the same bits on tensors that hold the same values.  The
 * valid entries must name distinct rows in all three id arrays.
 *
 * Both id arrays nullptr is the call above.  Otherwise both are required and the rounding is to nearest (the bits of
 * stochastic rounding are named by the table row, which a translated id is not: the overload with `row_names` below
 * carries the table rows and rounds stochastically); one array alone, or stochastic rounding, aborts with the failed
 * condition.
 */
template <typename ElemT, typename IndexT, UpdateRoundings kRoundings = UpdateRoundings::kBoth>
void SparseRowAdam(ElemT* table,
                   float* exp_avg,
                   float* exp_avg_sq,
                   const int embed_width,
                   const IndexT* ids,
                   const ElemT* rows,
                   const SparseAdamOptions& options,
                   const hipStream_t stream,
                   const int64_t* exp_avg_ids,
                   const int64_t* exp_avg_sq_ids) {
  if (exp_avg_ids == nullptr && exp_avg_sq_ids == nullptr)
    return SparseRowAdam<ElemT, IndexT, kRoundings>(table, exp_avg, exp_avg_sq, embed_width, ids, rows, options, stream);
  static_assert(kRoundings != UpdateRoundings::kStochasticOnly, "placed moments are updated with round to nearest");
  detail::CheckCountSource(options);
  detail::CheckAdamOptions(options);
  CUEMBED_ASSERT(exp_avg_ids != nullptr && exp_avg_sq_ids != nullptr);
  CUEMBED_ASSERT(!options.stochastic_rounding);
  if (!detail::CheckRoundingAndWork<ElemT, UpdateRoundings::kNearestOnly>(options, table, ids, rows)) return;
  detail::CheckMoments(exp_avg, exp_avg_sq);
  detail::StepOperands p;
  p.table = table, p.state = exp_avg, p.state2 = exp_avg_sq, p.state_ids = exp_avg_ids, p.state2_ids = exp_avg_sq_ids;
  detail::LaunchSparseRowAdam<detail::StepVariant::kPlaced, UpdateRoundings::kNearestOnly>(p, embed_width, ids, rows,
                                                                                            options, stream);
}

namespace detail {
//! The named step itself (row_names != nullptr): the body of the overload below, and what a translation unit that wants
//! the named kernels alone calls.
template <typename ElemT, typename IndexT, UpdateRoundings kRoundings>
void SparseRowAdamNamed(ElemT* table, float* exp_avg, float* exp_avg_sq, const int embed_width, const IndexT* ids,
                        const ElemT* rows, const SparseAdamOptions& options, const hipStream_t stream,
                        const int64_t* exp_avg_ids, const int64_t* exp_avg_sq_ids, const int64_t* row_names) {
  CUEMBED_ASSERT(row_names != nullptr);
  CheckCountSource(options);
  CheckAdamOptions(options);
  CUEMBED_ASSERT(exp_avg_ids != nullptr && exp_avg_sq_ids != nullptr);
  CUEMBED_ASSERT(options.stochastic_rounding);
  CUEMBED_ASSERT(sizeof(ElemT) == 2);
  if (!CheckRoundingAndWork<ElemT, kRoundings>(options, table, ids, rows)) return;
  CheckMoments(exp_avg, exp_avg_sq);
  if constexpr (kCanRoundStochastically<ElemT, kRoundings>) {
    StepOperands p;
    p.table = table, p.state = exp_avg, p.state2 = exp_avg_sq, p.state_ids = exp_avg_ids, p.state2_ids = exp_avg_sq_ids;
    p.row_names = row_names;
    LaunchSparseRowAdam<StepVariant::kNamed, UpdateRoundings::kStochasticOnly>(p, embed_width, ids, rows, options, stream);
  }
}
}  // namespace detail

/**
 * @brief The placed step with stochastic rounding: entry k updates table[ids[k], :] and its moments at rows
 * exp_avg_ids[k] / exp_avg_sq_ids[k] as above, and the one rounding to ElemT draws the bits of (seed, step,
 * row_names[k], column).  For a table behind the row cache: the three id arrays are translated and name slots,
 * `row_names` are the batch's own ids -- the table rows -- so that a row rounds with the same bits wherever the cache
 * has put it, and the result is bit for bit that of the unplaced stochastic call on tensors that hold the same values.
 * Lane bytes, plan and dispatch are that call's.
 *
 * row_names == nullptr is the call above (which refuses stochastic rounding with placed ids).  With names,
 * options.stochastic_rounding must be set, ElemT must be a 16-bit type and both moment id arrays are required.  The
 * valid entries must name distinct rows in every id array.  Misuse aborts with the failed condition.
 */
template <typename ElemT, typename IndexT, UpdateRoundings kRoundings = UpdateRoundings::kBoth>
void SparseRowAdam(ElemT* table,
                   float* exp_avg,
                   float* exp_avg_sq,
                   const int embed_width,
                   const IndexT* ids,
                   const ElemT* rows,
                   const SparseAdamOptions& options,
                   const hipStream_t stream,
                   const int64_t* exp_avg_ids,
                   const int64_t* exp_avg_sq_ids,
                   const int64_t* row_names) {
  if (row_names == nullptr) {
    if constexpr (kRoundings == UpdateRoundings::kStochasticOnly) {
      // (placed ids without names: round to nearest, not in this instantiation)
      CUEMBED_ASSERT(exp_avg_ids == nullptr && exp_avg_sq_ids == nullptr);
      return SparseRowAdam<ElemT, IndexT, kRoundings>(table, exp_avg, exp_avg_sq, embed_width, ids, rows, options, stream);
    } else {
      return SparseRowAdam<ElemT, IndexT, kRoundings>(table, exp_avg, exp_avg_sq, embed_width, ids, rows, options, stream,
                                                      exp_avg_ids, exp_avg_sq_ids);
    }
  }
  detail::SparseRowAdamNamed<ElemT, IndexT, kRoundings>(table, exp_avg, exp_avg_sq, embed_width, ids, rows, options, stream,
                                                        exp_avg_ids, exp_avg_sq_ids, row_names);
}

/**
 * @brief Advances the bias-factor clock by one step on the device: powers = (t, beta1^t, beta2^t) (fp64[3], starting at
 * (0, 1, 1)) becomes (t + 1, beta1^(t+1), beta2^(t+1)) and *bias_factor = sqrt(1 - beta2^t) / (1 - beta1^t) of the new
 * t, computed in fp64 and rounded once to fp32.  One single-thread launch, nothing read back: enqueue it in front of
 * SparseRowAdam(options.bias_factor_device = bias_factor) and a captured graph counts its own replays.
 */
inline void AdamClockAdvance(double* powers, float* bias_factor, const double beta1, const double beta2,
                             const hipStream_t stream = 0) {
  CUEMBED_ASSERT(powers != nullptr && bias_factor != nullptr);
  CUEMBED_ASSERT(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0);
  detail::AdamClockKernel<double><<<dim3(1), dim3(1), 0, stream>>>(powers, bias_factor, beta1, beta2);
}

}  // namespace cuembed

#endif  // CUEMBED_INCLUDE_SPARSE_ADAM_HPP_
