// MI355X (gfx950 / CDNA4) sparse optimizer step, the Adam family -- host API (an extension: the reference ends at the
// gradient).
//
//   cuembed::SparseRowAdam<ElemT, IndexT>(table, exp_avg, exp_avg_sq, embed_width, ids, rows, options, stream)
//   cuembed::AdamClockAdvance(powers, bias_factor, beta1, beta2, stream)
//
// SparseRowAdam consumes the compressed gradient like SparseRowUpdate (sparse_update.hpp) and keeps two fp32 moments per
// named row; AdamClockAdvance keeps the bias factor of the step in a device word, so that a captured step needs the host
// for neither the entry count nor the step number.
#ifndef CUEMBED_INCLUDE_SPARSE_ADAM_HPP_
#define CUEMBED_INCLUDE_SPARSE_ADAM_HPP_

#include "cuembed/include/sparse_adam_kernels.hpp"
#include "cuembed/include/sparse_update.hpp"

namespace cuembed {

//! Rule, hyper-parameters and the source of the entry count of one SparseRowAdam call.
struct SparseAdamOptions {
  AdamRule rule = AdamRule::kAdam;
  float lr = 0.f;                             //!< learning rate, unless ...
  const float* lr_device = nullptr;           //!< ... one fp32 word on the device holds it
  float bias_factor = 1.f;                    //!< c = sqrt(1 - beta2^t) / (1 - beta1^t) of step t (1: no correction), unless ...
  const float* bias_factor_device = nullptr;  //!< ... one fp32 word on the device holds it (AdamClockAdvance writes it)
  //! The kernel multiplies with these fp32 values as they are: form 1 - beta in double and round it once.
  float beta1 = 0.9f, one_minus_beta1 = 0.1f;
  float beta2 = 0.999f, one_minus_beta2 = 0.001f;
  float eps = 1e-8f;                          //!< added to sqrt(v)
  float weight_decay = 0.f;                   //!< decoupled (AdamW): w <- w - (lr * weight_decay) * w on the named rows; 0: off
  //! The entries are `pieces` blocks of `piece_rows` entries; entry j of piece p is valid iff j < count(p).
  int64_t piece_rows = 0;
  int pieces = 1;
  //! Exactly one source of the counts (see SparseUpdateOptions):
  int64_t num_rows = -1;
  const void* counts = nullptr;
  bool counts_are_int64 = false;
  const void* last_id = nullptr;
  //! Stochastic rounding of the one rounding to the table's type (see SparseUpdateOptions).
  bool stochastic_rounding = false;
  uint64_t rounding_seed = 0;
  uint64_t rounding_step = 0;
  const int64_t* rounding_step_device = nullptr;
};

namespace detail {

//! Entries a lane group keeps in flight when a lane holds one slice per entry.  With the two moment packs of a slice
//! next to its weights and gradient, two entries take 32 (fp32) to 48 (16-bit) registers of row data per lane: every
//! instantiation stays free of scratch and at or above 4 waves per SIMD (profiles/sparse_adam_kernel_resources.txt).
constexpr int kAdamEntriesInFlight = 2;

template <typename ElemT, typename IndexT, int N, AdamRule kRule, bool kStochastic>
inline void LaunchSparseRowAdam(ElemT* table, float* exp_avg, float* exp_avg_sq, const int width, const IndexT* ids,
                                const ElemT* rows, const SparseAdamOptions& o, const UpdateCounts& counts,
                                const hipStream_t stream) {
  const UpdateShape s = PlanUpdate(width / N, o.piece_rows * o.pieces, CurrentDeviceShape());
  UpdateRounding<kStochastic> rounding;
  if constexpr (kStochastic) {
    rounding.seed = o.rounding_seed;
    rounding.step = o.rounding_step;
    rounding.step_word = o.rounding_step_device;
  }
  AdamScalars h;
  h.beta1 = o.beta1;
  h.one_minus_beta1 = o.one_minus_beta1;
  h.beta2 = o.beta2;
  h.one_minus_beta2 = o.one_minus_beta2;
  h.eps = o.eps;
  h.weight_decay = o.weight_decay;
#define CUEMBED_LAUNCH_ADAM(CHUNKS, ENTRIES)                                                                        \
  SparseRowAdamKernel<ElemT, IndexT, N, kRule, CHUNKS, ENTRIES, kStochastic>                                        \
      <<<dim3(s.grid), dim3(kUpdateBlockThreads), 0, stream>>>(ids, rows, table, exp_avg, exp_avg_sq, width,         \
                                                               s.lanes_per_row, s.group, o.piece_rows, o.pieces,    \
                                                               counts, o.lr, o.lr_device, o.bias_factor,            \
                                                               o.bias_factor_device, h, rounding)
  if (s.chunks == 1) CUEMBED_LAUNCH_ADAM(1, kAdamEntriesInFlight);
  else if (s.chunks == kUpdateMaxChunks) CUEMBED_LAUNCH_ADAM(kUpdateMaxChunks, 1);
  else CUEMBED_LAUNCH_ADAM(0, 1);
#undef CUEMBED_LAUNCH_ADAM
}

template <typename ElemT, typename IndexT, int N, bool kStochastic>
inline void LaunchSparseRowAdamRule(ElemT* table, float* exp_avg, float* exp_avg_sq, const int width, const IndexT* ids,
                                    const ElemT* rows, const SparseAdamOptions& o, const UpdateCounts& counts,
                                    const hipStream_t stream) {
  switch (o.rule) {
    case AdamRule::kAdam:
      return LaunchSparseRowAdam<ElemT, IndexT, N, AdamRule::kAdam, kStochastic>(table, exp_avg, exp_avg_sq, width, ids, rows, o,
                                                                                counts, stream);
    case AdamRule::kRowwiseAdam:
      return LaunchSparseRowAdam<ElemT, IndexT, N, AdamRule::kRowwiseAdam, kStochastic>(table, exp_avg, exp_avg_sq, width, ids,
                                                                                       rows, o, counts, stream);
  }
  CUEMBED_ASSERT(false && "unknown Adam rule");
}

//! The lane width's instantiation: N = 16 / 8 / 4 bytes of ElemT.
template <typename ElemT, typename IndexT, bool kStochastic>
inline void LaunchSparseRowAdamBytes(const int bytes, ElemT* table, float* exp_avg, float* exp_avg_sq, const int width,
                                     const IndexT* ids, const ElemT* rows, const SparseAdamOptions& o,
                                     const UpdateCounts& counts, const hipStream_t stream) {
  constexpr int kMaxN = 16 / static_cast<int>(sizeof(ElemT));
  if (bytes == 16)
    LaunchSparseRowAdamRule<ElemT, IndexT, kMaxN, kStochastic>(table, exp_avg, exp_avg_sq, width, ids, rows, o, counts, stream);
  else if (bytes == 8)
    LaunchSparseRowAdamRule<ElemT, IndexT, kMaxN / 2, kStochastic>(table, exp_avg, exp_avg_sq, width, ids, rows, o, counts, stream);
  else
    LaunchSparseRowAdamRule<ElemT, IndexT, kMaxN / 4, kStochastic>(table, exp_avg, exp_avg_sq, width, ids, rows, o, counts, stream);
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
  using DevT = detail::DeviceElemT<ElemT>;
  const int sources = (options.num_rows >= 0) + (options.counts != nullptr) + (options.last_id != nullptr);
  CUEMBED_ASSERT(sources == 1);
  CUEMBED_ASSERT(options.pieces >= 1 && options.piece_rows >= 0);
  CUEMBED_ASSERT(options.pieces == 1 || options.counts != nullptr);   // several pieces: counts[pieces] on the device
  if (options.num_rows >= 0) CUEMBED_ASSERT(options.num_rows <= options.piece_rows);
  CUEMBED_ASSERT(options.beta1 >= 0.f && options.beta1 < 1.f && options.beta2 >= 0.f && options.beta2 < 1.f);
  CUEMBED_ASSERT(options.eps >= 0.f && options.weight_decay >= 0.f);
  constexpr bool kCanRoundStochastically = !std::is_same<ElemT, float>::value && kRoundings != UpdateRoundings::kNearestOnly;
  CUEMBED_ASSERT(!options.stochastic_rounding || kCanRoundStochastically);
  CUEMBED_ASSERT(options.stochastic_rounding || kRoundings != UpdateRoundings::kStochasticOnly);
  if (options.piece_rows == 0 || options.num_rows == 0) return;
  CUEMBED_ASSERT(table != nullptr && ids != nullptr && rows != nullptr);
  CUEMBED_ASSERT(exp_avg != nullptr && exp_avg_sq != nullptr);
  CUEMBED_ASSERT(reinterpret_cast<uintptr_t>(exp_avg_sq) % 4 == 0);
  const int bytes = detail::UpdateLaneBytes<DevT>(embed_width, table, rows, exp_avg, true,
                                                  options.rule == AdamRule::kAdam ? exp_avg_sq : nullptr);
  detail::UpdateCounts counts;
  counts.host_count = options.num_rows >= 0 ? options.num_rows : -1;
  counts.count_words = options.counts;
  counts.count_words_are_64 = options.counts_are_int64 ? 1 : 0;
  counts.last_id = options.last_id;
  DevT* t = reinterpret_cast<DevT*>(table);
  const DevT* g = reinterpret_cast<const DevT*>(rows);
  if constexpr (kCanRoundStochastically) {
    if (options.stochastic_rounding)
      return detail::LaunchSparseRowAdamBytes<DevT, IndexT, true>(bytes, t, exp_avg, exp_avg_sq, embed_width, ids, g, options,
                                                                  counts, stream);
  }
  if constexpr (kRoundings != UpdateRoundings::kStochasticOnly)
    detail::LaunchSparseRowAdamBytes<DevT, IndexT, false>(bytes, t, exp_avg, exp_avg_sq, embed_width, ids, g, options, counts,
                                                          stream);
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
