// MI355X (gfx950 / CDNA4) sparse optimizer step, the Adam family -- the kernels.
//
// The walk over the named rows is the one of every rule (WalkNamedRows, sparse_update_kernels.hpp: lane groups, slices,
// entries in flight, device-side counts, DISTINCT rows).  What is Adam's is here: the scalars, the arithmetic of a slice
// and of a row, the rule type that hands them to the walk, and the bias-factor clock.  The state is two fp32 tensors.
//
//   * kAdam: exp_avg and exp_avg_sq are [rows, width]; a lane moves 2 * N fp32 state elements per slice next to its N
//     weights and N gradient elements (22 bytes per fp16 element against Adagrad's 14).
//   * kRowwiseAdam: exp_avg is [rows, width], exp_avg_sq ONE word per row, updated from the mean of the row's squared
//     gradient with the butterfly of the row-wise Adagrad rule (AddSquares / GroupSum: every lane ends with the same
//     bits).  With the run-time loop the gradient row is read twice, the second time out of the cache.
//   * Only rows that a valid entry names are read or written: the moments of other rows do not decay (the "lazy"
//     behaviour of torch.optim.SparseAdam).
//   * All arithmetic is fp32 with one unfused IEEE operation per step (Arith); the one rounding to the table's type
//     happens at the store, to nearest or stochastically (SliceRounding).  The kernel does no fp64 arithmetic: the bias
//     factor c = sqrt(1 - beta2^t) / (1 - beta1^t) arrives as an fp32 value or an fp32 device word (AdamClockKernel
//     keeps that word current inside a captured graph), and the step size is the one product lr * c.
#ifndef CUEMBED_INCLUDE_SPARSE_ADAM_KERNELS_HPP_
#define CUEMBED_INCLUDE_SPARSE_ADAM_KERNELS_HPP_

#include "cuembed/include/sparse_update_kernels.hpp"

namespace cuembed {

//! The rules (all in fp32; g = gradient element, w = table element, m / v = first / second moment, c = bias factor):
//!   w <- w - (lr * weight_decay) * w                         (only if weight_decay != 0: decoupled, named rows only)
//!   m <- beta1 * m + (1 - beta1) * g
enum class AdamRule {
  kAdam = 0,        //!< v <- beta2 * v + (1 - beta2) * (g * g);  w <- w - (lr * c) * m / (sqrt(v) + eps)
  kRowwiseAdam = 1  //!< v_r <- beta2 * v_r + (1 - beta2) * mean_j(g_j^2);  w_j <- w_j - ((lr * c) / (sqrt(v_r) + eps)) * m_j
};

namespace detail {

//! The hyper-parameters as the fp32 values the kernel multiplies with: the host forms 1 - beta in double and rounds once.
struct AdamScalars {
  float beta1, one_minus_beta1;
  float beta2, one_minus_beta2;
  float eps;
  float weight_decay;
};

//! What one launch derives from the scalars, the learning rate and the bias factor, once per thread.
struct AdamStepSizes {
  float step;    //!< lr * c
  float decay;   //!< lr * weight_decay
  bool decays;   //!< weight_decay != 0
};

__device__ __forceinline__ float DecayedWeight(const float w, const AdamStepSizes& z) {
  using A = Arith<float>;
  return z.decays ? A::add(w, -A::mul(z.decay, w)) : w;
}

__device__ __forceinline__ float FirstMoment(const float m, const float x, const AdamScalars& h) {
  using A = Arith<float>;
  return A::add(A::mul(h.beta1, m), A::mul(h.one_minus_beta1, x));
}

__device__ __forceinline__ float SecondMoment(const float v, const float x_squared, const AdamScalars& h) {
  using A = Arith<float>;
  return A::add(A::mul(h.beta2, v), A::mul(h.one_minus_beta2, x_squared));
}

//! Adam on one slice: m and v updated in place, returns the new weights.
template <typename ElemT, int N, typename RoundT = SliceRounding<ElemT, N, false>>
__device__ __forceinline__ Pack<ElemT, N> AdamStep(const Pack<ElemT, N>& w, const Pack<ElemT, N>& g, StatePack<N>& m,
                                                   StatePack<N>& v, const AdamStepSizes& z, const AdamScalars& h,
                                                   const RoundT& round = RoundT()) {
  using A = Arith<float>;
  Pack<ElemT, N> out;
#pragma unroll
  for (int e = 0; e < N; ++e) {
    const float x = A::widen(g.v[e]);
    const float m_new = FirstMoment(m.at(e), x, h);
    const float v_new = SecondMoment(v.at(e), A::mul(x, x), h);
    m.at(e) = m_new;
    v.at(e) = v_new;
    const float d = A::mul(z.step, m_new) / A::add(sqrtf(v_new), h.eps);
    out.v[e] = round(A::add(DecayedWeight(A::widen(w.v[e]), z), -d), e);
  }
  return out;
}

//! Row-wise Adam on one slice: m updated in place, returns w - scale * m with scale = (lr * c) / (sqrt(v_r) + eps).
template <typename ElemT, int N, typename RoundT = SliceRounding<ElemT, N, false>>
__device__ __forceinline__ Pack<ElemT, N> RowwiseAdamStep(const Pack<ElemT, N>& w, const Pack<ElemT, N>& g,
                                                          StatePack<N>& m, const float scale, const AdamStepSizes& z,
                                                          const AdamScalars& h, const RoundT& round = RoundT()) {
  using A = Arith<float>;
  Pack<ElemT, N> out;
#pragma unroll
  for (int e = 0; e < N; ++e) {
    const float m_new = FirstMoment(m.at(e), A::widen(g.v[e]), h);
    m.at(e) = m_new;
    out.v[e] = round(A::add(DecayedWeight(A::widen(w.v[e]), z), -A::mul(scale, m_new)), e);
  }
  return out;
}

//! The row-wise rule's per-row part: v_r <- beta2 * v_r + (1 - beta2) * (sum / width); returns (lr * c) / (sqrt(v_r) +
//! eps).  `before` was loaded together with the rows; every lane of the group computes the same value from the same
//! bits and lane 0 stores the state.
__device__ __forceinline__ float RowwiseAdamScale(float* v_of_row, const float before, const float sum, const int width,
                                                  const bool store, const AdamStepSizes& z, const AdamScalars& h) {
  const float v_new = SecondMoment(before, sum / static_cast<float>(width), h);
  if (store) *v_of_row = v_new;
  return z.step / Arith<float>::add(sqrtf(v_new), h.eps);
}

//! The two rules as the walk sees them (WalkNamedRows, sparse_update_kernels.hpp): exp_avg is per element; exp_avg_sq
//! is per element (kAdam) or the row's word (kRowwiseAdam).
template <AdamRule kRule>
struct AdamStepRule {
  static constexpr bool kRowState = kRule == AdamRule::kRowwiseAdam;
  static constexpr int kStates = kRowState ? 1 : 2;
  AdamStepSizes z;
  AdamScalars h;
  __device__ __forceinline__ float Row(float* word, const float before, const float sum, const int width,
                                       const bool store) const {
    return RowwiseAdamScale(word, before, sum, width, store, z, h);
  }
  template <typename ElemT, int N, typename RoundT>
  __device__ __forceinline__ Pack<ElemT, N> Slice(const Pack<ElemT, N>& w, const Pack<ElemT, N>& g, StatePack<N>* s,
                                                  const float row, const RoundT& round) const {
    if constexpr (kRowState) return RowwiseAdamStep(w, g, s[0], row, z, h, round);
    else return AdamStep(w, g, s[0], s[1], z, h, round);
  }
};

/**
 * @brief table[ids[k], :] and the moments of row ids[k] <- rule(table[ids[k], :], rows[k, :]) for every valid entry k.
 *
 * Launch: as SparseRowUpdateKernel -- 1-D grid of kUpdateBlockThreads-thread workgroups, `group` (a power of two <= 64)
 * lanes per entry, lanes_per_row = width / N slices per row; kChunks >= 1 needs lanes_per_row <= kChunks * group.
 * kEntriesInFlight (1 or 2) entries are in flight per group when kChunks == 1.
 */
template <typename ElemT, typename IndexT, int N, AdamRule kRule, int kChunks, int kEntriesInFlight, bool kStochastic = false>
__global__ void __launch_bounds__(kUpdateBlockThreads)
    SparseRowAdamKernel(const IndexT* __restrict__ ids, const ElemT* __restrict__ rows, ElemT* __restrict__ table,
                        float* __restrict__ exp_avg, float* __restrict__ exp_avg_sq, const int width,
                        const int lanes_per_row, const int group, const int64_t piece_rows, const int pieces,
                        const UpdateCounts counts, const float lr_value, const float* __restrict__ lr_word,
                        const float bias_value, const float* __restrict__ bias_word, const AdamScalars h,
                        const UpdateRounding<kStochastic> rounding = UpdateRounding<kStochastic>()) {
  const float lr = lr_word != nullptr ? *lr_word : lr_value;
  const float c = bias_word != nullptr ? *bias_word : bias_value;
  const AdamStepRule<kRule> rule{{Arith<float>::mul(lr, c), Arith<float>::mul(lr, h.weight_decay), h.weight_decay != 0.f}, h};
  WalkNamedRows<ElemT, IndexT, N, kChunks, kEntriesInFlight, kStochastic>(
      ids, rows, table, exp_avg, exp_avg_sq, width, lanes_per_row, group, piece_rows, pieces, counts, rounding, rule);
}

/**
 * @brief The same step with the moments in places of their own: entry k's weights at table[ids[k], :], its first moment
 * at row exp_avg_ids[k] of `exp_avg`, its second at row exp_avg_sq_ids[k] of `exp_avg_sq` -- a row of `width` elements
 * (kAdam) or the row's one word (kRowwiseAdam).  WalkNamedRows' kPlaced + kPlacedTwice: what a table behind the row
 * cache with two state planes launches (row_cache.hpp).  Round to nearest; SparseRowAdamNamedKernel rounds
 * stochastically.  Same launch as SparseRowAdamKernel.
 */
template <typename ElemT, typename IndexT, int N, AdamRule kRule, int kChunks, int kEntriesInFlight, bool kStochastic = false>
__global__ void __launch_bounds__(kUpdateBlockThreads)
    SparseRowAdamPlacedKernel(const IndexT* __restrict__ ids, const int64_t* __restrict__ exp_avg_ids,
                              const int64_t* __restrict__ exp_avg_sq_ids, const ElemT* __restrict__ rows,
                              ElemT* __restrict__ table, float* __restrict__ exp_avg, float* __restrict__ exp_avg_sq,
                              const int width, const int lanes_per_row, const int group, const int64_t piece_rows,
                              const int pieces, const UpdateCounts counts, const float lr_value,
                              const float* __restrict__ lr_word, const float bias_value,
                              const float* __restrict__ bias_word, const AdamScalars h) {
  static_assert(!kStochastic, "placed moments are updated with round to nearest");
  const float lr = lr_word != nullptr ? *lr_word : lr_value;
  const float c = bias_word != nullptr ? *bias_word : bias_value;
  const AdamStepRule<kRule> rule{{Arith<float>::mul(lr, c), Arith<float>::mul(lr, h.weight_decay), h.weight_decay != 0.f}, h};
  WalkNamedRows<ElemT, IndexT, N, kChunks, kEntriesInFlight, false, true, true>(
      ids, rows, table, exp_avg, exp_avg_sq, width, lanes_per_row, group, piece_rows, pieces, counts,
      UpdateRounding<false>(), rule, exp_avg_ids, exp_avg_sq_ids);
}

/**
 * @brief The placed step with stochastic rounding: as SparseRowAdamPlacedKernel, and the rounding bits of entry k are
 * those of table row row_names[k] (WalkNamedRows' kNamed): a translated id is not the table row, so the walk carries the
 * rows next to the three placed ids.  16-bit tables only.  Same launch as SparseRowAdamKernel.
 */
template <typename ElemT, typename IndexT, int N, AdamRule kRule, int kChunks, int kEntriesInFlight>
__global__ void __launch_bounds__(kUpdateBlockThreads)
    SparseRowAdamNamedKernel(const IndexT* __restrict__ ids, const int64_t* __restrict__ exp_avg_ids,
                             const int64_t* __restrict__ exp_avg_sq_ids, const int64_t* __restrict__ row_names,
                             const ElemT* __restrict__ rows, ElemT* __restrict__ table, float* __restrict__ exp_avg,
                             float* __restrict__ exp_avg_sq, const int width, const int lanes_per_row, const int group,
                             const int64_t piece_rows, const int pieces, const UpdateCounts counts,
                             const float lr_value, const float* __restrict__ lr_word, const float bias_value,
                             const float* __restrict__ bias_word, const AdamScalars h,
                             const UpdateRounding<true> rounding) {
  const float lr = lr_word != nullptr ? *lr_word : lr_value;
  const float c = bias_word != nullptr ? *bias_word : bias_value;
  const AdamStepRule<kRule> rule{{Arith<float>::mul(lr, c), Arith<float>::mul(lr, h.weight_decay), h.weight_decay != 0.f}, h};
  WalkNamedRows<ElemT, IndexT, N, kChunks, kEntriesInFlight, true, true, true, true>(
      ids, rows, table, exp_avg, exp_avg_sq, width, lanes_per_row, group, piece_rows, pieces, counts, rounding, rule,
      exp_avg_ids, exp_avg_sq_ids, row_names);
}

/**
 * @brief The same step on a GROUP of separate table tensors: ids[k] is a global row of the tables laid end to end, and
 * entry k updates row ids[k] - row_base[t] of tables[t] and of that table's two moment tensors (WalkNamedRows' kGrouped;
 * grouped.state0 = the exp_avg bases, grouped.state1 = the exp_avg_sq bases).  Round to nearest.  Same launch as
 * SparseRowAdamKernel, plus GroupedLdsWords(num_tables, 2) * 8 bytes of dynamic LDS.
 */
template <typename ElemT, typename IndexT, int N, AdamRule kRule, int kChunks, int kEntriesInFlight>
__global__ void __launch_bounds__(kUpdateBlockThreads)
    SparseRowAdamGroupedKernel(const IndexT* __restrict__ ids, const ElemT* __restrict__ rows,
                               const GroupedTables<true> grouped, const int width, const int lanes_per_row,
                               const int group, const int64_t piece_rows, const int pieces, const UpdateCounts counts,
                               const float lr_value, const float* __restrict__ lr_word, const float bias_value,
                               const float* __restrict__ bias_word, const AdamScalars h) {
  const float lr = lr_word != nullptr ? *lr_word : lr_value;
  const float c = bias_word != nullptr ? *bias_word : bias_value;
  const AdamStepRule<kRule> rule{{Arith<float>::mul(lr, c), Arith<float>::mul(lr, h.weight_decay), h.weight_decay != 0.f}, h};
  WalkNamedRows<ElemT, IndexT, N, kChunks, kEntriesInFlight, false, false, false, false, true>(
      ids, rows, nullptr, nullptr, nullptr, width, lanes_per_row, group, piece_rows, pieces, counts,
      UpdateRounding<false>(), rule, nullptr, nullptr, nullptr, grouped);
}

/**
 * @brief The grouped Adam step with stochastic rounding (16-bit tables): as SparseRowAdamGroupedKernel, and the one
 * rounding of entry k draws the bits of (grouped.seeds[t], step, ids[k] - row_base[t], column), t the entry's table:
 * those of SparseRowAdamKernel<.., kStochastic> on table t alone with seed seeds[t].  rounding.seed is not read.
 * GroupedLdsWords(num_tables, 2, true) * 8 bytes of dynamic LDS.
 */
template <typename ElemT, typename IndexT, int N, AdamRule kRule, int kChunks, int kEntriesInFlight>
__global__ void __launch_bounds__(kUpdateBlockThreads)
    SparseRowAdamGroupedStochasticKernel(const IndexT* __restrict__ ids, const ElemT* __restrict__ rows,
                                         const GroupedSeededTables grouped, const int width,
                                         const int lanes_per_row, const int group, const int64_t piece_rows,
                                         const int pieces, const UpdateCounts counts, const float lr_value,
                                         const float* __restrict__ lr_word, const float bias_value,
                                         const float* __restrict__ bias_word, const AdamScalars h,
                                         const UpdateRounding<true> rounding) {
  static_assert(sizeof(ElemT) == 2, "stochastic rounding is for the 16-bit table types");
  const float lr = lr_word != nullptr ? *lr_word : lr_value;
  const float c = bias_word != nullptr ? *bias_word : bias_value;
  const AdamStepRule<kRule> rule{{Arith<float>::mul(lr, c), Arith<float>::mul(lr, h.weight_decay), h.weight_decay != 0.f}, h};
  WalkNamedRows<ElemT, IndexT, N, kChunks, kEntriesInFlight, true, false, false, false, true>(
      ids, rows, nullptr, nullptr, nullptr, width, lanes_per_row, group, piece_rows, pieces, counts, rounding, rule,
      nullptr, nullptr, nullptr, grouped);
}

/**
 * @brief The bias-factor clock: one thread advances (t, beta1^t, beta2^t) in fp64 and writes
 * c = sqrt(1 - beta2^t) / (1 - beta1^t), computed in fp64 and rounded once, to the fp32 word the update kernel reads.
 * Launch <<<1, 1>>>.  The running products carry a relative error of about t * 2^-53.  (A template so that the header
 * can be included from several translation units; RealT is double.)
 */
template <typename RealT>
__global__ void AdamClockKernel(RealT* __restrict__ powers, float* __restrict__ bias_factor, const RealT beta1,
                                const RealT beta2) {
  static_assert(sizeof(RealT) == 8, "the clock runs in fp64");
  const RealT t = powers[0] + 1.0;
  const RealT p1 = powers[1] * beta1;
  const RealT p2 = powers[2] * beta2;
  powers[0] = t;
  powers[1] = p1;
  powers[2] = p2;
  *bias_factor = static_cast<float>(sqrt(1.0 - p2) / (1.0 - p1));
}

}  // namespace detail
}  // namespace cuembed

#endif  // CUEMBED_INCLUDE_SPARSE_ADAM_KERNELS_HPP_
