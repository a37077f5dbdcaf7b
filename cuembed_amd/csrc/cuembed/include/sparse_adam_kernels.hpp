// MI355X (gfx950 / CDNA4) sparse optimizer step, the Adam family -- the kernels.
//
// The structure is SparseRowUpdateKernel's (sparse_update_kernels.hpp): one power-of-two lane group per gradient entry,
// 16 / 8 / 4 bytes of the row per lane and slice, kChunks slices per lane in registers (1, 4, or 0 = a run-time loop),
// the ids of an iteration first, then every load of the iteration, then the arithmetic and the stores; gradient rows
// with non-temporal loads; the entry counts read on the device (UpdateCounts); no atomics on table data, so the valid
// entries must name DISTINCT rows.  What is new is the state: two fp32 tensors.
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

/**
 * @brief table[ids[k], :] and the moments of row ids[k] <- rule(table[ids[k], :], rows[k, :]) for every valid entry k.
 *
 * Launch: as SparseRowUpdateKernel -- 1-D grid of kUpdateBlockThreads-thread workgroups, `group` (a power of two <= 64)
 * lanes per entry, lanes_per_row = width / N slices per row; kChunks >= 1 needs lanes_per_row <= kChunks * group.
 * kEntries (1 or 2) entries are in flight per group when kChunks == 1.
 */
template <typename ElemT, typename IndexT, int N, AdamRule kRule, int kChunks, int kEntriesInFlight, bool kStochastic = false>
__global__ void __launch_bounds__(kUpdateBlockThreads)
    SparseRowAdamKernel(const IndexT* __restrict__ ids, const ElemT* __restrict__ rows, ElemT* __restrict__ table,
                        float* __restrict__ exp_avg, float* __restrict__ exp_avg_sq, const int width,
                        const int lanes_per_row, const int group, const int64_t piece_rows, const int pieces,
                        const UpdateCounts counts, const float lr_value, const float* __restrict__ lr_word,
                        const float bias_value, const float* __restrict__ bias_word, const AdamScalars h,
                        const UpdateRounding<kStochastic> rounding = UpdateRounding<kStochastic>()) {
  static_assert(!kStochastic || sizeof(ElemT) == 2, "stochastic rounding is for the 16-bit table types");
  static_assert(kEntriesInFlight == 1 || (kEntriesInFlight == 2 && kChunks == 1), "two entries in flight: one slice per lane");
  using RoundT = SliceRounding<ElemT, N, kStochastic>;
  constexpr bool kRowwise = kRule == AdamRule::kRowwiseAdam;
  constexpr int kEntries = kEntriesInFlight;
  constexpr int kSlices = kChunks == 0 ? 1 : kChunks;
  AdamStepSizes z;
  {
    const float lr = lr_word != nullptr ? *lr_word : lr_value;
    const float c = bias_word != nullptr ? *bias_word : bias_value;
    z.step = Arith<float>::mul(lr, c);
    z.decay = Arith<float>::mul(lr, h.weight_decay);
    z.decays = h.weight_decay != 0.f;
  }
  uint64_t seed = 0, round_step = 0;
  if constexpr (kStochastic) {
    seed = rounding.seed;
    round_step = rounding.step_word != nullptr ? static_cast<uint64_t>(*rounding.step_word) : rounding.step;
  }
  const int lane = static_cast<int>(threadIdx.x) & (group - 1);
  const int groups_per_block = kUpdateBlockThreads / group;
  const int64_t first = static_cast<int64_t>(blockIdx.x) * groups_per_block + static_cast<int>(threadIdx.x) / group;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * groups_per_block;

  for (int piece = 0; piece < pieces; ++piece) {
    const int64_t count = PieceCount<IndexT>(counts, piece, piece_rows);
    const int64_t base = static_cast<int64_t>(piece) * piece_rows;
    for (int64_t k = first; k < count; k += stride * kEntries) {
      int64_t r[kEntries];
      bool live[kEntries];
#pragma unroll
      for (int u = 0; u < kEntries; ++u) {
        live[u] = k + u * stride < count;
        r[u] = live[u] ? WidenIndex(ids[base + k + u * stride]) : 0;
      }
      if constexpr (kChunks == 0) {
        // any width: slices lane, lane + group, ... one after the other
        const ElemT* g_row = RowPtr(rows, base + k, width);
        ElemT* w_row = const_cast<ElemT*>(RowPtr(table, r[0], width));
        float* m_row = exp_avg + RowElems(r[0], width);
        float scale = 0.f;
        if constexpr (kRowwise) {
          const float before = exp_avg_sq[r[0]];
          float sum = 0.f;
          for (int c = lane; c < lanes_per_row; c += group) sum = AddSquares(sum, LoadPack<ElemT, N>(g_row + c * N));
          scale = RowwiseAdamScale(exp_avg_sq + r[0], before, GroupSum(sum, group), width, lane == 0, z, h);
        }
        for (int c = lane; c < lanes_per_row; c += group) {
          const Pack<ElemT, N> g = kRowwise ? LoadPack<ElemT, N>(g_row + c * N) : LoadPackStreaming<ElemT, N>(g_row + c * N);
          const Pack<ElemT, N> w = LoadPack<ElemT, N>(w_row + c * N);
          StatePack<N> m = StatePack<N>::Load(m_row + c * N);
          RoundT round;
          if constexpr (kStochastic) round = RoundT(seed, round_step, r[0], c * N);
          if constexpr (kRowwise) {
            StorePack<ElemT, N>(w_row + c * N, RowwiseAdamStep(w, g, m, scale, z, h, round));
          } else {
            float* v_at = exp_avg_sq + RowElems(r[0], width) + c * N;
            StatePack<N> v = StatePack<N>::Load(v_at);
            StorePack<ElemT, N>(w_row + c * N, AdamStep(w, g, m, v, z, h, round));
            v.Store(v_at);
          }
          m.Store(m_row + c * N);
        }
      } else {
        Pack<ElemT, N> g[kEntries][kSlices], w[kEntries][kSlices];
        StatePack<N> m[kEntries][kSlices];
        StatePack<N> v[kRowwise ? 1 : kEntries][kRowwise ? 1 : kSlices];
        bool has[kEntries][kSlices];
        float row_v[kEntries];
        RoundT round[kEntries][kSlices];
#pragma unroll
        for (int u = 0; u < kEntries; ++u) {
          if constexpr (kRowwise) row_v[u] = live[u] ? exp_avg_sq[r[u]] : 0.f;
#pragma unroll
          for (int c = 0; c < kSlices; ++c) {
            const int col = (lane + c * group) * N;
            has[u][c] = live[u] && lane + c * group < lanes_per_row;
            if (has[u][c]) {
              g[u][c] = LoadPackStreaming<ElemT, N>(RowPtr(rows, base + k + u * stride, width) + col);
              w[u][c] = LoadPack<ElemT, N>(RowPtr(table, r[u], width) + col);
              m[u][c] = StatePack<N>::Load(exp_avg + RowElems(r[u], width) + col);
              if constexpr (!kRowwise) v[u][c] = StatePack<N>::Load(exp_avg_sq + RowElems(r[u], width) + col);
            }
          }
        }
        if constexpr (kStochastic) {
          // the random bits need nothing that was loaded: they are computed while the loads are in flight
#pragma unroll
          for (int u = 0; u < kEntries; ++u)
#pragma unroll
            for (int c = 0; c < kSlices; ++c)
              if (has[u][c]) round[u][c] = RoundT(seed, round_step, r[u], (lane + c * group) * N);
        }
#pragma unroll
        for (int u = 0; u < kEntries; ++u) {
          float scale = 0.f;
          if constexpr (kRowwise) {
            // (a group whose second entry is past the count still takes part in the butterfly: its lanes are active)
            float sum = 0.f;
#pragma unroll
            for (int c = 0; c < kSlices; ++c)
              if (has[u][c]) sum = AddSquares(sum, g[u][c]);
            sum = GroupSum(sum, group);
            if (live[u]) scale = RowwiseAdamScale(exp_avg_sq + r[u], row_v[u], sum, width, lane == 0, z, h);
          }
#pragma unroll
          for (int c = 0; c < kSlices; ++c) {
            if (!has[u][c]) continue;
            const int col = (lane + c * group) * N;
            ElemT* w_at = const_cast<ElemT*>(RowPtr(table, r[u], width)) + col;
            if constexpr (kRowwise) {
              StorePack<ElemT, N>(w_at, RowwiseAdamStep(w[u][c], g[u][c], m[u][c], scale, z, h, round[u][c]));
            } else {
              StorePack<ElemT, N>(w_at, AdamStep(w[u][c], g[u][c], m[u][c], v[u][c], z, h, round[u][c]));
              v[u][c].Store(exp_avg_sq + RowElems(r[u], width) + col);
            }
            m[u][c].Store(exp_avg + RowElems(r[u], width) + col);
          }
        }
      }
    }
  }
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
