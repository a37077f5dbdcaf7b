// MI355X (gfx950 / CDNA4) sparse optimizer step -- the kernel.
//
// The reference stops at the compressed gradient (its README lists optimizers under "future release"); this is the
// consumer of that gradient: for every valid entry k, row r = ids[k] of the table (and the optimizer state of row r)
// is updated in place from rows[k, :].  Rows that no entry names are neither read nor written.
//
//   * One lane group (a power of two, at most a wave) per gradient entry; every lane owns `kChunks` slices of N
//     elements (16 bytes wherever the row size and the base pointers allow, 8 or 4 bytes otherwise).  A 512-byte row
//     takes half a wave, so a wave of 256-thread workgroups keeps two rows -- with two entries in flight per group,
//     four -- in flight.
//   * The ids of an iteration are loaded first, then every gradient and table slice of the iteration, then the
//     arithmetic and the stores.  Gradient rows are read once, with non-temporal loads (nothing reads them again);
//     table rows are read and written with plain accesses (the next forward looks the hot ones up again).
//   * All arithmetic is fp32 with one unfused IEEE operation per step (Arith) and exactly one rounding to the
//     table's type at the store.
//   * Row-wise Adagrad reduces the row's sum of squares inside the lane group with a butterfly of cross-lane reads
//     (`__shfl_xor`): no LDS, no atomics.  Every lane ends with the same bits, so no broadcast is needed.
//   * The number of valid entries is read on the device (UpdateCounts): the grid is fixed from the capacity, every
//     group strides over the entries of a piece, and a workgroup with nothing to do leaves after reading the counts.
//     Entries at or past the count are ignored whatever they hold; a count above the capacity (the backward then
//     wrote nothing) or below zero makes the piece empty.
//   * The valid entries must name DISTINCT rows (a coalesced gradient): there are no atomics on table data.
#ifndef CUEMBED_INCLUDE_SPARSE_UPDATE_KERNELS_HPP_
#define CUEMBED_INCLUDE_SPARSE_UPDATE_KERNELS_HPP_

#include "cuembed/include/gather_reduce_kernels.hpp"

namespace cuembed {

//! The update rules (all in fp32; g = gradient element, w = table element, s = state):
enum class UpdateRule {
  kSgd = 0,            //!< w <- w - lr * g                                           (no state)
  kAdagrad = 1,        //!< s <- s + g^2;  w <- w - lr * g / (sqrt(s) + eps)          (fp32 state [rows, width])
  kRowwiseAdagrad = 2  //!< s_r <- s_r + mean_j(g_j^2);  w_j <- w_j - lr * g_j / (sqrt(s_r) + eps)   (fp32 state [rows])
};

namespace detail {

constexpr int kUpdateBlockThreads = 256;
//! Slices of a row a lane holds in registers at once: 1 (the row fits its lane group), 4 (rows of up to four times
//! the group), or 0 = a run-time loop over the slices for anything wider (row-wise Adagrad then reads the gradient
//! row a second time, out of the cache it has just been loaded into).
constexpr int kUpdateMaxChunks = 4;

//! Where the number of valid entries of each piece comes from; exactly one source is set.
struct UpdateCounts {
  int64_t host_count;       //!< >= 0: known on the host (one piece); < 0: read on the device
  const void* count_words;  //!< counts[pieces] on the device ...
  int count_words_are_64;   //!< ... as int64 (else int32)
  const void* last_id;      //!< one index-typed word on the device: count = *last_id + 1 (one piece)
};

template <typename IndexT>
__device__ __forceinline__ int64_t PieceCount(const UpdateCounts& c, const int piece, const int64_t piece_rows) {
  int64_t n;
  if (c.host_count >= 0) n = c.host_count;
  else if (c.last_id != nullptr) n = static_cast<int64_t>(*static_cast<const IndexT*>(c.last_id)) + 1;
  else if (c.count_words_are_64) n = static_cast<const int64_t*>(c.count_words)[piece];
  else n = static_cast<const int32_t*>(c.count_words)[piece];
  return (n < 0 || n > piece_rows) ? 0 : n;   // over capacity: the producer wrote nothing, so nothing is applied
}

//! N fp32 state elements (Adagrad) move as packs of at most four: 16 bytes per access.
template <int N>
struct StatePack {
  static constexpr int kM = N < 4 ? N : 4;
  Pack<float, kM> p[N / kM];
  static __device__ __forceinline__ StatePack Load(const float* s) {
    StatePack r;
#pragma unroll
    for (int i = 0; i < N / kM; ++i) r.p[i] = *reinterpret_cast<const Pack<float, kM>*>(s + i * kM);
    return r;
  }
  __device__ __forceinline__ void Store(float* s) const {
#pragma unroll
    for (int i = 0; i < N / kM; ++i) *reinterpret_cast<Pack<float, kM>*>(s + i * kM) = p[i];
  }
  __device__ __forceinline__ float& at(int e) { return p[e / kM].v[e % kM]; }
};

//! sum_e g_e^2 of one slice, added to `acc` in element order.
template <typename ElemT, int N>
__device__ __forceinline__ float AddSquares(float acc, const Pack<ElemT, N>& g) {
  using A = Arith<float>;
#pragma unroll
  for (int e = 0; e < N; ++e) {
    const float x = A::widen(g.v[e]);
    acc = A::add(acc, A::mul(x, x));
  }
  return acc;
}

//! Sum over the lanes of a group (a power of two <= 64): every lane ends with the same bits.
__device__ __forceinline__ float GroupSum(float v, const int group) {
  for (int d = group >> 1; d > 0; d >>= 1) v = Arith<float>::add(v, __shfl_xor(v, d));
  return v;
}

//! w <- w - step * g, one slice (SGD: step = lr; row-wise Adagrad: step = lr / (sqrt(s_r) + eps)).
template <typename ElemT, int N>
__device__ __forceinline__ Pack<ElemT, N> ScaledStep(const Pack<ElemT, N>& w, const Pack<ElemT, N>& g, const float step) {
  using A = Arith<float>;
  Pack<ElemT, N> out;
#pragma unroll
  for (int e = 0; e < N; ++e)
    out.v[e] = static_cast<ElemT>(A::add(A::widen(w.v[e]), -A::mul(step, A::widen(g.v[e]))));
  return out;
}

//! Adagrad on one slice: s <- s + g^2 (in place), returns w - lr * g / (sqrt(s) + eps).
template <typename ElemT, int N>
__device__ __forceinline__ Pack<ElemT, N> AdagradStep(const Pack<ElemT, N>& w, const Pack<ElemT, N>& g, StatePack<N>& s,
                                                      const float lr, const float eps) {
  using A = Arith<float>;
  Pack<ElemT, N> out;
#pragma unroll
  for (int e = 0; e < N; ++e) {
    const float x = A::widen(g.v[e]);
    const float acc = A::add(s.at(e), A::mul(x, x));
    s.at(e) = acc;
    const float d = A::mul(lr, x) / A::add(sqrtf(acc), eps);
    out.v[e] = static_cast<ElemT>(A::add(A::widen(w.v[e]), -d));
  }
  return out;
}

//! The row-wise rule's per-row part: s_r <- s_r + sum / width; returns lr / (sqrt(s_r) + eps).  `before` is the row's
//! state, loaded together with the rows so that the load does not wait for the reduction.  Every lane of the group
//! computes the same value from the same bits; lane 0 stores the state.
__device__ __forceinline__ float RowwiseStep(float* state_of_row, const float before, const float sum, const int width,
                                             const bool store, const float lr, const float eps) {
  using A = Arith<float>;
  const float acc = A::add(before, sum / static_cast<float>(width));
  if (store) *state_of_row = acc;
  return lr / A::add(sqrtf(acc), eps);
}

/**
 * @brief table[ids[k], :] (and its state) <- rule(table[ids[k], :], rows[k, :]) for every valid entry k.
 *
 * Launch: 1-D grid of kUpdateBlockThreads-thread workgroups, `group` (a power of two <= 64) lanes per entry,
 * lanes_per_row = width / N slices per row; kChunks >= 1 needs lanes_per_row <= kChunks * group.
 * Entries: `pieces` blocks of `piece_rows` entries, entry j of piece p valid iff j < count(p).
 */
template <typename ElemT, typename IndexT, int N, UpdateRule kRule, int kChunks>
__global__ void __launch_bounds__(kUpdateBlockThreads)
    SparseRowUpdateKernel(const IndexT* __restrict__ ids, const ElemT* __restrict__ rows, ElemT* __restrict__ table,
                          float* __restrict__ state, const int width, const int lanes_per_row, const int group,
                          const int64_t piece_rows, const int pieces, const UpdateCounts counts, const float lr_value,
                          const float* __restrict__ lr_word, const float eps) {
  constexpr bool kRowwise = kRule == UpdateRule::kRowwiseAdagrad;
  constexpr bool kAdagrad = kRule == UpdateRule::kAdagrad;
  // entries in flight per group: two when a lane holds one slice per entry
  constexpr int kEntries = kChunks == 1 ? 2 : 1;
  constexpr int kSlices = kChunks == 0 ? 1 : kChunks;
  const float lr = lr_word != nullptr ? *lr_word : lr_value;
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
        float step = lr;
        if constexpr (kRowwise) {
          const float before = state[r[0]];
          float sum = 0.f;
          for (int c = lane; c < lanes_per_row; c += group) sum = AddSquares(sum, LoadPack<ElemT, N>(g_row + c * N));
          step = RowwiseStep(state + r[0], before, GroupSum(sum, group), width, lane == 0, lr, eps);
        }
        for (int c = lane; c < lanes_per_row; c += group) {
          const Pack<ElemT, N> g = kRowwise ? LoadPack<ElemT, N>(g_row + c * N) : LoadPackStreaming<ElemT, N>(g_row + c * N);
          const Pack<ElemT, N> w = LoadPack<ElemT, N>(w_row + c * N);
          if constexpr (kAdagrad) {
            float* s_at = state + RowElems(r[0], width) + c * N;
            StatePack<N> s = StatePack<N>::Load(s_at);
            StorePack<ElemT, N>(w_row + c * N, AdagradStep(w, g, s, lr, eps));
            s.Store(s_at);
          } else {
            StorePack<ElemT, N>(w_row + c * N, ScaledStep(w, g, step));
          }
        }
      } else {
        Pack<ElemT, N> g[kEntries][kSlices], w[kEntries][kSlices];
        StatePack<N> s[kAdagrad ? kEntries : 1][kAdagrad ? kSlices : 1];
        bool has[kEntries][kSlices];
        float row_state[kEntries];
#pragma unroll
        for (int u = 0; u < kEntries; ++u) {
          if constexpr (kRowwise) row_state[u] = live[u] ? state[r[u]] : 0.f;
#pragma unroll
          for (int c = 0; c < kSlices; ++c) {
            const int col = (lane + c * group) * N;
            has[u][c] = live[u] && lane + c * group < lanes_per_row;
            if (has[u][c]) {
              g[u][c] = LoadPackStreaming<ElemT, N>(RowPtr(rows, base + k + u * stride, width) + col);
              w[u][c] = LoadPack<ElemT, N>(RowPtr(table, r[u], width) + col);
              if constexpr (kAdagrad) s[u][c] = StatePack<N>::Load(state + RowElems(r[u], width) + col);
            }
          }
        }
#pragma unroll
        for (int u = 0; u < kEntries; ++u) {
          float step = lr;
          if constexpr (kRowwise) {
            // (a group whose second entry is past the count still takes part in the butterfly: its lanes are active)
            float sum = 0.f;
#pragma unroll
            for (int c = 0; c < kSlices; ++c)
              if (has[u][c]) sum = AddSquares(sum, g[u][c]);
            sum = GroupSum(sum, group);
            if (live[u]) step = RowwiseStep(state + r[u], row_state[u], sum, width, lane == 0, lr, eps);
          }
#pragma unroll
          for (int c = 0; c < kSlices; ++c) {
            if (!has[u][c]) continue;
            const int col = (lane + c * group) * N;
            ElemT* w_at = const_cast<ElemT*>(RowPtr(table, r[u], width)) + col;
            if constexpr (kAdagrad) {
              StorePack<ElemT, N>(w_at, AdagradStep(w[u][c], g[u][c], s[u][c], lr, eps));
              s[u][c].Store(state + RowElems(r[u], width) + col);
            } else {
              StorePack<ElemT, N>(w_at, ScaledStep(w[u][c], g[u][c], step));
            }
          }
        }
      }
    }
  }
}

}  // namespace detail
}  // namespace cuembed

#endif  // CUEMBED_INCLUDE_SPARSE_UPDATE_KERNELS_HPP_
