// MI355X (gfx950 / CDNA4) kernels that TRAIN a group of tables beyond sum pooling with table gradients only (an
// extension; the group is that of grouped_gather_kernels.hpp: bag g = t * B + b, results [B, T, W]):
//
//   WeightGradGroupedKernel   the gradient of a weighted sum-forward with respect to the per-lookup weights:
//                             grad_w[p] = ElemT( fp32 < tables[t][indices[p], :], grad_y[b, t, :] > )
//   GroupedMeanScaleKernel    grad_y of a mean-pooled group -> grad_y of the equivalent sum-pooled one:
//                             out[b, t, :] = ElemT( float(grad_y[b, t, :]) * MeanFactor(bag t * B + b) )
//
// WeightGradGroupedKernel is WeightGradKernel (gather_reduce_kernels.hpp) on a group: behind a prologue that finds the
// bag, the work of a lane group is the single-table kernel's own text -- the software-pipelined 8-lookup batches with
// the transposing butterfly where a row fits one pass of the lane group, the strided walk otherwise -- so a lookup's
// dot product is summed in the same order and has the same bits.  (A second kernel, not a shared body: routed through
// one inlined function, 20 of WeightGradKernel's 36 instantiations took 2-4 more registers; as it is they are
// untouched.  A change to either walk belongs in both.)  Two things depend on the bag: the table base, tables[g / B],
// and the gradient row, b * T + t (GroupedBag::Of / OutputRow).  The base is read from memory and kept in a
// GlobalPtr, so that the row loads stay global_load.
//
// GroupedMeanScaleKernel is a streaming kernel: one lane group per row of grad_y finds its bag, computes the bag's mean
// factor itself (unweighted: 1 / length; weighted: 1 / the fp32 sum of the bag's weights, each lane a strided part of
// it, folded by a butterfly; 0 when the denominator is 0) and moves the row through registers in 16-, 8- or 4-byte
// lanes with one fp32 multiply and one rounding per element.  No second pass, no scratch buffer; out may alias grad_y
// (a lane reads a pack before it writes the same pack, and no other lane touches it).
//
// Every address is formed in 64 bits (WidenIndex, RowPtr's arithmetic in GlobalRowPtr, int64_t begin), as in the
// single-table kernels.
#ifndef CUEMBED_INCLUDE_GROUPED_TRAIN_KERNELS_HPP_
#define CUEMBED_INCLUDE_GROUPED_TRAIN_KERNELS_HPP_

#include <cstdint>

#include "cuembed/include/gather_reduce_kernels.hpp"
#include "cuembed/include/grouped_gather_kernels.hpp"

namespace cuembed {
namespace detail {

//! RowPtr on a base in global memory: the address is formed in the global address space and only then handed on as a
//! plain pointer, which the compiler then knows to be global (a GlobalPtr cast straight back to a plain pointer is
//! folded away together with what it says).
template <typename ElemT>
__device__ __forceinline__ const ElemT* GlobalRowPtr(const GlobalPtr<ElemT> base, const int64_t r, const int width) {
  const int64_t row_bytes = static_cast<int64_t>(static_cast<uint32_t>(width) * static_cast<uint32_t>(sizeof(ElemT)));
  return (const ElemT*)(GlobalPtr<ElemT>)((GlobalPtr<char>)base + r * row_bytes);
}

// ---------------------------------------------------------------------------
// Weight gradient of a group.
//   block = (group, bags_per_block), group a power of two <= 64; grid = ceil(T * B / bags_per_block)
// ---------------------------------------------------------------------------
template <typename ElemT, typename IndexT, typename OffsetT, int N>
__global__ void __launch_bounds__(kMaxBlockThreads)
WeightGradGroupedKernel(const ElemT* const* __restrict__ tables,   // [num_tables] table bases, in device memory
                        const int batch_per_table,                 // B
                        const int num_tables,                      // T
                        const int width,
                        const int batch,                           // T * B
                        const IndexT* __restrict__ indices,
                        const OffsetT* __restrict__ offsets,       // [T * B + 1], null => fixed hotness
                        const int num_hots,
                        const ElemT* __restrict__ grad_y,          // [B, T, width]
                        ElemT* __restrict__ grad_w) {              // the layout of indices
  const int64_t bag_id = static_cast<int64_t>(blockIdx.x) * blockDim.y + threadIdx.y;
  if (bag_id >= batch) return;
  const GroupedBag bag = GroupedBag::Of(bag_id, batch_per_table);
  // requested in front of the offset loads: in flight with them
  const GlobalPtr<ElemT> table = (GlobalPtr<ElemT>)tables[bag.table];
  int64_t begin;
  int hot = num_hots;
  if (offsets != nullptr) {
    begin = static_cast<int64_t>(offsets[bag_id]);
    hot = static_cast<int>(static_cast<int64_t>(offsets[bag_id + 1]) - begin);
  } else {
    begin = bag_id * num_hots;
  }
  const int64_t gy_row = bag.OutputRow(num_tables);
  const int lane_x = threadIdx.x;
  const int group = blockDim.x;
  const IndexT* my_idx = indices + begin;
  ElemT* my_out = grad_w + begin;
  const ElemT* my_gy = grad_y + gy_row * width;
  // ---- from here on: WeightGradKernel's text, its row addresses formed on the GlobalPtr (GlobalRowPtr for RowPtr) ----
  const int chunks = width / N;  // N-element slices per row

  static_assert(kForwardUnroll == 8, "the transposing reduction below is written for 8 partial dots");
  if (chunks <= group && group >= 8) {
    // ---- a row fits one pass of the group (every shape up to 64 lanes x 16 B) ----
    // Software-pipelined: the rows of batch k+1 (and the row ids of batch k+2) are requested
    // BEFORE the cross-lane reduction of batch k, so loads are in flight during the ~15 dependent
    // cross-lane steps and a row request never waits for its own id.
    // The 8 partial dots are folded with a transposing butterfly: each exchange step halves the
    // number of values a lane still carries (4 + 2 + 1 exchanges leave lane l with the sum, over
    // its 8-lane subgroup, of lookup l & 7), then log2(group / 8) plain steps finish it --
    // 7..10 cross-lane operations per 8 lookups instead of 8 x log2(group).
    const bool has_column = lane_x < chunks;
    Pack<ElemT, N> g;
    if (has_column) g = LoadPack<ElemT, N>(my_gy + static_cast<int64_t>(lane_x) * N);
    const GlobalPtr<ElemT> lane_base = table + static_cast<int64_t>(lane_x) * N;
    Pack<ElemT, N> row[kForwardUnroll];
    IndexT ahead[kForwardUnroll];  // row ids of the batch AFTER the one whose rows are in flight
    // full batches take the branch-free path; only the last, partial batch is predicated
    auto request_ids = [&](const int j0) {
      if (j0 + kForwardUnroll <= hot) {
#pragma unroll
        for (int u = 0; u < kForwardUnroll; ++u) ahead[u] = my_idx[j0 + u];
      } else {
#pragma unroll
        for (int u = 0; u < kForwardUnroll; ++u)
          if (j0 + u < hot) ahead[u] = my_idx[j0 + u];
      }
    };
    auto request_rows = [&](const int j0) {  // consumes `ahead`
      if (!has_column) return;
      if (j0 + kForwardUnroll <= hot) {
#pragma unroll
        for (int u = 0; u < kForwardUnroll; ++u)
          row[u] = LoadPack<ElemT, N>(GlobalRowPtr<ElemT>(lane_base, WidenIndex(ahead[u]), width));
      } else {
#pragma unroll
        for (int u = 0; u < kForwardUnroll; ++u)
          if (j0 + u < hot) row[u] = LoadPack<ElemT, N>(GlobalRowPtr<ElemT>(lane_base, WidenIndex(ahead[u]), width));
      }
    };
    request_ids(0);
    request_rows(0);
    request_ids(kForwardUnroll);
    for (int j0 = 0; j0 < hot; j0 += kForwardUnroll) {
      float dot[kForwardUnroll];
      if (j0 + kForwardUnroll <= hot) {
#pragma unroll
        for (int u = 0; u < kForwardUnroll; ++u) dot[u] = has_column ? DotPack<ElemT, N>(row[u], g, 0.f) : 0.f;
      } else {
#pragma unroll
        for (int u = 0; u < kForwardUnroll; ++u)
          dot[u] = (j0 + u < hot && has_column) ? DotPack<ElemT, N>(row[u], g, 0.f) : 0.f;
      }
      __builtin_amdgcn_sched_barrier(0);
      request_rows(j0 + kForwardUnroll);
      request_ids(j0 + 2 * kForwardUnroll);
      __builtin_amdgcn_sched_barrier(0);
      float four[4], two[2];
#pragma unroll
      for (int k = 0; k < 4; ++k) {  // exchange with lane ^ 1: keep the even or the odd lookup of a pair
        const bool odd = lane_x & 1;
        const float got = __shfl_xor(odd ? dot[2 * k] : dot[2 * k + 1], 1, group);
        four[k] = (odd ? dot[2 * k + 1] : dot[2 * k]) + got;
      }
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const bool odd = lane_x & 2;
        const float got = __shfl_xor(odd ? four[2 * k] : four[2 * k + 1], 2, group);
        two[k] = (odd ? four[2 * k + 1] : four[2 * k]) + got;
      }
      float one;
      {
        const bool odd = lane_x & 4;
        const float got = __shfl_xor(odd ? two[0] : two[1], 4, group);
        one = (odd ? two[1] : two[0]) + got;
      }
      for (int d = 8; d < group; d <<= 1) one += __shfl_xor(one, d, group);
      // lane l < 8 now holds lookup j0 + l: one coalesced store per batch
      if (lane_x < kForwardUnroll && j0 + lane_x < hot) my_out[j0 + lane_x] = static_cast<ElemT>(one);
    }
    return;
  }

  for (int j0 = 0; j0 < hot; j0 += kForwardUnroll) {
    const int nb = hot - j0 < kForwardUnroll ? hot - j0 : kForwardUnroll;
    float dot[kForwardUnroll];
#pragma unroll
    for (int u = 0; u < kForwardUnroll; ++u) dot[u] = 0.f;
    for (int c = lane_x; c < chunks; c += group) {
      const Pack<ElemT, N> g = LoadPack<ElemT, N>(my_gy + static_cast<int64_t>(c) * N);
      Pack<ElemT, N> row[kForwardUnroll];
#pragma unroll
      for (int u = 0; u < kForwardUnroll; ++u) {
        if (u < nb)
          row[u] = LoadPack<ElemT, N>((const ElemT*)(table + RowElems(WidenIndex(my_idx[j0 + u]), width) +
                                                     static_cast<int64_t>(c) * N));
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < kForwardUnroll; ++u) {
        if (u < nb) dot[u] = DotPack<ElemT, N>(row[u], g, dot[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < kForwardUnroll; ++u) {
      for (int d = group >> 1; d > 0; d >>= 1) dot[u] += __shfl_xor(dot[u], d, group);
    }
    if (lane_x == 0) {
#pragma unroll
      for (int u = 0; u < kForwardUnroll; ++u)
        if (u < nb) my_out[j0 + u] = static_cast<ElemT>(dot[u]);
    }
  }
}

// ---------------------------------------------------------------------------
// Mean scaling of a group's grad_y.
//   block = (group, rows_per_block), group a power of two <= 64; grid = ceil(B * T / rows_per_block)
//   rows = B * T rows of grad_y; row r = b * T + t belongs to bag t * B + b
// ---------------------------------------------------------------------------
template <typename ElemT, typename OffsetT, int N, bool kWeighted>
__global__ void __launch_bounds__(kMaxBlockThreads)
GroupedMeanScaleKernel(const ElemT* grad_y,                        // [B, T, width]  (may be `out`)
                       const OffsetT* __restrict__ offsets,        // [T * B + 1], null => fixed hotness
                       const ElemT* __restrict__ weights,          // the layout of the indices (kWeighted)
                       const int batch_per_table,                  // B
                       const int num_tables,                       // T
                       const int width,
                       const int rows,                             // B * T
                       const int num_hots,
                       ElemT* out) {                               // [B, T, width]
  const int lane_x = threadIdx.x;
  const int group = blockDim.x;
  const int64_t row = static_cast<int64_t>(blockIdx.x) * blockDim.y + threadIdx.y;
  if (row >= rows) return;
  const uint32_t sample = static_cast<uint32_t>(row) / static_cast<uint32_t>(num_tables);
  const uint32_t table = static_cast<uint32_t>(row) - sample * static_cast<uint32_t>(num_tables);
  const int64_t bag = static_cast<int64_t>(table) * batch_per_table + sample;
  int64_t begin;
  int hot = num_hots;
  if (offsets != nullptr) {
    begin = static_cast<int64_t>(offsets[bag]);
    hot = static_cast<int>(static_cast<int64_t>(offsets[bag + 1]) - begin);
  } else {
    begin = bag * num_hots;
  }
  float weight_sum = 0.f;
  if constexpr (kWeighted) {
    const ElemT* my_w = weights + begin;
    for (int j = lane_x; j < hot; j += group) weight_sum += static_cast<float>(my_w[j]);
    // (a + b in both lanes of a pair: every lane of the group ends with the same bits)
    for (int d = group >> 1; d > 0; d >>= 1) weight_sum += __shfl_xor(weight_sum, d, group);
  }
  const float factor = MeanFactor<kWeighted>(weight_sum, hot);
  const int chunks = width / N;
  const ElemT* src = grad_y + row * width;
  ElemT* dst = out + row * width;
  for (int c = lane_x; c < chunks; c += group) {
    const Pack<ElemT, N> v = LoadPackStreaming<ElemT, N>(src + static_cast<int64_t>(c) * N);
    Pack<ElemT, N> r;
#pragma unroll
    for (int e = 0; e < N; ++e) r.v[e] = static_cast<ElemT>(static_cast<float>(v.v[e]) * factor);
    StorePack<ElemT, N>(dst + static_cast<int64_t>(c) * N, r);   // (read next, by the scatter-add: not streamed past L2)
  }
}

}  // namespace detail
}  // namespace cuembed

#endif  // CUEMBED_INCLUDE_GROUPED_TRAIN_KERNELS_HPP_
