// MI355X (gfx950 / CDNA4) gather-reduce kernels for a GROUP of tables of one width and one element type, pooled in one
// launch (an extension: the reference lists "multiple tables" under future work).
//
// The bags of T tables lie one table after the other: bag g = t * B + b belongs to table t and sample b (B =
// batch_per_table, the table-major order of FBGEMM's table-batched op).  That is the single-table problem with batch
// T * B in which two things depend on the bag:
//   * which table base a lane reads from:  tables[g / B];
//   * where the pooled row is stored:      out[b, t, :] of a contiguous [B, T, W] -- what torch.stack(per_table, dim=1)
//     builds from T single-table calls.
// The sample walk (WalkSample), the row pools (RowPool::Gather, QuantizedRowPool::Gather), the arithmetic and its order
// are the single-table kernels' own, so the result has the bits of T single-table calls.
//
//   GatherReduceGroupedKernel            GatherReduceKernel on a group (fp32 accumulation, column slices = 1)
//   GatherReduceQuantizedGroupedKernel   GatherReduceQuantizedKernel on a group of fused 8-bit tables
//
// The table base is a PER-LANE value: B need not be a multiple of the samples of a wavefront or a workgroup, so
// neighbouring lane groups of one wavefront may sit in different tables.  It costs one 32-bit unsigned division and one
// 8-byte load per thread, in a prologue in front of the walk (GroupedBag::OfThread): the bag of a thread is fixed by its
// grid position and sample_order alone, so the load of tables[t] is issued BEFORE the walk's staging loads and barrier
// (kLdsStaged) or its offset loads (CSR) and is in flight with them -- in a call without sample_order, no round trip of
// its own in front of the first row load (with sample_order the walk reads sample_order[p] a second time and waits for
// it in front of the offset loads: one more round trip, a cache hit, than the single-table kernel has).  The walk
// arrives at the same bag (`sample`); the prologue's table and sample also give the output row (one division per thread
// in all).
// A pointer read from memory is a generic pointer to the compiler: the lane base is kept in a global-memory pointer type
// (GlobalPtr) so that the row loads are global_load as in the single-table kernels, not flat_load (which also counts
// against the LDS counter).
#ifndef CUEMBED_INCLUDE_GROUPED_GATHER_KERNELS_HPP_
#define CUEMBED_INCLUDE_GROUPED_GATHER_KERNELS_HPP_

#include <cstdint>
#include <type_traits>

#include "cuembed/include/gather_reduce_kernels.hpp"
#include "cuembed/include/quantized_rows_kernels.hpp"

namespace cuembed {
namespace detail {

//! Bag g = table * batch_per_table + sample of a group (g < num_tables * batch_per_table <= INT_MAX).
struct GroupedBag {
  uint32_t table;
  uint32_t sample;
  static __device__ __forceinline__ GroupedBag Of(const int64_t bag, const int batch_per_table) {
    GroupedBag g;
    const uint32_t per_table = static_cast<uint32_t>(batch_per_table);
    g.table = static_cast<uint32_t>(bag) / per_table;
    g.sample = static_cast<uint32_t>(bag) - g.table * per_table;
    return g;
  }
  //! The bag WalkSample will hand to the thread at slot threadIdx.y of workgroup blockIdx.x (column slices 1): grid
  //! position p pools bag p, or sample_order[p] in the walks that honour it (all but kLdsStaged).  A thread without a bag
  //! (p >= batch) gets bag 0: it loads a valid table pointer and leaves the walk before using it.
  template <IndexSource kSource>
  static __device__ __forceinline__ GroupedBag OfThread(const int batch, const int batch_per_table,
                                                        const int32_t* __restrict__ sample_order) {
    int64_t bag = static_cast<int64_t>(blockIdx.x) * blockDim.y + threadIdx.y;
    if (bag >= batch) bag = 0;
    else if (kSource != IndexSource::kLdsStaged && sample_order != nullptr) bag = sample_order[bag];
    return Of(bag, batch_per_table);
  }
  //! Row of the bag in out[B, T, :] (< T * B <= INT_MAX: ONE register to keep through the walk, not table and sample).
  __device__ __forceinline__ uint32_t OutputRow(const int num_tables) const {
    return sample * static_cast<uint32_t>(num_tables) + table;
  }
};

//! A pointer into GLOBAL memory, typed as one (see the head of this file).
template <typename T>
using GlobalPtr = const T __attribute__((address_space(1))) *;

// ---------------------------------------------------------------------------
// Occupancy the grouped kernels are asked to hold (amdgpu_waves_per_eu): that of the corresponding single-table
// instantiation.  The grouped kernels run the single-table kernels' code with one or two more live registers; without
// the hint, where that crosses an occupancy step the scheduler gives the step up and orders the consume phase of
// Gather for parallelism (68 -> 106 VGPRs in the worst case); with it, it keeps the row-by-row order and the step.
// The tables hold waves per SIMD of GatherReduceKernel (AccT = float) / GatherReduceQuantizedKernel, one digit per
// instantiation in the order [element][IndexT 32/64][OffsetT 32/64][N: widest first][weighted][IndexSource]; they are
// written by `tools/grouped_forward_resources.py --tables`; its report checks the result (scratch, spills, occupancy
// against the counterpart): regenerate them when the single-table kernels or the compiler change.
// SIX digits are lower than the single-table kernel's: weighted cross-lane kernels with int32 offsets (plain: fp32
// int64 ids 16-byte lanes, fp16 int32 ids and bf16 int32 / int64 ids 8-byte lanes; 8-bit: fp32 out int64 ids and fp16 out
// int32 ids, 4 codes per lane).  Held to the single-table step they spill 2-4 VGPRs (12-20 bytes of scratch per lane);
// one step lower they need none (the 8-bit fp32-out one: two steps lower).  No scratch comes first: those six sit below
// their counterparts, five by one wave per SIMD and one by two.
// ---------------------------------------------------------------------------
constexpr char kSingleTableWaves[] =
    "888867888878888888888867888878888888888867888878888888888867888878888888"
    "755544888767888788755544888767888788745544888867888878745544888867888878"
    "757544888767888788757544888767888788756544888867888878756544888867888878";
constexpr char kSingleTableWavesQuantized[] =
    "745535867756888877745535867756888877646535868746888857646535868746878857"
    "745535867754888755745535867744888745646534868744888855646534868744878845";

constexpr int WavesIndex(const int elem, const bool index64, const bool offset64, const int n_step, const bool weighted,
                         const IndexSource source) {
  return ((((elem * 2 + (index64 ? 1 : 0)) * 2 + (offset64 ? 1 : 0)) * 3 + n_step) * 2 + (weighted ? 1 : 0)) * 3 +
         static_cast<int>(source);
}
template <typename ElemT, typename IndexT, typename OffsetT, int N, bool kWeighted, IndexSource kSource>
constexpr int GroupedWaves() {
  constexpr int kMaxN = 16 / static_cast<int>(sizeof(ElemT));
  static_assert(N == kMaxN || N == kMaxN / 2 || N == kMaxN / 4, "lanes of 16, 8 or 4 bytes");
  constexpr int elem = std::is_same<ElemT, float>::value ? 0 : (std::is_same<ElemT, _Float16>::value ? 1 : 2);
  return kSingleTableWaves[WavesIndex(elem, sizeof(IndexT) == 8, sizeof(OffsetT) == 8,
                                      N == kMaxN ? 0 : (N == kMaxN / 2 ? 1 : 2), kWeighted, kSource)] - '0';
}
template <typename OutT, typename IndexT, typename OffsetT, int N, bool kWeighted, IndexSource kSource>
constexpr int GroupedQuantizedWaves() {
  static_assert(N == 16 || N == 8 || N == 4, "16, 8 or 4 codes per lane");
  return kSingleTableWavesQuantized[WavesIndex(std::is_same<OutT, float>::value ? 0 : 1, sizeof(IndexT) == 8,
                                               sizeof(OffsetT) == 8, N == 16 ? 0 : (N == 8 ? 1 : 2), kWeighted, kSource)] - '0';
}

// ---------------------------------------------------------------------------
// Sum / mean on a group of tables.
//   block = (lanes_per_row, samples_per_block); grid = ceil(T * B / samples_per_block)
//   dynamic LDS (kLdsStaged only) = samples_per_block * num_hots * (sizeof(IndexT) [+ sizeof(ElemT) if weighted]):
//   the workgroup's staged indices are contiguous across a table boundary in the [T, B, H] layout
// ---------------------------------------------------------------------------
template <typename ElemT,    // table / output element
          typename IndexT,   // int32_t / int64_t
          typename OffsetT,  // CSR offset type (unused for kLdsStaged)
          int N,             // elements per lane
          bool kWeighted,
          IndexSource kSource,
          int kUnroll = kForwardUnroll,
          bool kPipelined = kForwardPipelined,
          int kBlockThreads = kMaxBlockThreads>
__global__ void __launch_bounds__(kBlockThreads)
__attribute__((amdgpu_waves_per_eu(GroupedWaves<ElemT, IndexT, OffsetT, N, kWeighted, kSource>())))
GatherReduceGroupedKernel(const ElemT* const* __restrict__ tables,   // [num_tables] table bases, in device memory
                          const int batch_per_table,                 // B
                          const int num_tables,                      // T
                          const int width,
                          const int batch,                           // T * B
                          const IndexT* __restrict__ indices,
                          const OffsetT* __restrict__ offsets,       // [T * B + 1], null => fixed hotness
                          const int num_hots,
                          const ElemT* __restrict__ weights,
                          const bool is_mean,
                          ElemT* __restrict__ out,                   // [B, T, width]
                          const bool stream_rows,                    // RowLoadPolicy::kStreaming, one value for the group
                          const int32_t* __restrict__ sample_order) {  // a permutation of the T * B bags (CSR only), or null
  const int64_t column0 = static_cast<int64_t>(threadIdx.x) * N;
  RowPool<ElemT, float, N, kWeighted> pool;
  int64_t sample;
  int hot;
  const GroupedBag bag = GroupedBag::OfThread<kSource>(batch, batch_per_table, sample_order);
  // this lane's columns of row 0 of the bag's table: requested here, in front of the walk's own loads
  const GlobalPtr<ElemT> lane_base = (GlobalPtr<ElemT>)tables[bag.table] + column0;
  const uint32_t out_row = bag.OutputRow(num_tables);   // (bag == the walk's `sample`)
  const auto gather = [&](const int count, const auto index_at, const auto weight_at) {
    const ElemT* base = (const ElemT*)lane_base;
    if (stream_rows) pool.template Gather<kUnroll, kPipelined, true>(base, width, count, index_at, weight_at);
    else pool.template Gather<kUnroll, kPipelined, false>(base, width, count, index_at, weight_at);
  };
  if (!WalkSample<kSource, kWeighted>(blockIdx.x, batch, indices, offsets, num_hots, weights, sample_order, sample, hot,
                                      gather))
    return;
  const int64_t row = out_row;
  FinishPooledRow<ElemT, float, N, kWeighted>(pool, hot, is_mean, out + row * width + column0);
}

// ---------------------------------------------------------------------------
// Sum / mean on a group of fused 8-bit tables (same block, grid and LDS; weights in the output's type).
// ---------------------------------------------------------------------------
template <typename OutT,     // output and weight element: float or _Float16
          typename IndexT,
          typename OffsetT,
          int N,             // codes per lane: 16, 8 or 4
          bool kWeighted,
          IndexSource kSource,
          int kUnroll = (N == 16 ? 4 : kForwardUnroll)>
__global__ void __launch_bounds__(N == 16 ? kQuantizedWideLaneThreads : kMaxBlockThreads)
__attribute__((amdgpu_waves_per_eu(GroupedQuantizedWaves<OutT, IndexT, OffsetT, N, kWeighted, kSource>())))
GatherReduceQuantizedGroupedKernel(const uint8_t* const* __restrict__ tables,   // [num_tables], in device memory
                                   const int batch_per_table,
                                   const int num_tables,
                                   const int width,
                                   const int batch,                             // T * B
                                   const IndexT* __restrict__ indices,
                                   const OffsetT* __restrict__ offsets,         // [T * B + 1], null => fixed hotness
                                   const int num_hots,
                                   const OutT* __restrict__ weights,
                                   const bool is_mean,
                                   OutT* __restrict__ out,                      // [B, T, width]
                                   const bool stream_rows,
                                   const int32_t* __restrict__ sample_order) {
  using A = Arith<float>;
  const int lane_x = threadIdx.x;
  const int row_bytes = width + kQuantizedTrailerBytes;
  const int64_t trailer_delta = width - lane_x * N;
  QuantizedRowPool<OutT, N, kWeighted> pool;
  int64_t sample;
  int hot;
  const GroupedBag bag = GroupedBag::OfThread<kSource>(batch, batch_per_table, sample_order);
  // this lane's first code of row 0 of the bag's table: requested here, in front of the walk's own loads
  const GlobalPtr<uint8_t> lane_base = (GlobalPtr<uint8_t>)tables[bag.table] + lane_x * N;
  const uint32_t out_row = bag.OutputRow(num_tables);   // (bag == the walk's `sample`)
  const auto gather = [&](const int count, const auto index_at, const auto weight_at) {
    const uint8_t* base = (const uint8_t*)lane_base;
    if (stream_rows) pool.template Gather<kUnroll, true>(base, trailer_delta, row_bytes, count, index_at, weight_at);
    else pool.template Gather<kUnroll, false>(base, trailer_delta, row_bytes, count, index_at, weight_at);
  };
  if (!WalkSample<kSource, kWeighted>(blockIdx.x, batch, indices, offsets, num_hots, weights, sample_order, sample, hot,
                                      gather))
    return;

  // ---- epilogue of GatherReduceQuantizedKernel: the bag's bias once, mean scaling (MeanFactor), one rounding to OutT ----
  const float inv = is_mean ? MeanFactor<kWeighted>(pool.weight_sum, hot) : 1.f;
  float v[N];
#pragma unroll
  for (int e = 0; e < N; ++e) {
    v[e] = A::add(pool.acc[e], pool.bias_sum);
    if (is_mean) v[e] = A::mul(v[e], inv);
  }
  const int64_t row = out_row;
  StoreWideStreaming<OutT, N>(out + row * static_cast<int64_t>(width) + lane_x * N, v);
}

}  // namespace detail
}  // namespace cuembed

#endif  // CUEMBED_INCLUDE_GROUPED_GATHER_KERNELS_HPP_
