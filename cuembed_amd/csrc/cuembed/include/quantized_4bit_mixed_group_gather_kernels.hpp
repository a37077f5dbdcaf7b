// MI355X (gfx950 / CDNA4) gather-reduce kernel for a group of fused 4-bit row-wise tables of DIFFERENT widths, pooled in
// one launch (an extension: the reference has neither quantized tables nor groups).  The sibling of
// GatherReduceQuantizedMixedGroupKernel (quantized_mixed_group_gather_kernels.hpp, 8-bit rows, which stays as it is) on
// the rows of quantized_4bit_rows_kernels.hpp.
//
// Layout: the input is the mixed group's -- bag g = t * B + b belongs to table t and sample b; CSR has one indices[nnz],
// one offsets[T * B + 1] and optional weights[nnz]; fixed hotness has indices [T, B, H].  Table t is fused rows
// [rows_t, W_t / 2 + 4] of bytes: W_t / 2 bytes of codes (element 2i in the low nibble of byte i), the row's fp16 scale,
// its fp16 bias; W_t % 8 == 0.  The result is out[B, D] of OutT (float or _Float16; the weights have that type too), D =
// sum W_t: bag (t, b) at columns [c_t, c_t + W_t) of row b -- torch.cat of T single-table 4-bit results on dim 1.
//
// The work split is the mixed group's: a 256-thread workgroup serves bags of ONE table, which takes L_t = min(W_t / N,
// 256) lanes per bag and 256 / L_t bags per workgroup; the table follows from blockIdx.x by MixedGroupTableOfBlock, so
// the descriptor entry (MixedGroupEntry as it is, lanes counted in lanes of N codes), the table base (a
// GlobalPtr<uint8_t>), the width, the row pitch W_t / 2 + 4, the lane count and the column base are scalar values.
//
// N, the codes of one lane, is one value for the launch: 32, 16 or 8, the largest that divides every W_t
// (Quantized4BitMixedGroupCodesPerLane, quantized_4bit_mixed_group_lookup.hpp).  A lane's codes are N / 2 bytes in ONE
// load (global_load_dwordx4 / dwordx2 / dword) at a 4-byte aligned address: the row pitch promises no more than that, the
// hardware asks no more, so alignment never narrows N -- every base must be 4-byte aligned and that is all.  out is
// 16-byte aligned (asserted on the host) and every c_t and D are multiples of N, so out + b * D + c_t + column is a
// multiple of N elements >= 16 bytes: StoreWideStreaming<OutT, N> is always aligned.  The 256-thread workgroup is what the
// 32-code pool needs anyway (89 - 166 registers in the single-table kernel: kQuantized4BitWideLaneThreads).
//
// Per lookup a lane forms RowPtr(lane_base, id, W_t / 2 + 4) and reads the trailer dword trailer_delta = W_t / 2 -
// column / 2 bytes behind its codes (Quantized4BitRowPool::Gather as it is: mask-and-shift unpack into
// v_cvt_f32_ubyte0..3, even / odd accumulators, Quantized4BitUnroll<N>() lookups in flight).  A row of more than 256
// lanes (W > 256 * N: 2,056 at N = 8, 8,224 at N = 32) takes the column loop: every pass has its own pool, re-reads the
// row's trailer (4 bytes that all lanes of the row share) and has its own trailer_delta -- so the group serves widths at
// N = 32 that the single-table call narrows to 16.  The walks are the mixed group's: fixed hotness staged through LDS, CSR
// by cross-lane reads when L_t divides 64 (the next chunk of indices in flight while the current one is pooled),
// broadcast reads otherwise.  The epilogue is the single-table kernel's: even / odd back into element order, bias_sum
// once, MeanFactor, one rounding to OutT, a streaming store.  fp32 accumulation per element in lookup order: the bits of
// T calls of GatherReduceQuantized4BitKernel, whatever N they and this launch take.
#ifndef CUEMBED_INCLUDE_QUANTIZED_4BIT_MIXED_GROUP_GATHER_KERNELS_HPP_
#define CUEMBED_INCLUDE_QUANTIZED_4BIT_MIXED_GROUP_GATHER_KERNELS_HPP_

#include <cstdint>

#include "cuembed/include/mixed_group_gather_kernels.hpp"
#include "cuembed/include/quantized_4bit_rows_kernels.hpp"

namespace cuembed {
namespace detail {

// ---------------------------------------------------------------------------
// Sum / mean on a group of fused 4-bit tables of mixed widths.
//   block = kMixedGroupBlockThreads (1-D); grid = descriptor[num_tables].first_block
//   dynamic LDS (kStaged only) = max_t(spb_t) * num_hots * (sizeof(IndexT) [+ sizeof(OutT) if weighted])
// ---------------------------------------------------------------------------
template <typename OutT,     // output and weight element: float or _Float16
          typename IndexT,   // int32_t / int64_t
          typename OffsetT,  // CSR offset type (unused when offsets == nullptr)
          int N,             // codes per lane, one value for the launch: 32, 16 or 8
          bool kWeighted,
          bool kStaged>      // fixed hotness, the workgroup's indices staged in LDS
__global__ void __launch_bounds__(kMixedGroupBlockThreads)
GatherReduceQuantized4BitMixedGroupKernel(const uint8_t* const* __restrict__ tables,       // [num_tables] bases, device memory
                                          const MixedGroupEntry* __restrict__ descriptor,  // [num_tables + 1], device memory
                                          const int num_tables,
                                          const int batch_per_table,                        // B
                                          const IndexT* __restrict__ indices,
                                          const OffsetT* __restrict__ offsets,              // [T * B + 1], null => fixed hotness
                                          const int num_hots,
                                          const OutT* __restrict__ weights,
                                          const bool is_mean,
                                          OutT* __restrict__ out,                           // [B, out_width]
                                          const int out_width,                              // D
                                          const bool stream_rows) {                         // RowLoadPolicy::kStreaming
  using A = Arith<float>;
  constexpr int kUnroll = Quantized4BitUnroll<N>();
  constexpr int kLaneBytes = N / 2;
  static_assert(kMixedGroupBlockThreads <= kQuantized4BitWideLaneThreads, "the 32-code pool's register budget");
  // ---- the workgroup's table: scalar values ----
  const int table = MixedGroupTableOfBlock(descriptor, num_tables, static_cast<int>(blockIdx.x));
  const MixedGroupEntry entry = descriptor[table];
  const GlobalPtr<uint8_t> table_base = (GlobalPtr<uint8_t>)tables[table];
  const int width = entry.width;
  const int code_bytes = CodeBytes4Bit(width);
  const int row_bytes = code_bytes + kQuantized4BitTrailerBytes;
  const int lanes = entry.lanes;
  const int row_lanes = width / N;                                   // > lanes only for rows wider than the workgroup
  const int slots = static_cast<int>(blockDim.x) / lanes;            // spb_t
  const int64_t first_sample = static_cast<int64_t>(static_cast<int>(blockIdx.x) - entry.first_block) * slots;
  // ---- the thread's bag ----
  const int tid = threadIdx.x;
  const int slot = static_cast<int>(static_cast<uint32_t>(tid) / static_cast<uint32_t>(lanes));
  const int lane = tid - slot * lanes;
  const int64_t sample = first_sample + slot;
  const bool has_bag = slot < slots && sample < batch_per_table;
  const int64_t bag = static_cast<int64_t>(table) * batch_per_table + sample;

  const IndexT* my_idx;
  const OutT* my_w;
  int hot = num_hots;
  if constexpr (kStaged) {
    // ---- fixed hotness: the indices (+ weights) of the workgroup's bags, contiguous in [T, B, H], go through LDS once ----
    extern __shared__ __attribute__((aligned(16))) unsigned char quantized_4bit_mixed_lds_raw[];
    IndexT* stage_idx = reinterpret_cast<IndexT*>(quantized_4bit_mixed_lds_raw);
    OutT* stage_w = reinterpret_cast<OutT*>(stage_idx + slots * num_hots);
    const int64_t left = batch_per_table - first_sample;             // >= 1: the workgroup has at least one bag
    const int bags = static_cast<int>(left < slots ? left : slots);
    const int64_t first = (static_cast<int64_t>(table) * batch_per_table + first_sample) * num_hots;
    const int count = bags * num_hots;
    for (int i = tid; i < count; i += static_cast<int>(blockDim.x)) {
      stage_idx[i] = indices[first + i];
      if constexpr (kWeighted) stage_w[i] = weights[first + i];
    }
    __syncthreads();
    if (!has_bag) return;
    my_idx = stage_idx + slot * num_hots;
    my_w = stage_w + slot * num_hots;
  } else {
    if (!has_bag) return;
    int64_t begin;
    if (offsets != nullptr) {
      begin = static_cast<int64_t>(offsets[bag]);
      hot = static_cast<int>(static_cast<int64_t>(offsets[bag + 1]) - begin);
    } else {
      begin = bag * num_hots;
    }
    my_idx = indices + begin;
    my_w = weights + begin;
  }

  OutT* out_row = out + sample * out_width + entry.column_base;
  // One pass of the column loop: `row_lane` = which N codes of the row this lane pools in the pass; walk(gather) hands the
  // bag's lookups to gather(count, index_at, weight_at) in lookup order (the contract of Quantized4BitRowPool::Gather).
  const auto pool_columns = [&](const int row_lane, const auto walk) {
    Quantized4BitRowPool<OutT, N, kWeighted> pool;
    const int first_byte = row_lane * kLaneBytes;                    // < code_bytes: the load stays inside the row's codes
    const uint8_t* lane_base = (const uint8_t*)(table_base + first_byte);
    const int64_t trailer_delta = code_bytes - first_byte;           // the row's trailer, from this pass's codes
    walk([&](const int count, const auto index_at, const auto weight_at) {
      if (stream_rows) pool.template Gather<kUnroll, true>(lane_base, trailer_delta, row_bytes, count, index_at, weight_at);
      else pool.template Gather<kUnroll, false>(lane_base, trailer_delta, row_bytes, count, index_at, weight_at);
    });
    // ---- epilogue of GatherReduceQuantized4BitKernel: even / odd accumulators back into element order, the bag's bias
    // once, mean scaling, one rounding to OutT ----
    const float inv = is_mean ? MeanFactor<kWeighted>(pool.weight_sum, hot) : 1.f;
    float v[N];
#pragma unroll
    for (int e = 0; e < N; ++e) {
      v[e] = A::add(pool.acc[e / 8][e % 2][(e % 8) / 2], pool.bias_sum);
      if (is_mean) v[e] = A::mul(v[e], inv);
    }
    StoreWideStreaming<OutT, N>(out_row + row_lane * N, v);
  };
  // every lookup read where it lies (LDS when staged, else one address per bag: a broadcast load that mostly hits L1)
  const auto walk_direct = [&](const auto gather) {
    gather(hot, [&](int j) { return WidenIndex(my_idx[j]); }, [&](int j) { return my_w[j]; });
  };

  if (!kStaged && lanes <= 64 && 64 % lanes == 0) {
    // ---- the lanes of a bag are consecutive lanes of ONE wavefront (and the row fits them: one pass): they fetch
    // `lanes` indices (+ weights) with one coalesced load and hand them to each other with cross-lane reads; the next
    // chunk is fetched while the current one is pooled
    pool_columns(lane, [&](const auto gather) {
      IndexT cur_i = static_cast<IndexT>(0);
      OutT cur_w = static_cast<OutT>(0);
      if (lane < hot) {
        cur_i = my_idx[lane];
        if constexpr (kWeighted) cur_w = my_w[lane];
      }
      for (int c = 0; c < hot; c += lanes) {
        IndexT next_i = static_cast<IndexT>(0);
        OutT next_w = static_cast<OutT>(0);
        if (c + lanes + lane < hot) {
          next_i = my_idx[c + lanes + lane];
          if constexpr (kWeighted) next_w = my_w[c + lanes + lane];
        }
        gather((hot - c < lanes) ? hot - c : lanes, [&](int j) { return WidenIndex(__shfl(cur_i, j, lanes)); },
               [&](int j) { return ShuffleElem(cur_w, j, lanes); });
        cur_i = next_i;
        cur_w = next_w;
      }
    });
  } else {
    for (int row_lane = lane; row_lane < row_lanes; row_lane += lanes) pool_columns(row_lane, walk_direct);
  }
}

}  // namespace detail
}  // namespace cuembed

#endif  // CUEMBED_INCLUDE_QUANTIZED_4BIT_MIXED_GROUP_GATHER_KERNELS_HPP_
