// MI355X (gfx950 / CDNA4) gather-reduce kernel for a group of tables of DIFFERENT widths (one element type), pooled in
// one launch (an extension: the reference lists "multiple tables" under future work).
//
// Layout: the input is the same-width group's (grouped_gather_kernels.hpp) -- bag g = t * B + b belongs to table t and
// sample b; CSR has one indices[nnz], one offsets[T * B + 1] and optional weights[nnz]; fixed hotness has indices
// [T, B, H].  The result is out[B, D], D = sum of the widths: bag (t, b) is stored at columns [c_t, c_t + W_t) of row b,
// c_t the exclusive prefix sum of the widths -- torch.cat of T single-table results on dim 1.
//
// A WORKGROUP SERVES BAGS OF ONE TABLE.  With N elements per lane (one value for the launch), table t takes
// L_t = min(W_t / N, blockDim.x) lanes per bag and a workgroup holds spb_t = blockDim.x / L_t consecutive bags of it:
// thread tid is lane tid % L_t of slot tid / L_t, threads past spb_t * L_t idle.  Table t owns ceil(B / spb_t)
// consecutive workgroups; the grid is their sum.  The table of a workgroup follows from blockIdx.x by a search over the
// prefix of those counts -- every wavefront loads 64 prefix words at a time, one per lane, and counts the ones at or
// below blockIdx.x with a ballot -- so it is a wavefront-uniform value, and the words of the table (width, column base,
// lanes, first workgroup: one 16-byte descriptor entry) and its base pointer are scalar loads into scalar registers.
// The base is kept in a global-address-space pointer (GlobalPtr) so that the row loads are global_load, not flat_load.
//
// A row wider than the workgroup's lanes (fp32 W = 514 at 8-byte lanes: 257 lanes, 256 threads) is pooled by a COLUMN
// LOOP: a lane pools columns lane, lane + L_t, ... of its bag one after the other, walking the bag once per pass (the
// indices come out of LDS or L1 after the first).  Only rows of more than blockDim.x lanes take a second pass.
//
// The walk is a sibling of WalkSample (gather_reduce_kernels.hpp) that takes slot, lane and the lanes of a bag as
// values: fixed hotness staged through LDS (a workgroup's bags are consecutive bags of one table, so its indices are
// contiguous in [T, B, H]), CSR by cross-lane reads when L_t divides 64 and by broadcast loads otherwise -- a choice that
// is uniform per workgroup.  The pooling is RowPool::Gather, the epilogue FinishPooledRow: fp32 accumulation in lookup
// order and one rounding at the store, so the result has the bits of T single-table calls.
#ifndef CUEMBED_INCLUDE_MIXED_GROUP_GATHER_KERNELS_HPP_
#define CUEMBED_INCLUDE_MIXED_GROUP_GATHER_KERNELS_HPP_

#include <cstdint>

#include "cuembed/include/gather_reduce_kernels.hpp"
#include "cuembed/include/grouped_gather_kernels.hpp"

namespace cuembed {
namespace detail {

constexpr int kMixedGroupBlockThreads = 256;

//! One entry of the device descriptor of a mixed-width group (FillMixedGroupDescriptor, mixed_group_lookup.hpp): T + 1
//! entries; entry T closes the prefixes (width 0, column_base D, lanes 0, first_block = the grid).
struct MixedGroupEntry {
  int32_t width;        //!< W_t, elements per row
  int32_t column_base;  //!< c_t, first column of the table in a row of out
  int32_t lanes;        //!< L_t, lanes that pool one bag: min(W_t / N, block threads)
  int32_t first_block;  //!< workgroups of the tables in front of this one
};

//! The table whose workgroups include `block`: the t with first_block[t] <= block < first_block[t + 1].  Uniform per
//! wavefront (a ballot's population count); every lane of the wavefront must call it.
__device__ __forceinline__ int MixedGroupTableOfBlock(const MixedGroupEntry* __restrict__ descriptor,
                                                      const int num_tables, const int block) {
  const int lane = static_cast<int>(threadIdx.x & 63u);
  int table = 0;
  for (int base = 0; base < num_tables; base += 64) {
    const int t = base + lane;
    // tables in front of the workgroup's: those whose successor's first workgroup is at or below `block`
    const bool before = t < num_tables && descriptor[t + 1].first_block <= block;
    const int count = __builtin_popcountll(__builtin_amdgcn_ballot_w64(before));
    table += count;
    if (count < 64) break;
  }
  return __builtin_amdgcn_readfirstlane(table);
}

// ---------------------------------------------------------------------------
// Sum / mean on a group of tables of mixed widths.
//   block = kMixedGroupBlockThreads (1-D); grid = descriptor[num_tables].first_block
//   dynamic LDS (kStaged only) = max_t(spb_t) * num_hots * (sizeof(IndexT) [+ sizeof(ElemT) if weighted])
// ---------------------------------------------------------------------------
template <typename ElemT,    // table / output element
          typename IndexT,   // int32_t / int64_t
          typename OffsetT,  // CSR offset type (unused when offsets == nullptr)
          int N,             // elements per lane, one value for the launch
          bool kWeighted,
          bool kStaged,      // fixed hotness, the workgroup's indices staged in LDS
          int kUnroll = kForwardUnroll>
__global__ void __launch_bounds__(kMixedGroupBlockThreads)
GatherReduceMixedGroupKernel(const ElemT* const* __restrict__ tables,             // [num_tables] table bases, device memory
                             const MixedGroupEntry* __restrict__ descriptor,      // [num_tables + 1], device memory
                             const int num_tables,
                             const int batch_per_table,                            // B
                             const IndexT* __restrict__ indices,
                             const OffsetT* __restrict__ offsets,                  // [T * B + 1], null => fixed hotness
                             const int num_hots,
                             const ElemT* __restrict__ weights,
                             const bool is_mean,
                             ElemT* __restrict__ out,                              // [B, out_width]
                             const int out_width,                                  // D
                             const bool stream_rows) {                             // RowLoadPolicy::kStreaming
  // ---- the workgroup's table: scalar values ----
  const int table = MixedGroupTableOfBlock(descriptor, num_tables, static_cast<int>(blockIdx.x));
  const MixedGroupEntry entry = descriptor[table];
  const GlobalPtr<ElemT> table_base = (GlobalPtr<ElemT>)tables[table];
  const int width = entry.width;
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
  const ElemT* my_w;
  int hot = num_hots;
  if constexpr (kStaged) {
    // ---- fixed hotness: the indices (+ weights) of the workgroup's bags, contiguous in [T, B, H], go through LDS once ----
    extern __shared__ __attribute__((aligned(16))) unsigned char mixed_lds_raw[];
    IndexT* stage_idx = reinterpret_cast<IndexT*>(mixed_lds_raw);
    ElemT* stage_w = reinterpret_cast<ElemT*>(stage_idx + slots * num_hots);
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

  ElemT* out_row = out + sample * out_width + entry.column_base;
  // One pass of the column loop: `columns` = this lane's first column of the pass; walk(gather) hands the bag's lookups
  // to gather(count, index_at, weight_at) in lookup order (the contract of RowPool::Gather).
  const auto pool_columns = [&](const int columns, const auto walk) {
    RowPool<ElemT, float, N, kWeighted> pool;
    const ElemT* lane_base = (const ElemT*)(table_base + columns);
    walk([&](const int count, const auto index_at, const auto weight_at) {
      if (stream_rows) pool.template Gather<kUnroll, kForwardPipelined, true>(lane_base, width, count, index_at, weight_at);
      else pool.template Gather<kUnroll, kForwardPipelined, false>(lane_base, width, count, index_at, weight_at);
    });
    FinishPooledRow<ElemT, float, N, kWeighted>(pool, hot, is_mean, out_row + columns);
  };
  // every lookup read where it lies (LDS when staged, else one address per bag: a broadcast load that mostly hits L1)
  const auto walk_direct = [&](const auto gather) {
    gather(hot, [&](int j) { return WidenIndex(my_idx[j]); }, [&](int j) { return my_w[j]; });
  };

  if (!kStaged && lanes <= 64 && 64 % lanes == 0) {
    // ---- the lanes of a bag are consecutive lanes of ONE wavefront (and the row fits them: one pass): they fetch
    // `lanes` indices (+ weights) with one coalesced load and hand them to each other with cross-lane reads; the next
    // chunk is fetched while the current one is pooled (WalkSample's kWaveShuffle branch, the group a run-time value)
    pool_columns(lane * N, [&](const auto gather) {
      IndexT cur_i = static_cast<IndexT>(0);
      ElemT cur_w = static_cast<ElemT>(0);
      if (lane < hot) {
        cur_i = my_idx[lane];
        if constexpr (kWeighted) cur_w = my_w[lane];
      }
      for (int c = 0; c < hot; c += lanes) {
        IndexT next_i = static_cast<IndexT>(0);
        ElemT next_w = static_cast<ElemT>(0);
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
    for (int row_lane = lane; row_lane < row_lanes; row_lane += lanes) pool_columns(row_lane * N, walk_direct);
  }
}

}  // namespace detail
}  // namespace cuembed

#endif  // CUEMBED_INCLUDE_MIXED_GROUP_GATHER_KERNELS_HPP_
