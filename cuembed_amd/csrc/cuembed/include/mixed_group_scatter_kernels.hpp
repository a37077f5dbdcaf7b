// MI355X (gfx950 / CDNA4) kernels for the backward of a group of tables of DIFFERENT widths (an extension; the group is
// that of mixed_group_gather_kernels.hpp: bag g = t * B + b, grad_y [B, D], table t at columns [c_t, c_t + W_t)).
//
//   MixedGroupScatterAddKernel   the scatter-add of the sorted lookups of ALL tables into one compressed gradient
//                                rows[capacity, W_max], entry k in rows[k, :W_t] of the table t its id falls in
//   MixedGroupMeanScaleKernel    grad_y of a mean-pooled mixed group -> grad_y of the equivalent sum-pooled one
//
// MixedGroupScatterAddKernel is a SIBLING of SegmentedScatterAddKernel (scatter_add_kernels.hpp), assembled from the same
// phases.  ScatterStage, ScatterPlace, StageSentinels, NameRuns, RunSum, FlushStore, ChainPartials and
// ZeroSharedAndTailRowsKernel are used as they are, with width = W_max: the gradient is PADDED to the widest table, so
// every row address stays row * W_max.  Two phases know about the tables:
//
//   StageMixedLookups   (for StageLookups) a sorted lookup carries the sample id s = b * T + t.  Once per lookup:
//                       b = s / T (QuotientMagic), t = s - b * T, (c_t, W_t) from a [T][2] device array read through L1
//                       (no bound on T), and what goes to LDS is the lookup's SOURCE OFFSET (b * D + c_t) / N in lane
//                       units -- 31 bits next to kRunEndBit -- plus, in a second region, its lane count W_t / N.
//   WalkMixedSegment    (for WalkSegment) the same rolling window; lane L of the padded row requests nothing for a lookup
//                       with L >= W_t / N and adds +0 for it.  The predicate is per lookup: a segment holds runs of
//                       several tables.  A run inside the segment ends in one non-temporal store of its ACTIVE lanes.
//
// Padding columns (>= W_t of an entry's table): a run that lies inside one segment never touches them; a run that is
// chained through ChainPartials -- whose flushes are not predicated -- gets zeros there (a plain store of +0 partials, or
// +0 atomics onto the row that ZeroSharedAndTailRowsKernel zeroed over all W_max columns).  So: untouched or zero.
#ifndef CUEMBED_INCLUDE_MIXED_GROUP_SCATTER_KERNELS_HPP_
#define CUEMBED_INCLUDE_MIXED_GROUP_SCATTER_KERNELS_HPP_

#include <cstdint>

#include "cuembed/include/gather_reduce_kernels.hpp"
#include "cuembed/include/scatter_add_kernels.hpp"

namespace cuembed {
namespace detail {

//! ScatterStage plus the lane counts of the staged lookups: uint16 [segments][packed_stride], one per packed word (a row
//! has at most kMaxBlockThreads lanes).  The host sizes the launch from `bytes`, the kernel carves from the same object.
struct MixedScatterStage {
  ScatterStage base;
  unsigned lane_counts;
  unsigned bytes;
  __host__ __device__ static MixedScatterStage Of(const int segments, const int segment_len, const int lanes, const int n,
                                                  const bool weighted, const int elem_bytes) {
    MixedScatterStage s;
    s.base = ScatterStage::Of(segments, segment_len, lanes, n, weighted, elem_bytes);
    s.lane_counts = s.base.bytes;   // (a multiple of 16)
    s.bytes = ScatterStage::Up16(s.lane_counts + static_cast<unsigned>(segments) * s.base.packed_stride * 2u);
    return s;
  }
};

//! Staging of a mixed group: StageLookups' loop with the translation sample id -> (source offset, lane count).
//! `table_columns`: [T][2] = (c_t, W_t) in elements; `row_lanes` = D / N.  Positions past nnz hold offset 0 and NO lanes.
template <typename GradT, typename IndexT, int N, bool kWeighted>
__device__ __forceinline__ void StageMixedLookups(const ScatterStageView<GradT>& st, uint16_t* __restrict__ lane_counts,
                                                  const ScatterPlace& at, const IndexT* __restrict__ rows,
                                                  const IndexT* __restrict__ sample_ids, const GradT* __restrict__ weights,
                                                  const int2* __restrict__ table_columns, const uint32_t num_tables,
                                                  const uint32_t by_tables_magic, const int by_tables_shift,
                                                  const uint32_t row_lanes) {
  const int tid = at.seg * at.lanes + at.lane_x;
  const int threads = at.lanes * at.segments;
  for (int e0 = tid; e0 < at.block_len; e0 += threads * kStageBatch) {
    int32_t r[kStageBatch], r_next[kStageBatch];
    uint32_t sid[kStageBatch];
    GradT wv[kStageBatch];
#pragma unroll
    for (int q = 0; q < kStageBatch; ++q) {
      const int64_t g = at.block_begin + e0 + q * threads;
      const bool in = e0 + q * threads < at.block_len && g < at.nnz;
      r[q] = in ? static_cast<int32_t>(rows[g]) : -1;
      r_next[q] = (in && g + 1 < at.nnz) ? static_cast<int32_t>(rows[g + 1]) : -1;
      sid[q] = in ? static_cast<uint32_t>(static_cast<int32_t>(sample_ids[g])) : 0u;
      if constexpr (kWeighted) wv[q] = in ? weights[g] : static_cast<GradT>(0);
    }
    uint32_t sample[kStageBatch];
    int2 column[kStageBatch];
#pragma unroll
    for (int q = 0; q < kStageBatch; ++q) {   // (all table reads of the batch requested before the first is used)
      sample[q] = static_cast<uint32_t>((static_cast<uint64_t>(sid[q]) * by_tables_magic) >> by_tables_shift);
      column[q] = table_columns[sid[q] - sample[q] * num_tables];
    }
#pragma unroll
    for (int q = 0; q < kStageBatch; ++q) {
      const int e = e0 + q * threads;
      if (e < at.block_len) {
        const int s = at.SegmentOf(e);
        const int i = e - s * at.segment_len;
        uint32_t pk = 0;
        uint16_t lc = 0;
        if (r[q] >= 0) {
          pk = (sample[q] * row_lanes + static_cast<uint32_t>(column[q].x) / N) | (r_next[q] != r[q] ? kRunEndBit : 0u);
          lc = static_cast<uint16_t>(static_cast<uint32_t>(column[q].y) / N);
          if constexpr (kWeighted) st.weights[s * st.row_stride + i] = wv[q];
        }
        st.rows[s * st.row_stride + 1 + i] = r[q];
        st.packed[s * st.packed_stride + i] = pk;
        lane_counts[s * st.packed_stride + i] = lc;
      }
    }
  }
}

//! The walk of one segment of a mixed group: WalkSegment with a per-lookup lane predicate.  `row_lane`: which lane of
//! the PADDED row (W_max / N lanes) this thread is; `lane_src`: this lane's elements of grad_y's first N-element unit
//! row, i.e. grad_y + row_lane * N; `lane_dst`: this lane's elements of row 0 of the gradient; `width` = W_max.
template <typename GradT, int N, bool kWeighted, int kWindow>
__device__ __forceinline__ void WalkMixedSegment(const ScatterStageView<GradT>& st, const uint16_t* __restrict__ lane_counts,
                                                 const ScatterPlace& at, const int row_lane,
                                                 const GradT* __restrict__ lane_src, GradT* __restrict__ lane_dst,
                                                 const int width) {
  using Sum = RunSum<GradT, N, kWeighted>;
  const int seg = at.seg, lane_x = at.lane_x, lanes = at.lanes, segment_len = at.segment_len;
  const int32_t* my_rows = st.rows + seg * st.row_stride + 1;  // my_rows[-1] = lookup before the segment
  const uint32_t* my_pk = st.packed + seg * st.packed_stride;
  const uint16_t* my_lc = lane_counts + seg * st.packed_stride;
  const GradT* my_w = st.weights + seg * st.row_stride;
  typedef uint32_t __attribute__((ext_vector_type(4))) word4_t;
  typedef uint32_t __attribute__((ext_vector_type(2))) word2_t;
  constexpr int K = kWindow;
  static_assert(K % 4 == 0, "packed ids are fetched four at a time");

  bool first_pending = my_rows[0] >= 0 && my_rows[-1] == my_rows[0];   // the first run came in from before
  const bool tail_shared = my_rows[segment_len - 1] >= 0 && my_rows[segment_len] == my_rows[segment_len - 1];

  Sum sum;
  sum.Zero();
  auto note = [&](const int slot, const int64_t row, const int flag) {
    if (lane_x == 0) {
      st.partial_rows[seg * 2 + slot] = row;
      st.flags[seg] |= flag;
    }
  };
  auto park = [&](float* partials) {
    float a[N];
    sum.Unpair(a);
#pragma unroll
    for (int e = 0; e < N; ++e) partials[(seg * N + e) * lanes + lane_x] = a[e];
  };
  // the K packed words of a batch, and bit u of `active` = this lane has elements of lookup u's table
  auto fetch_ids = [&](uint32_t (&dst)[K], uint32_t& active, const int i0) {
    active = 0;
#pragma unroll
    for (int q = 0; q < K / 4; ++q) {
      const word4_t v = *reinterpret_cast<const word4_t*>(my_pk + i0 + 4 * q);
      dst[4 * q + 0] = v.x; dst[4 * q + 1] = v.y; dst[4 * q + 2] = v.z; dst[4 * q + 3] = v.w;
      const word2_t c = *reinterpret_cast<const word2_t*>(my_lc + i0 + 4 * q);
      active |= (row_lane < static_cast<int>(c.x & 0xffffu) ? 1u : 0u) << (4 * q + 0);
      active |= (row_lane < static_cast<int>(c.x >> 16) ? 1u : 0u) << (4 * q + 1);
      active |= (row_lane < static_cast<int>(c.y & 0xffffu) ? 1u : 0u) << (4 * q + 2);
      active |= (row_lane < static_cast<int>(c.y >> 16) ? 1u : 0u) << (4 * q + 3);
    }
  };
  typedef uint32_t __attribute__((ext_vector_type(sizeof(Pack<GradT, N>) / 4))) raw_t;
  auto gather = [&](const uint32_t packed, const bool on) {
    raw_t v = {};
    if (on) v = *reinterpret_cast<const raw_t*>(RowPtr(lane_src, static_cast<int64_t>(packed & ~kRunEndBit), N));
    return v;
  };

  raw_t g[K];
  uint32_t cur[K], nxt[K];
  uint32_t cur_on, nxt_on = 0;
  fetch_ids(cur, cur_on, 0);
#pragma unroll
  for (int u = 0; u < K; ++u) g[u] = gather(cur[u], (cur_on >> u) & 1u);
  auto batch = [&](const int i, auto more_tag) {
    constexpr bool kMore = decltype(more_tag)::value;
    if constexpr (kMore) fetch_ids(nxt, nxt_on, i + K);
    GradT w[K];
    if constexpr (kWeighted) {
#pragma unroll
      for (int u = 0; u < K; ++u) w[u] = my_w[i + u];
    }
#pragma unroll
    for (int u = 0; u < K; ++u) {
      typename Sum::pair_t f[Sum::kPairs];
      Sum::Term(__builtin_bit_cast(Pack<GradT, N>, g[u]), w[u], f);   // (a lane without elements: +0 [* w])
      if constexpr (kMore) {
        __builtin_amdgcn_sched_barrier(0);   // the registers of lookup i are free: request i + K into them
        g[u] = gather(nxt[u], (nxt_on >> u) & 1u);
        __builtin_amdgcn_sched_barrier(0);
      }
      if ((cur_on >> u) & 1u) sum.Add(f);   // (an inactive lane keeps its +0: 0 * inf or 0 * nan never enters)
      if (static_cast<int32_t>(cur[u]) < 0) {   // kRunEndBit: the run ends with this lookup
        const uint32_t row = static_cast<uint32_t>(my_rows[i + u]);
        if (first_pending) {   // its first lookups are in earlier segments
          park(st.head_partials);
          note(0, static_cast<int64_t>(row), kPartHead);
        } else if ((cur_on >> u) & 1u) {   // the run's lookups are of ONE table: its lanes store, the padding stays
          GradT* dst = const_cast<GradT*>(RowPtr(lane_dst, static_cast<int64_t>(row), width));
          float a[N];
          sum.Unpair(a);
          FlushStore<GradT, N>(dst, a);
        }
        first_pending = false;
        sum.Restart();
      }
    }
    if constexpr (kMore) {
#pragma unroll
      for (int u = 0; u < K; ++u) cur[u] = nxt[u];
      cur_on = nxt_on;
    }
  };
  int i = 0;
  for (; i + K < segment_len; i += K) batch(i, std::true_type{});
  batch(i, std::false_type{});   // the last K lookups: nothing left to request
  if (tail_shared)   // the last run goes on into the next segment (kPartWhole: it also came in)
    note(1, static_cast<int64_t>(static_cast<uint32_t>(my_rows[segment_len - 1])), kPartTail | (first_pending ? kPartWhole : 0));
  __syncthreads();   // nobody reads the staged ids any more: tail_partials lies on top of them
  if (tail_shared) park(st.tail_partials);
}

//! block = (lanes of one column slice of the PADDED row, segments_per_block); grid and dynamic LDS as
//! SegmentedScatterAddKernel's for width = W_max (PlanScatter), the LDS plus the lane counts (MixedScatterStage).
//! `rows` are the remapped (dense, ascending) ids of the sorted lookups, `sample_ids` their b * T + t, `run_ids` the
//! global row ids that NameRuns writes into inverse_mapping.  capacity_rows / capacity_overflow: as in
//! SegmentedScatterAddKernel -- a launch whose last id does not fit writes nothing and raises the word.
template <typename GradT, typename IndexT, int N, bool kWeighted, int kWindow>
__global__ void __launch_bounds__(kMaxBlockThreads)
MixedGroupScatterAddKernel(const GradT* __restrict__ grad_y,           // [B, D]
                           const int2* __restrict__ table_columns,     // [T][2] = (c_t, W_t), elements
                           const uint32_t num_tables,
                           const uint32_t by_tables_magic,
                           const int by_tables_shift,
                           const uint32_t row_lanes,                   // D / N
                           const int width,                            // W_max: the pitch of grad_out
                           const IndexT* __restrict__ rows,
                           const IndexT* __restrict__ sample_ids,
                           const GradT* __restrict__ weights,
                           const int64_t nnz,
                           const int segment_len,
                           const int segment_shift,
                           GradT* __restrict__ grad_out,               // [capacity, W_max]
                           const int column_slices,
                           const int xcds,
                           const IndexT* __restrict__ run_ids,
                           IndexT* __restrict__ inverse_mapping,
                           const int64_t capacity_rows,
                           uint32_t* __restrict__ capacity_overflow) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  const int lanes = blockDim.x, segments_per_block = blockDim.y;  // (lanes of ONE column slice)
  const int block_len = segments_per_block * segment_len;
  const ColumnSlice cs = ColumnSlice::Of(blockIdx.x, column_slices, xcds);
  const ScatterPlace at{static_cast<int>(threadIdx.x), lanes, static_cast<int>(threadIdx.y), segments_per_block,
                        segment_len, segment_shift, block_len, cs.block * block_len, nnz};
  if (at.block_begin >= nnz) return;  // the grid is rounded up to whole rounds of `xcds` workgroups
  if (capacity_rows > 0) {
    const uint32_t last = static_cast<uint32_t>(rows[nnz - 1]);
    if (static_cast<int64_t>(last) >= capacity_rows) {
      if (blockIdx.x == 0 && threadIdx.x == 0 && threadIdx.y == 0 && capacity_overflow != nullptr)
        atomicOr(capacity_overflow, 1u);
      return;
    }
  }
  const MixedScatterStage stage =
      MixedScatterStage::Of(segments_per_block, segment_len, lanes, N, kWeighted, static_cast<int>(sizeof(GradT)));
  const ScatterStageView<GradT> st(lds_raw, stage.base);
  uint16_t* lane_counts = reinterpret_cast<uint16_t*>(lds_raw + stage.lane_counts);
  const int row_lane = cs.slice * lanes + at.lane_x;   // this thread's lane of the padded row

  StageMixedLookups<GradT, IndexT, N, kWeighted>(st, lane_counts, at, rows, sample_ids, weights, table_columns,
                                                 num_tables, by_tables_magic, by_tables_shift, row_lanes);
  if (at.lane_x == 0) st.flags[at.seg] = 0;
  __syncthreads();
  StageSentinels<GradT, IndexT>(st, at, rows, nullptr);
  __syncthreads();
  if (run_ids != nullptr && cs.slice == 0) NameRuns<GradT, IndexT>(st, at, ~0u, run_ids, inverse_mapping);
  const int64_t column0 = static_cast<int64_t>(row_lane) * N;
  WalkMixedSegment<GradT, N, kWeighted, kWindow>(st, lane_counts, at, row_lane, grad_y + column0, grad_out + column0, width);
  __syncthreads();
  if (at.block_begin + at.seg * segment_len >= nnz) return;   // a segment past the end has nothing parked
  ChainPartials<GradT, N, false>(st, at, grad_out + column0, width);
}

// ---------------------------------------------------------------------------
// Mean scaling of a mixed group's grad_y: GroupedMeanScaleKernel's arithmetic on [B, D].
//   block = (group, slices_per_block), group a power of two <= 64 that covers W_max / N lanes (or 64);
//   grid = ceil(B * T / slices_per_block); lane group r = b * T + t scales grad_y[b, c_t : c_t + W_t] by the mean factor
//   of bag t * B + b.
// The weighted factor is 1 / the fp32 sum of the bag's weights, and a float sum has an order: this kernel takes the one
// GroupedMeanScaleKernel takes for a one-table group of width W_t on aligned buffers -- g_t lanes (the power of two that
// covers W_t * sizeof / its own lane bytes, at most 64) each sum a strided part, a butterfly folds them -- so that the
// factor, and with it every element, has the bits of that call.  g_t <= group (the launch's lanes are no wider than the
// table's own), so lane l plays lane l mod g_t of that call and the butterfly below g_t stays inside each copy.
// ---------------------------------------------------------------------------
template <typename ElemT, typename OffsetT, int N, bool kWeighted>
__global__ void __launch_bounds__(kMaxBlockThreads)
MixedGroupMeanScaleKernel(const ElemT* grad_y,                        // [B, D]  (may be `out`)
                          const int2* __restrict__ table_columns,     // [T][2] = (c_t, W_t), elements
                          const OffsetT* __restrict__ offsets,        // [T * B + 1], null => fixed hotness
                          const ElemT* __restrict__ weights,          // the layout of the indices (kWeighted)
                          const int batch_per_table,                  // B
                          const int num_tables,                       // T
                          const int out_width,                        // D
                          const int rows,                             // B * T
                          const int num_hots,
                          ElemT* out) {                               // [B, D]
  const int lane_x = threadIdx.x;
  const int group = blockDim.x;
  const int64_t row = static_cast<int64_t>(blockIdx.x) * blockDim.y + threadIdx.y;
  if (row >= rows) return;
  const uint32_t sample = static_cast<uint32_t>(row) / static_cast<uint32_t>(num_tables);
  const uint32_t table = static_cast<uint32_t>(row) - sample * static_cast<uint32_t>(num_tables);
  const int2 column = table_columns[table];
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
    const uint32_t row_bytes = static_cast<uint32_t>(column.y) * static_cast<uint32_t>(sizeof(ElemT));
    const uint32_t own_lanes = row_bytes / (row_bytes % 16 == 0 ? 16u : (row_bytes % 8 == 0 ? 8u : 4u));
    int own_group = 1;
    while (own_group < static_cast<int>(own_lanes) && own_group < 64) own_group *= 2;
    if (own_group > group) own_group = group;   // (never on a launch that follows the lane rule)
    const ElemT* my_w = weights + begin;
    for (int j = lane_x & (own_group - 1); j < hot; j += own_group) weight_sum += static_cast<float>(my_w[j]);
    for (int d = own_group >> 1; d > 0; d >>= 1) weight_sum += __shfl_xor(weight_sum, d, group);
  }
  const float factor = MeanFactor<kWeighted>(weight_sum, hot);
  const int chunks = column.y / N;
  const int64_t first = static_cast<int64_t>(sample) * out_width + column.x;
  const ElemT* src = grad_y + first;
  ElemT* dst = out + first;
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

#endif  // CUEMBED_INCLUDE_MIXED_GROUP_SCATTER_KERNELS_HPP_
