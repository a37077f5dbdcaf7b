// MI355X (gfx950 / CDNA4) sparse optimizer step on a group of tables of DIFFERENT widths -- the kernels.
//
// The compressed gradient of a mixed-width group (mixed_group_backward.hpp) names GLOBAL rows of the tables laid end to
// end, ascending, and pads every gradient row to the widest table: entry k holds its gradient in rows[k, :W_t].
// WalkNamedRows (sparse_update_kernels.hpp) gives every entry of a launch the same lane group, so a launch sized for the
// widest table would leave most lanes idle on the narrow ones (a 16-wide fp16 row fills 2 of the 16 lanes of a 128-wide
// one).  This is its sibling for such a group, with the lane group chosen PER TABLE inside the launch:
//
//   * The workgroup stages, once, in dynamic LDS: row_base[T + 1], the T base pointers of the tables and of every state
//     tensor the rule has, and the T widths (MixedGroupUpdateLdsBytes).
//   * A wavefront takes TILES of 64 consecutive entries, in a grid-stride loop over the tiles.  Lane j loads ids[k0 + j]
//     and resolves ITS OWN entry with the branch-free binary search over the staged row_base: one search per entry (the
//     grouped walk makes one per lane of a group), and (t, r) stay in registers.
//   * The wavefront serves the tile in PASSES.  A pass takes the next unserved entries that share one table t -- a
//     uniform loop driven by a ballot.  With g_t the lane group PlanUpdate gives W_t / N lanes, a pass serves up to
//     64 / g_t entries: lane l works on entry first + l / g_t, slice l % g_t, fetches that entry's row from the lane that
//     resolved it with a cross-lane read and reads table t's pointers and width from LDS at a uniform address.  A tile
//     inside one table uses all 64 lanes in every pass; a tile that straddles a cut costs one partial pass more.
//   * Inside a pass, in the order the grouped walk found it must be: the gradient loads first (they need k and t only),
//     then table and state loads, the row word loaded with the rows, then GroupSum over g_t lanes.  Passes of rows that
//     fit a lane group keep kInFlight (1 or 2) passes' loads in flight, as the single-table walk keeps two entries.
//   * A row wider than 64 lanes puts the whole wavefront on one entry, with the run-time loop over the slices of
//     WalkNamedRows' kChunks == 0; a row-wise rule then reads the gradient row a second time, out of the cache.
//   * The arithmetic is the rules' own (UpdateStep / AdamStepRule, StatePack, AddSquares, GroupSum, SliceRounding): the
//     only ordered quantity, the row-wise rules' sum of g^2, is formed per lane in slice order and then by the butterfly
//     over g_t lanes, which is the order of the single-table step at width W_t and the same N.  So tables and state have
//     the bits of T single-table steps run at the group's lane width.
//   * The padded columns rows[k, W_t:] are never addressed.  Round to nearest only.
#ifndef CUEMBED_INCLUDE_MIXED_GROUP_UPDATE_KERNELS_HPP_
#define CUEMBED_INCLUDE_MIXED_GROUP_UPDATE_KERNELS_HPP_

#include "cuembed/include/sparse_adam_kernels.hpp"
#include "cuembed/include/sparse_update_kernels.hpp"

namespace cuembed {
namespace detail {

constexpr int kMixedUpdateWave = 64;                                           //!< lanes of a wavefront = entries of a tile
constexpr int kMixedUpdateWaves = kUpdateBlockThreads / kMixedUpdateWave;      //!< wavefronts of a workgroup

//! What the walk over a mixed-width group reads besides ids and rows, all in device memory.
struct MixedGroupTables {
  const void* const* tables;     //!< [num_tables] table bases
  const float* const* state0;    //!< [num_tables] bases of the rule's first state tensor, or nullptr (no state)
  const float* const* state1;    //!< [num_tables] bases of its second, or nullptr
  const int64_t* row_base;       //!< [num_tables + 1] ascending, row_base[0] = 0
  const int* widths;             //!< [num_tables] elements per row of table t
  int num_tables;
};

//! Dynamic LDS of the walk in bytes: 8-byte words -- row_base[T + 1], the T table bases, the T bases of each state tensor
//! the rule has -- then the T widths as 4-byte ints.  T = kGroupedMaxTables with two state tensors: 36,836 bytes, inside
//! the 64 KiB a launch gets without asking.
constexpr int MixedGroupUpdateLdsBytes(const int num_tables, const int state_tensors) {
  return 8 * (num_tables + 1 + num_tables * (1 + state_tensors)) + 4 * num_tables;
}

//! A wave-uniform value, told to the compiler (it lands in scalar registers: a uniform base pointer then addresses the
//! row through the scalar operand of global_load / global_store).
__device__ __forceinline__ int WaveUniform(const int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ int64_t WaveUniform(const int64_t v) {
  const uint32_t lo = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(v)));
  const uint32_t hi = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(v >> 32)));
  return static_cast<int64_t>((static_cast<uint64_t>(hi) << 32) | lo);
}

//! The staged words of one table (uniform reads) as typed GLOBAL pointers, and its width.
template <typename ElemT, bool kUsesState0, bool kUsesState1>
struct MixedTablePlace {
  GlobalRowPtr<ElemT> table;
  GlobalRowPtr<float> state0, state1;
  int width;
  __device__ __forceinline__ void Read(const int64_t* words, const int* widths, const int T, const int t) {
    table = (GlobalRowPtr<ElemT>)reinterpret_cast<ElemT*>(static_cast<uintptr_t>(WaveUniform(words[T + 1 + t])));
    if constexpr (kUsesState0)
      state0 = (GlobalRowPtr<float>)reinterpret_cast<float*>(static_cast<uintptr_t>(WaveUniform(words[2 * T + 1 + t])));
    if constexpr (kUsesState1)
      state1 = (GlobalRowPtr<float>)reinterpret_cast<float*>(
          static_cast<uintptr_t>(WaveUniform(words[(kUsesState0 ? 3 : 2) * T + 1 + t])));
    width = WaveUniform(widths[t]);
  }
  __device__ __forceinline__ ElemT* Table() const { return (ElemT*)table; }
  __device__ __forceinline__ float* State0() const { return (float*)state0; }
  __device__ __forceinline__ float* State1() const { return (float*)state1; }
};

//! One pass of a tile, planned by the whole wavefront (every field is wave-uniform): the entries first .. first + n - 1
//! of the tile, all of table t, lanes_per_row = W_t / N slices each; group_log2 = log2 of PlanUpdate's lane group for
//! that many lanes; wide: more than 64 lanes, so n == 1 and the wavefront loops over the slices.
struct MixedPass {
  int first, n, t, lanes_per_row, group_log2;
  bool wide;
};

/**
 * @brief The walk over the named rows of a mixed-width group: tables[t][r, :W_t] and the state of row r of table t <-
 * rule(tables[t][r, :W_t], rows[k, :W_t]) for every valid entry k, t the last table with row_base[t] <= ids[k] and
 * r = ids[k] - row_base[t].  The body of the two kernels below.
 *
 * rows has a pitch of `max_width` elements.  One piece of `total_entries` entries; the count as in WalkNamedRows.
 * kInFlight: passes whose loads are in flight together (rows that fit a lane group only): 2, or 1 for an instantiation
 * that would spill with two (kMixedPassesInFlight).
 */
template <typename ElemT, typename IndexT, int N, int kInFlight, typename RuleT>
__device__ __forceinline__ void WalkMixedGroupRows(const IndexT* __restrict__ ids, const ElemT* __restrict__ rows,
                                                   const MixedGroupTables& g, const int max_width,
                                                   const int64_t total_entries, const UpdateCounts& counts,
                                                   const RuleT& rule) {
  static_assert(kInFlight == 1 || kInFlight == 2, "one or two passes in flight");
  using RoundT = SliceRounding<ElemT, N, false>;
  constexpr int kStates = RuleT::kStates;
  constexpr bool kRowState = RuleT::kRowState;
  constexpr int kHeld = kStates > 0 ? kStates : 1;
  constexpr bool kUsesState0 = kStates >= 1 || kRowState;
  constexpr bool kUsesState1 = kStates == 2 || (kStates == 1 && kRowState);
  using PlaceT = MixedTablePlace<ElemT, kUsesState0, kUsesState1>;
  // the tensor of the row words (only read if kRowState): the first state plane of a rule without per-element state
  const auto row_words_at = [](const PlaceT& at) { return kStates == 0 ? at.State0() : at.State1(); };

  // ---- stage the group, once per workgroup
  extern __shared__ int64_t mixed_group_lds_words[];
  int64_t* const words = mixed_group_lds_words;
  const int T = g.num_tables;
  int* const widths = reinterpret_cast<int*>(words + (T + 1 + T * (1 + (kUsesState0 ? 1 : 0) + (kUsesState1 ? 1 : 0))));
  for (int i = threadIdx.x; i <= T; i += kUpdateBlockThreads) words[i] = g.row_base[i];
  for (int i = threadIdx.x; i < T; i += kUpdateBlockThreads) {
    words[T + 1 + i] = static_cast<int64_t>(reinterpret_cast<uintptr_t>(g.tables[i]));
    if constexpr (kUsesState0) words[2 * T + 1 + i] = static_cast<int64_t>(reinterpret_cast<uintptr_t>(g.state0[i]));
    if constexpr (kUsesState1)
      words[(kUsesState0 ? 3 : 2) * T + 1 + i] = static_cast<int64_t>(reinterpret_cast<uintptr_t>(g.state1[i]));
    widths[i] = g.widths[i];
  }
  __syncthreads();

  const int lane = static_cast<int>(threadIdx.x) & (kMixedUpdateWave - 1);
  const int64_t first_tile = static_cast<int64_t>(blockIdx.x) * kMixedUpdateWaves + static_cast<int>(threadIdx.x) / kMixedUpdateWave;
  const int64_t tile_stride = static_cast<int64_t>(gridDim.x) * kMixedUpdateWaves;
  const int64_t count = PieceCount<IndexT>(counts, 0, total_entries);
  const int64_t tiles = (count + kMixedUpdateWave - 1) / kMixedUpdateWave;

  for (int64_t tile = first_tile; tile < tiles; tile += tile_stride) {
    // ---- lane j resolves entry k0 + j: its table and its row in that table, kept in registers
    const int64_t k0 = tile * kMixedUpdateWave;
    const bool live = k0 + lane < count;
    int64_t r = live ? WidenIndex(ids[k0 + lane]) : 0;
    int t = 0;
    for (int n = T; n > 1;) {   // (the LAST t with row_base[t] <= r: a table without rows owns nothing; any r gives a t in [0, T))
      const int half = n >> 1;
      if (words[t + half] <= r) t += half;
      n -= half;
    }
    r -= words[t];
    uint64_t todo = __ballot(live);

    // the next pass: the run of unserved entries from the lowest one on that share its table, cut at what a pass serves
    const auto next_pass = [&](const uint64_t unserved) {
      MixedPass p;
      p.first = WaveUniform(static_cast<int>(__builtin_ctzll(unserved)));
      p.t = __builtin_amdgcn_readlane(t, p.first);
      p.lanes_per_row = WaveUniform(widths[p.t]) / N;
      p.wide = p.lanes_per_row > kMixedUpdateWave;
      p.group_log2 = p.lanes_per_row <= 1 ? 0 : (p.wide ? 6 : 32 - __builtin_clz(static_cast<unsigned>(p.lanes_per_row - 1)));
      const uint64_t same = (__ballot(live && t == p.t) & unserved) >> p.first;
      const int run = ~same == 0 ? 64 : static_cast<int>(__builtin_ctzll(~same));   // (entries first .. first + run - 1)
      const int most = p.wide ? 1 : kMixedUpdateWave >> p.group_log2;
      p.n = run < most ? run : most;
      return p;
    };
    const auto served = [](const MixedPass& p) {
      return (p.n >= 64 ? ~uint64_t{0} : ((uint64_t{1} << p.n) - 1)) << p.first;
    };

    while (todo != 0) {
      MixedPass pass[kInFlight];
      pass[0] = next_pass(todo);
      todo &= ~served(pass[0]);
      if (pass[0].wide) {
        // ---- a row wider than the wavefront: one entry, slices lane, lane + 64, ... one after the other
        const MixedPass& p = pass[0];
        PlaceT at;
        at.Read(words, widths, T, p.t);
        const int64_t row_in_table = WaveUniform(static_cast<int64_t>(__shfl(static_cast<long long>(r), p.first)));
        const ElemT* g_row = RowPtr(rows, k0 + p.first, max_width);
        ElemT* w_row = const_cast<ElemT*>(RowPtr(at.Table(), row_in_table, at.width));
        float row = 0.f;
        if constexpr (kRowState) {
          float* const word = row_words_at(at) + row_in_table;
          const float before = *word;
          float sum = 0.f;
          for (int c = lane; c < p.lanes_per_row; c += kMixedUpdateWave) sum = AddSquares(sum, LoadPack<ElemT, N>(g_row + c * N));
          row = rule.Row(word, before, GroupSum(sum, kMixedUpdateWave), at.width, lane == 0);
        }
        for (int c = lane; c < p.lanes_per_row; c += kMixedUpdateWave) {
          const Pack<ElemT, N> gr = kRowState ? LoadPack<ElemT, N>(g_row + c * N) : LoadPackStreaming<ElemT, N>(g_row + c * N);
          const Pack<ElemT, N> w = LoadPack<ElemT, N>(w_row + c * N);
          const int64_t at_state = RowElems(row_in_table, at.width) + c * N;
          StatePack<N> s[kHeld];
          LoadStates<kStates>(s, at.State0(), at.State1(), at_state, at_state);
          StorePack<ElemT, N>(w_row + c * N, rule.Slice(w, gr, s, row, RoundT()));
          StoreStates<kStates>(s, at.State0(), at.State1(), at_state, at_state);
        }
        continue;   // (pass[1 ...] was never set: the next turn of the loop starts from `todo`)
      }
      // ---- rows that fit a lane group: up to kInFlight passes, the loads of all of them in flight together.  `passes`
      // is wave-uniform (it comes from ballots and todo alone), which is what lets the cross-lane reads below (__shfl,
      // GroupSum) sit inside `if (u < passes)`: every lane of the wavefront takes the same side.  pass[u] is set for
      // u < passes only; nothing reads it beyond.
      int passes = 1;
      if constexpr (kInFlight == 2) {
        if (todo != 0) {
          pass[1] = next_pass(todo);
          if (!pass[1].wide) {
            todo &= ~served(pass[1]);
            passes = 2;
          }
        }
      }
      PlaceT at[kInFlight];
      Pack<ElemT, N> gr[kInFlight], w[kInFlight];
      StatePack<N> s[kInFlight][kHeld];
      bool has[kInFlight];
      int col[kInFlight];
      int64_t row_in_table[kInFlight];
      float row_word[kInFlight];
      // the gradient rows need nothing but k and the table's width: their loads go first
#pragma unroll
      for (int u = 0; u < kInFlight; ++u) {
        has[u] = false;
        if (u < passes) {
          const MixedPass& p = pass[u];
          const int entry = lane >> p.group_log2;
          const int slice = lane & ((1 << p.group_log2) - 1);
          has[u] = entry < p.n && slice < p.lanes_per_row;
          col[u] = slice * N;
          const int source = (p.first + entry) & (kMixedUpdateWave - 1);   // (lanes without an entry read any lane)
          if (has[u]) gr[u] = LoadPackStreaming<ElemT, N>(RowPtr(rows, k0 + p.first + entry, max_width) + col[u]);
          row_in_table[u] = static_cast<int64_t>(__shfl(static_cast<long long>(r), source));
          at[u].Read(words, widths, T, p.t);
        }
      }
#pragma unroll
      for (int u = 0; u < kInFlight; ++u) {
        if (u < passes && has[u]) {
          if constexpr (kRowState) row_word[u] = row_words_at(at[u])[row_in_table[u]];
          w[u] = LoadPack<ElemT, N>(RowPtr(at[u].Table(), row_in_table[u], at[u].width) + col[u]);
          const int64_t at_state = RowElems(row_in_table[u], at[u].width) + col[u];
          LoadStates<kStates>(s[u], at[u].State0(), at[u].State1(), at_state, at_state);
        }
      }
#pragma unroll
      for (int u = 0; u < kInFlight; ++u) {
        if (u < passes) {
          float row = 0.f;
          if constexpr (kRowState) {
            // (every lane of the wavefront takes part in the butterfly: the lanes without a slice add zero)
            const float sum = GroupSum(has[u] ? AddSquares(0.f, gr[u]) : 0.f, 1 << pass[u].group_log2);
            if (has[u]) row = rule.Row(row_words_at(at[u]) + row_in_table[u], row_word[u], sum, at[u].width, col[u] == 0);
          }
          if (has[u]) {
            ElemT* w_at = const_cast<ElemT*>(RowPtr(at[u].Table(), row_in_table[u], at[u].width)) + col[u];
            const int64_t at_state = RowElems(row_in_table[u], at[u].width) + col[u];
            StorePack<ElemT, N>(w_at, rule.Slice(w[u], gr[u], s[u], row, RoundT()));
            StoreStates<kStates>(s[u], at[u].State0(), at[u].State1(), at_state, at_state);
          }
        }
      }
    }
  }
}

//! Passes in flight of the kernel launched for (rule, N): two, as the single-table walk's two entries.  A specialisation
//! on (rule, N) is where a fallback to one goes for an instantiation that would spill with two
//! (profiles/mixed_group_sparse_update_kernel_resources.txt).
template <auto kRule, int N>
constexpr int kMixedPassesInFlight = 2;
//! Adam on eight 16-bit elements per lane: two passes hold 2 x (8 + 8 + 16 + 16) registers of row data next to the walk's
//! own and leave 2 waves per SIMD (172 VGPRs); with one pass it has 123 VGPRs and 4 waves per SIMD (the single-table kernel: 6).
template <>
constexpr int kMixedPassesInFlight<AdamRule::kAdam, 8> = 1;

/**
 * @brief SGD / Adagrad / row-wise Adagrad on a mixed-width group (WalkMixedGroupRows).  g.state0 holds the bases of the
 * rule's one state tensor (nullptr for SGD): fp32 [rows_t, W_t] (kAdagrad) or [rows_t] (kRowwiseAdagrad).
 *
 * Launch: 1-D grid of kUpdateBlockThreads-thread workgroups (PlanMixedGroupUpdate), MixedGroupUpdateLdsBytes(num_tables,
 * the rule's state tensors) bytes of dynamic LDS.
 */
template <typename ElemT, typename IndexT, int N, UpdateRule kRule, int kInFlight>
__global__ void __launch_bounds__(kUpdateBlockThreads)
    SparseRowUpdateMixedGroupKernel(const IndexT* __restrict__ ids, const ElemT* __restrict__ rows,
                                    const MixedGroupTables g, const int max_width, const int64_t total_entries,
                                    const UpdateCounts counts, const float lr_value, const float* __restrict__ lr_word,
                                    const float eps) {
  const UpdateStep<kRule> rule{lr_word != nullptr ? *lr_word : lr_value, eps};
  WalkMixedGroupRows<ElemT, IndexT, N, kInFlight>(ids, rows, g, max_width, total_entries, counts, rule);
}

/**
 * @brief Adam / row-wise Adam on a mixed-width group: g.state0 = the exp_avg bases (fp32 [rows_t, W_t]), g.state1 = the
 * exp_avg_sq bases ([rows_t, W_t], or [rows_t] for kRowwiseAdam).  Launch as above, with two state tensors.
 */
template <typename ElemT, typename IndexT, int N, AdamRule kRule, int kInFlight>
__global__ void __launch_bounds__(kUpdateBlockThreads)
    SparseRowAdamMixedGroupKernel(const IndexT* __restrict__ ids, const ElemT* __restrict__ rows,
                                  const MixedGroupTables g, const int max_width, const int64_t total_entries,
                                  const UpdateCounts counts, const float lr_value, const float* __restrict__ lr_word,
                                  const float bias_value, const float* __restrict__ bias_word, const AdamScalars h) {
  const float lr = lr_word != nullptr ? *lr_word : lr_value;
  const float c = bias_word != nullptr ? *bias_word : bias_value;
  const AdamStepRule<kRule> rule{{Arith<float>::mul(lr, c), Arith<float>::mul(lr, h.weight_decay), h.weight_decay != 0.f}, h};
  WalkMixedGroupRows<ElemT, IndexT, N, kInFlight>(ids, rows, g, max_width, total_entries, counts, rule);
}

}  // namespace detail
}  // namespace cuembed

#endif  // CUEMBED_INCLUDE_MIXED_GROUP_UPDATE_KERNELS_HPP_
