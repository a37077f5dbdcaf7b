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
//     table's type at the store: to nearest, or (kStochastic, 16-bit tables) stochastically with the counter-based bits
//     of stochastic_rounding.hpp -- one Philox call per 16-byte slice, issued after the slice's loads; the bits depend
//     on (seed, step, table row, column) only, so every lane width, body and grid stores the same table.
//   * Row-wise Adagrad reduces the row's sum of squares inside the lane group with a butterfly of cross-lane reads
//     (`__shfl_xor`): no LDS, no atomics.  Every lane ends with the same bits, so no broadcast is needed.
//   * The number of valid entries is read on the device (UpdateCounts): the grid is fixed from the capacity, every
//     group strides over the entries of a piece, and a workgroup with nothing to do leaves after reading the counts.
//     Entries at or past the count are ignored whatever they hold; a count above the capacity (the backward then
//     wrote nothing) or below zero makes the piece empty.
//   * The valid entries must name DISTINCT rows (a coalesced gradient): there are no atomics on table data.
//   * All of this is ONE device function, WalkNamedRows, for the five rules (SGD, Adagrad, row-wise Adagrad here; Adam and
//     row-wise Adam in sparse_adam_kernels.hpp).  A rule type tells it how many per-element fp32 state tensors a slice
//     carries (0 / 1 / 2), whether the row has a state word of its own, and the arithmetic of a row and of a slice.
//   * The tables may be a GROUP of separate tensors (kGrouped; host API: grouped_sparse_update.hpp): the ids are then
//     global rows of the tables laid end to end and the walk finds each entry's table itself, from row_base and the base
//     pointers staged in LDS.  A grouped stochastic walk rounds table t with a seed of its own, seeds[t], staged there too.
#ifndef CUEMBED_INCLUDE_SPARSE_UPDATE_KERNELS_HPP_
#define CUEMBED_INCLUDE_SPARSE_UPDATE_KERNELS_HPP_

#include "cuembed/include/gather_reduce_kernels.hpp"
#include "cuembed/include/stochastic_rounding.hpp"

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

//! What stochastic rounding needs besides the fp32 value; an empty kernel argument when it is off.
template <bool kStochastic>
struct UpdateRounding {};
template <>
struct UpdateRounding<true> {
  uint64_t seed;
  uint64_t step;             //!< the step, unless ...
  const int64_t* step_word;  //!< ... one int64 word on the device holds it (a replayed graph draws fresh bits)
};

//! The one rounding to the table's type, for the N elements of a slice: to nearest ...
template <typename ElemT, int N, bool kStochastic>
struct SliceRounding {
  __device__ __forceinline__ ElemT operator()(const float x, const int) const { return static_cast<ElemT>(x); }
};
//! ... or stochastic, with the N fields of the slice's Philox call that belong to its columns (a slice of N = 8, 4 or
//! 2 elements never straddles a column group of 8).  Only the N / 2 words that hold them are kept, picked with selects:
//! nothing here is indexed at run time, so everything stays in registers.
template <typename ElemT, int N>
struct SliceRounding<ElemT, N, true> {
  static_assert(N == 8 || N == 4 || N == 2, "a 16-bit slice is 16, 8 or 4 bytes");
  uint32_t words[N / 2];
  __device__ __forceinline__ SliceRounding() {}
  __device__ __forceinline__ SliceRounding(const uint64_t seed, const uint64_t step, const int64_t row, const int col) {
    const PhiloxWords p = RoundingWords(seed, step, static_cast<uint64_t>(row), static_cast<uint32_t>(col) >> 3);
    if constexpr (N == 8) {
      words[0] = p.w[0], words[1] = p.w[1], words[2] = p.w[2], words[3] = p.w[3];
    } else if constexpr (N == 4) {
      const bool upper = (col & 4) != 0;
      words[0] = upper ? p.w[2] : p.w[0];
      words[1] = upper ? p.w[3] : p.w[1];
    } else {
      const uint32_t lo = (col & 2) != 0 ? p.w[1] : p.w[0];
      const uint32_t hi = (col & 2) != 0 ? p.w[3] : p.w[2];
      words[0] = (col & 4) != 0 ? hi : lo;
    }
  }
  __device__ __forceinline__ ElemT operator()(const float x, const int e) const {
    return StochasticRound<ElemT>(x, (words[e >> 1] >> ((e & 1) * 16)) & 0xFFFFu);
  }
};

//! w <- w - step * g, one slice (SGD: step = lr; row-wise Adagrad: step = lr / (sqrt(s_r) + eps)).
template <typename ElemT, int N, typename RoundT = SliceRounding<ElemT, N, false>>
__device__ __forceinline__ Pack<ElemT, N> ScaledStep(const Pack<ElemT, N>& w, const Pack<ElemT, N>& g, const float step,
                                                     const RoundT& round = RoundT()) {
  using A = Arith<float>;
  Pack<ElemT, N> out;
#pragma unroll
  for (int e = 0; e < N; ++e)
    out.v[e] = round(A::add(A::widen(w.v[e]), -A::mul(step, A::widen(g.v[e]))), e);
  return out;
}

//! Adagrad on one slice: s <- s + g^2 (in place), returns w - lr * g / (sqrt(s) + eps).
template <typename ElemT, int N, typename RoundT = SliceRounding<ElemT, N, false>>
__device__ __forceinline__ Pack<ElemT, N> AdagradStep(const Pack<ElemT, N>& w, const Pack<ElemT, N>& g, StatePack<N>& s,
                                                      const float lr, const float eps, const RoundT& round = RoundT()) {
  using A = Arith<float>;
  Pack<ElemT, N> out;
#pragma unroll
  for (int e = 0; e < N; ++e) {
    const float x = A::widen(g.v[e]);
    const float acc = A::add(s.at(e), A::mul(x, x));
    s.at(e) = acc;
    const float d = A::mul(lr, x) / A::add(sqrtf(acc), eps);
    out.v[e] = round(A::add(A::widen(w.v[e]), -d), e);
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

//! What the walk needs to know of a rule (RuleT of WalkNamedRows):
//!   kStates    per-element fp32 state tensors a slice carries next to its weights and gradient: 0, 1 or 2;
//!   kRowState  whether there is one more state word per row, fed with the row's summed squared gradient;
//!   Row(word, before, sum, width, store)   the per-row part: updates the word (lane 0 stores), returns the row's factor;
//!   Slice(w, g, s, row, round)             the new weights of one slice; updates the slice's state packs s[] in place.
//! The rules of SparseRowUpdateKernel; those of SparseRowAdamKernel are sparse_adam_kernels.hpp's AdamStepRule.
template <UpdateRule kRule>
struct UpdateStep {
  static constexpr int kStates = kRule == UpdateRule::kAdagrad ? 1 : 0;
  static constexpr bool kRowState = kRule == UpdateRule::kRowwiseAdagrad;
  float lr, eps;
  __device__ __forceinline__ float Row(float* word, const float before, const float sum, const int width,
                                       const bool store) const {
    return RowwiseStep(word, before, sum, width, store, lr, eps);
  }
  template <typename ElemT, int N, typename RoundT>
  __device__ __forceinline__ Pack<ElemT, N> Slice(const Pack<ElemT, N>& w, const Pack<ElemT, N>& g, StatePack<N>* s,
                                                  const float row, const RoundT& round) const {
    if constexpr (kStates == 1) return AdagradStep(w, g, s[0], lr, eps, round);
    else return ScaledStep(w, g, kRowState ? row : lr, round);
  }
};

//! The per-element state packs of one slice, `at0` / `at1` elements into the rule's kStates tensors (written out per
//! tensor: the pointers keep their __restrict__, which an array of them indexed in a loop loses).  The two offsets differ
//! only in a walk with two placed ids.
template <int kStates, int N>
__device__ __forceinline__ void LoadStates(StatePack<N>* s, const float* state0, const float* state1, const int64_t at0,
                                           const int64_t at1) {
  if constexpr (kStates > 0) s[0] = StatePack<N>::Load(state0 + at0);
  if constexpr (kStates > 1) s[1] = StatePack<N>::Load(state1 + at1);
}
template <int kStates, int N>
__device__ __forceinline__ void StoreStates(const StatePack<N>* s, float* state0, float* state1, const int64_t at0,
                                            const int64_t at1) {
  if constexpr (kStates > 1) s[1].Store(state1 + at1);
  if constexpr (kStates > 0) s[0].Store(state0 + at0);
}

//! The row that addresses an entry's state: the table row, or (kPlaced) the entry's own place for it.
template <bool kPlaced>
__device__ __forceinline__ int64_t StateRow(const int64_t table_row, const int64_t placed_row) {
  if constexpr (kPlaced) return placed_row;
  else return table_row;
}
//! The row that names an entry's rounding bits: the table row, or (kNamed) the name the entry carries for them.
template <bool kNamed>
__device__ __forceinline__ int64_t RoundingRow(const int64_t table_row, const int64_t named_row) {
  if constexpr (kNamed) return named_row;
  else return table_row;
}
//! The row that addresses an entry in `state1`: like state0's, or (kPlacedTwice) a second place of its own.
template <bool kPlaced, bool kPlacedTwice>
__device__ __forceinline__ int64_t State1Row(const int64_t table_row, const int64_t placed_row,
                                             const int64_t placed1_row) {
  if constexpr (kPlacedTwice) return placed1_row;
  else return StateRow<kPlaced>(table_row, placed_row);
}

//! A pointer into GLOBAL memory that is written through, typed as one (grouped_gather_kernels.hpp's GlobalPtr for the
//! forward): a pointer that was read from memory is a generic pointer to the compiler, and row traffic through it would
//! be flat_load / flat_store instead of global_load / global_store.
template <typename T>
using GlobalRowPtr = T __attribute__((address_space(1))) *;

//! What a walk over a GROUP of separate table tensors needs (WalkNamedRows' kGrouped): the base pointers of the T tables
//! and of their state tensors, and where each table begins in the rows laid end to end.  An empty kernel argument
//! without kGrouped.
template <bool kGrouped>
struct GroupedTables {};
template <>
struct GroupedTables<true> {
  const void* const* tables;     //!< [num_tables] table bases, in device memory
  const float* const* state0;    //!< [num_tables] bases of the rule's first state tensor, or nullptr (no state)
  const float* const* state1;    //!< [num_tables] bases of its second, or nullptr
  const int64_t* row_base;       //!< [num_tables + 1] in device memory, ascending, row_base[0] = 0
  int num_tables;
};
//! The same for a grouped STOCHASTIC walk, with the tables' rounding seeds: a type of its own, so that the kernel
//! arguments of the round-to-nearest kernels keep their layout.
struct GroupedSeededTables : GroupedTables<true> {
  const uint64_t* seeds;         //!< [num_tables] in device memory: table t rounds with the bits of (seeds[t], step, row, column)
};
//! The argument of a walk: nothing, the group, or (kSeeded) the group with its seeds.
template <bool kGrouped, bool kSeeded>
using GroupedTablesOf = std::conditional_t<kGrouped && kSeeded, GroupedSeededTables, GroupedTables<kGrouped>>;

//! Dynamic LDS of a grouped walk, in 8-byte words: row_base[T + 1], then the T table bases, then the T bases of each
//! state tensor the rule has, then (a stochastic walk) the T seeds.
constexpr int GroupedLdsWords(const int num_tables, const int state_tensors, const bool stochastic = false) {
  return num_tables + 1 + num_tables * (1 + state_tensors + (stochastic ? 1 : 0));
}
//! The most tables a grouped step takes: 32 KiB of LDS with two state tensors, 40 KiB with the seeds of a stochastic
//! step -- inside the 64 KiB a launch gets without asking.
constexpr int kGroupedMaxTables = 1023;

//! The rounding seed of one entry's table: kept only by a grouped stochastic walk.
template <bool kSeeded>
struct EntrySeed {};
template <>
struct EntrySeed<true> {
  uint64_t seed;
};

//! Where one entry's weights and state live.  Without kGrouped: in the walk's own table / state0 / state1, nothing is
//! kept and every accessor hands its argument back.  With kGrouped: in the tensors of the table that owns the entry's
//! global row, found by Resolve; the accessors ignore their argument.  kSeeded (with kGrouped only): the group's seeds
//! are staged behind the pointers and Resolve keeps seeds[t] next to them; without it nothing of the seeds is compiled in.
template <typename ElemT, bool kGrouped, bool kUsesState0, bool kUsesState1, bool kSeeded = false>
struct EntryPlace {
  static_assert(!kSeeded, "only a grouped walk has a seed per table");
  __device__ __forceinline__ ElemT* Table(ElemT* table) const { return table; }
  __device__ __forceinline__ float* State0(float* state0) const { return state0; }
  __device__ __forceinline__ float* State1(float* state1) const { return state1; }
};
template <typename ElemT, bool kUsesState0, bool kUsesState1, bool kSeeded>
struct EntryPlace<ElemT, true, kUsesState0, kUsesState1, kSeeded> : EntrySeed<kSeeded> {
  //! Where the seeds begin in the staged words, in units of T (after the + 1 of row_base).
  static constexpr int kSeedPlane = 2 + (kUsesState0 ? 1 : 0) + (kUsesState1 ? 1 : 0);
  GlobalRowPtr<ElemT> table;
  GlobalRowPtr<float> state0, state1;
  __device__ __forceinline__ ElemT* Table(ElemT*) const { return (ElemT*)table; }
  __device__ __forceinline__ float* State0(float*) const { return (float*)state0; }
  __device__ __forceinline__ float* State1(float*) const { return (float*)state1; }

  //! The group's words from device memory into LDS (GroupedLdsWords), by the whole workgroup, with the barrier.  Every
  //! thread of the workgroup must call it.
  static __device__ __forceinline__ void Stage(int64_t* words, const GroupedTablesOf<true, kSeeded>& g) {
    const int T = g.num_tables;
    for (int i = threadIdx.x; i <= T; i += kUpdateBlockThreads) words[i] = g.row_base[i];
    for (int i = threadIdx.x; i < T; i += kUpdateBlockThreads) {
      words[T + 1 + i] = static_cast<int64_t>(reinterpret_cast<uintptr_t>(g.tables[i]));
      if constexpr (kUsesState0) words[2 * T + 1 + i] = static_cast<int64_t>(reinterpret_cast<uintptr_t>(g.state0[i]));
      if constexpr (kUsesState1)
        words[(kUsesState0 ? 3 : 2) * T + 1 + i] = static_cast<int64_t>(reinterpret_cast<uintptr_t>(g.state1[i]));
      if constexpr (kSeeded) words[kSeedPlane * T + 1 + i] = static_cast<int64_t>(g.seeds[i]);
    }
    __syncthreads();
  }

  //! The table t with row_base[t] <= row < row_base[t + 1], by binary search over the staged row_base (the LAST such t:
  //! a table without rows owns nothing); `row` becomes the row inside that table.  LDS reads only: they are counted
  //! apart from the global loads in flight and do not wait for them.  Any `row` gives a t in [0, T).
  __device__ __forceinline__ void Resolve(const int64_t* words, const int T, int64_t& row) {
    int t = 0;
    for (int n = T; n > 1;) {
      const int half = n >> 1;
      if (words[t + half] <= row) t += half;
      n -= half;
    }
    row -= words[t];
    table = (GlobalRowPtr<ElemT>)reinterpret_cast<ElemT*>(static_cast<uintptr_t>(words[T + 1 + t]));
    if constexpr (kUsesState0)
      state0 = (GlobalRowPtr<float>)reinterpret_cast<float*>(static_cast<uintptr_t>(words[2 * T + 1 + t]));
    if constexpr (kUsesState1)
      state1 = (GlobalRowPtr<float>)reinterpret_cast<float*>(
          static_cast<uintptr_t>(words[(kUsesState0 ? 3 : 2) * T + 1 + t]));
    if constexpr (kSeeded) this->seed = static_cast<uint64_t>(words[kSeedPlane * T + 1 + t]);
  }
};

/**
 * @brief The one walk over the named rows: table[ids[k], :] and the state of row ids[k] <- rule(table[ids[k], :],
 * rows[k, :]) for every valid entry k.  The body of both kernels below.
 *
 * state0 / state1: the rule's kStates per-element tensors [rows, width], then (kRowState) its per-row words [rows].
 * kPlaced: entry k's state -- the per-element packs and the row word -- is addressed by state_ids[k] instead of ids[k];
 * the weights still go by ids[k].  That is what a state plane behind the row cache needs (row_cache.hpp): one translated
 * id cannot reach both the cached weights and the cached state.  A separate instantiation: without kPlaced nothing of
 * state_ids is compiled in.
 * kPlacedTwice (with kPlaced, a rule with a state1): state0 still goes by state_ids[k], but state1 -- the second
 * per-element tensor, or the row words of a rule that keeps them there -- goes by state1_ids[k].  That is what the Adam
 * family behind the cache needs: exp_avg and exp_avg_sq are two allocations, each with a cached plane a whole number of
 * ITS rows away, so their row offsets differ (and, row-wise, their row sizes: 4 * width against 4 bytes).  Again a
 * separate instantiation: without kPlacedTwice nothing of state1_ids is compiled in.
 * kNamed (with kStochastic): the rounding bits of entry k are those of (seed, step, row_names[k], column) instead of
 * (seed, step, ids[k], column); weights and states are addressed as without it.  That is what stochastic rounding behind
 * the cache needs: the bits belong to the TABLE ROW, and a translated id -- a slot plus a plane's row offset -- is not
 * one, so the walk carries the table rows next to the placed ids.  A placed stochastic walk must therefore be named.
 * The names are loaded with the ids, before the row data, and the Philox calls stay where they are (kChunks >= 1: while
 * the row loads are in flight).  Again a separate instantiation: without kNamed nothing of row_names is compiled in.
 * kGrouped (never with kPlaced or kNamed): the tables are `grouped.num_tables` SEPARATE tensors and ids[k] is
 * a global row of the tables laid end to end (grouped_backward.hpp's keys).  `table`, `state0` and `state1` are not read;
 * entry k's table t is the one with row_base[t] <= ids[k] < row_base[t + 1], its weights are at tables[t] + (ids[k] -
 * row_base[t]) * width and each of its state planes at states[t] + (ids[k] - row_base[t]) * (width, or 1 for the row
 * words).  The workgroup stages row_base and the base pointers in LDS once (GroupedLdsWords of dynamic LDS); an entry is
 * then resolved with LDS reads alone (EntryPlace::Resolve), which with kChunks >= 1 happens after the entry's gradient
 * loads are issued: LDS reads have a counter of their own, so the search does not wait for the rows in flight, and a
 * search through global memory would (loads return in order).  The pointers stay in a global-address-space type, so
 * row traffic is global_load / global_store as in every other walk.  Again a separate instantiation: without kGrouped
 * every accessor of EntryPlace hands its argument back and nothing of `grouped` is compiled in.
 * kGrouped with kStochastic: the rounding bits of entry k are those of (grouped.seeds[t], step, ids[k] - row_base[t],
 * column) -- the bits of a single-table stochastic step on table t with seed seeds[t]; rounding.seed is not read.  The
 * seeds are staged in LDS behind the pointers and Resolve hands an entry's seed back with its pointers, so the order of a
 * kChunks >= 1 iteration stays: gradient loads, Resolve, table / state loads, then Philox while they are in flight.
 * kEntries entries are in flight per group: 2 when a lane holds one slice per entry (kChunks == 1), else 1.  With the
 * two moment packs of an Adam slice next to its weights and gradient, two entries take 32 (fp32) to 48 (16-bit)
 * registers of row data per lane: every kChunks == 1 instantiation stays free of scratch and at or above 4 waves per
 * SIMD (profiles/sparse_adam_kernel_resources.txt; the four-slice Adam bodies of the 16-bit types run at 2).
 */
template <typename ElemT, typename IndexT, int N, int kChunks, int kEntries, bool kStochastic, bool kPlaced = false,
          bool kPlacedTwice = false, bool kNamed = false, bool kGrouped = false, typename RuleT>
__device__ __forceinline__ void WalkNamedRows(const IndexT* __restrict__ ids, const ElemT* __restrict__ rows,
                                              ElemT* __restrict__ table, float* __restrict__ state0,
                                              float* __restrict__ state1, const int width, const int lanes_per_row,
                                              const int group, const int64_t piece_rows, const int pieces,
                                              const UpdateCounts& counts, const UpdateRounding<kStochastic>& rounding,
                                              const RuleT& rule, const int64_t* __restrict__ state_ids = nullptr,
                                              const int64_t* __restrict__ state1_ids = nullptr,
                                              const int64_t* __restrict__ row_names = nullptr,
                                              const GroupedTablesOf<kGrouped, kStochastic>& grouped =
                                                  GroupedTablesOf<kGrouped, kStochastic>()) {
  static_assert(!kStochastic || sizeof(ElemT) == 2, "stochastic rounding is for the 16-bit table types");
  static_assert(!kGrouped || (!kPlaced && !kNamed), "a grouped walk is neither placed nor named");
  static_assert(!kNamed || kStochastic, "row names name rounding bits: only a stochastic walk carries them");
  static_assert(!(kPlaced && kStochastic) || kNamed, "a placed, stochastic walk must be named");
  static_assert(!kPlacedTwice || (kPlaced && RuleT::kStates >= 1), "a second placed id is for a rule with a state1");
  static_assert(kEntries == 1 || (kEntries == 2 && kChunks == 1), "two entries in flight: one slice per lane");
  using RoundT = SliceRounding<ElemT, N, kStochastic>;
  constexpr int kStates = RuleT::kStates;
  constexpr bool kRowState = RuleT::kRowState;
  constexpr int kHeld = kStates > 0 ? kStates : 1;
  constexpr int kSlices = kChunks == 0 ? 1 : kChunks;
  // where an entry's weights and state live: the walk's own tensors, or (kGrouped) those of the entry's table
  using PlaceT = EntryPlace<ElemT, kGrouped, kStates >= 1 || kRowState, kStates == 2 || (kStates == 1 && kRowState),
                            kGrouped && kStochastic>;
  // the tensor of the row words (only read if kRowState)
  const auto row_words_at = [&](const PlaceT& at) { return kStates == 0 ? at.State0(state0) : at.State1(state1); };
  // the row of an entry's row word: it lives in state0 and goes by state0's row, or in state1 and goes by state1's
  const auto word_row = [](const int64_t table_row, const int64_t placed_row, const int64_t placed1_row) {
    if constexpr (kStates == 0) return StateRow<kPlaced>(table_row, placed_row);
    else return State1Row<kPlaced, kPlacedTwice>(table_row, placed_row, placed1_row);
  };
  uint64_t seed = 0, round_step = 0;
  if constexpr (kStochastic) {
    if constexpr (!kGrouped) seed = rounding.seed;
    round_step = rounding.step_word != nullptr ? static_cast<uint64_t>(*rounding.step_word) : rounding.step;
  }
  // the seed of an entry's rounding bits: the walk's, or (kGrouped) that of the entry's table
  const auto seed_at = [&](const PlaceT& at) {
    if constexpr (kGrouped && kStochastic) return at.seed;
    else return seed;
  };
  const int64_t* group_words = nullptr;   // (kGrouped: row_base and the base pointers, staged in LDS)
  int num_tables = 0;
  if constexpr (kGrouped) {
    extern __shared__ int64_t grouped_lds_words[];
    PlaceT::Stage(grouped_lds_words, grouped);
    group_words = grouped_lds_words;
    num_tables = grouped.num_tables;
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
      // where entry u's state lives: row r[u] like the weights, or (kPlaced) a row of its own.  (Plain values handed to
      // StateRow, nothing that takes the address of r[]: the instantiations without kPlaced compile to what they were.)
      int64_t placed[kEntries];
#pragma unroll
      for (int u = 0; u < kEntries; ++u) {
        if constexpr (kPlaced) placed[u] = live[u] ? state_ids[base + k + u * stride] : 0;
        else placed[u] = 0;
      }
      int64_t placed1[kEntries];   // (kPlacedTwice: where entry u's state1 lives)
#pragma unroll
      for (int u = 0; u < kEntries; ++u) {
        if constexpr (kPlacedTwice) placed1[u] = live[u] ? state1_ids[base + k + u * stride] : 0;
        else placed1[u] = 0;
      }
      int64_t named[kEntries];     // (kNamed: the row that names entry u's rounding bits)
#pragma unroll
      for (int u = 0; u < kEntries; ++u) {
        if constexpr (kNamed) named[u] = live[u] ? row_names[base + k + u * stride] : 0;
        else named[u] = 0;
      }
      if constexpr (kChunks == 0) {
        // any width: slices lane, lane + group, ... one after the other (a rule with a row word reads the gradient row
        // twice, the second time out of the cache it has just been loaded into)
        const ElemT* g_row = RowPtr(rows, base + k, width);
        PlaceT at;
        if constexpr (kGrouped) at.Resolve(group_words, num_tables, r[0]);   // (r[0]: from here the row in its table)
        float* const row_words = row_words_at(at);
        ElemT* w_row = const_cast<ElemT*>(RowPtr(at.Table(table), r[0], width));
        float row = 0.f;
        if constexpr (kRowState) {
          const float before = row_words[word_row(r[0], placed[0], placed1[0])];
          float sum = 0.f;
          for (int c = lane; c < lanes_per_row; c += group) sum = AddSquares(sum, LoadPack<ElemT, N>(g_row + c * N));
          row = rule.Row(row_words + word_row(r[0], placed[0], placed1[0]), before, GroupSum(sum, group), width, lane == 0);
        }
        for (int c = lane; c < lanes_per_row; c += group) {
          const Pack<ElemT, N> g = kRowState ? LoadPack<ElemT, N>(g_row + c * N) : LoadPackStreaming<ElemT, N>(g_row + c * N);
          const Pack<ElemT, N> w = LoadPack<ElemT, N>(w_row + c * N);
          StatePack<N> s[kHeld];
          LoadStates<kStates>(s, at.State0(state0), at.State1(state1), RowElems(StateRow<kPlaced>(r[0], placed[0]), width) + c * N,
                              RowElems(State1Row<kPlaced, kPlacedTwice>(r[0], placed[0], placed1[0]), width) + c * N);
          RoundT round;
          if constexpr (kStochastic) round = RoundT(seed_at(at), round_step, RoundingRow<kNamed>(r[0], named[0]), c * N);
          StorePack<ElemT, N>(w_row + c * N, rule.Slice(w, g, s, row, round));
          StoreStates<kStates>(s, at.State0(state0), at.State1(state1), RowElems(StateRow<kPlaced>(r[0], placed[0]), width) + c * N,
                               RowElems(State1Row<kPlaced, kPlacedTwice>(r[0], placed[0], placed1[0]), width) + c * N);
        }
      } else {
        Pack<ElemT, N> g[kEntries][kSlices], w[kEntries][kSlices];
        StatePack<N> s[kEntries][kSlices][kHeld];
        bool has[kEntries][kSlices];
        float row_word[kEntries];
        RoundT round[kEntries][kSlices];
        PlaceT at[kEntries];
        if constexpr (kGrouped) {
          // the gradient rows need nothing but k: their loads go first, and every entry's table is found while they are
          // in flight (r[u]: from here the row in its table)
#pragma unroll
          for (int u = 0; u < kEntries; ++u)
#pragma unroll
            for (int c = 0; c < kSlices; ++c) {
              has[u][c] = live[u] && lane + c * group < lanes_per_row;
              if (has[u][c])
                g[u][c] = LoadPackStreaming<ElemT, N>(RowPtr(rows, base + k + u * stride, width) + (lane + c * group) * N);
            }
#pragma unroll
          for (int u = 0; u < kEntries; ++u) at[u].Resolve(group_words, num_tables, r[u]);
        }
#pragma unroll
        for (int u = 0; u < kEntries; ++u) {
          if constexpr (kRowState)
            row_word[u] = live[u] ? row_words_at(at[u])[word_row(r[u], placed[u], placed1[u])] : 0.f;
#pragma unroll
          for (int c = 0; c < kSlices; ++c) {
            const int col = (lane + c * group) * N;
            if constexpr (!kGrouped) has[u][c] = live[u] && lane + c * group < lanes_per_row;
            if (has[u][c]) {
              if constexpr (!kGrouped)
                g[u][c] = LoadPackStreaming<ElemT, N>(RowPtr(rows, base + k + u * stride, width) + col);
              w[u][c] = LoadPack<ElemT, N>(RowPtr(at[u].Table(table), r[u], width) + col);
              LoadStates<kStates>(s[u][c], at[u].State0(state0), at[u].State1(state1),
                                  RowElems(StateRow<kPlaced>(r[u], placed[u]), width) + col,
                                  RowElems(State1Row<kPlaced, kPlacedTwice>(r[u], placed[u], placed1[u]), width) + col);
            }
          }
        }
        if constexpr (kStochastic) {
          // the random bits need nothing that was loaded: they are computed while the loads are in flight
#pragma unroll
          for (int u = 0; u < kEntries; ++u)
#pragma unroll
            for (int c = 0; c < kSlices; ++c)
              if (has[u][c])
                round[u][c] = RoundT(seed_at(at[u]), round_step, RoundingRow<kNamed>(r[u], named[u]),
                                     (lane + c * group) * N);
        }
#pragma unroll
        for (int u = 0; u < kEntries; ++u) {
          float row = 0.f;
          if constexpr (kRowState) {
            // (a group whose second entry is past the count still takes part in the butterfly: its lanes are active)
            float sum = 0.f;
#pragma unroll
            for (int c = 0; c < kSlices; ++c)
              if (has[u][c]) sum = AddSquares(sum, g[u][c]);
            sum = GroupSum(sum, group);
            if (live[u])
              row = rule.Row(row_words_at(at[u]) + word_row(r[u], placed[u], placed1[u]), row_word[u], sum, width,
                             lane == 0);
          }
#pragma unroll
          for (int c = 0; c < kSlices; ++c) {
            if (!has[u][c]) continue;
            const int col = (lane + c * group) * N;
            ElemT* w_at = const_cast<ElemT*>(RowPtr(at[u].Table(table), r[u], width)) + col;
            StorePack<ElemT, N>(w_at, rule.Slice(w[u][c], g[u][c], s[u][c], row, round[u][c]));
            StoreStates<kStates>(s[u][c], at[u].State0(state0), at[u].State1(state1),
                                 RowElems(StateRow<kPlaced>(r[u], placed[u]), width) + col,
                                  RowElems(State1Row<kPlaced, kPlacedTwice>(r[u], placed[u], placed1[u]), width) + col);
          }
        }
      }
    }
  }
}

/**
 * @brief table[ids[k], :] (and its state) <- rule(table[ids[k], :], rows[k, :]) for every valid entry k.
 *
 * Launch: 1-D grid of kUpdateBlockThreads-thread workgroups, `group` (a power of two <= 64) lanes per entry,
 * lanes_per_row = width / N slices per row; kChunks >= 1 needs lanes_per_row <= kChunks * group.
 * Entries: `pieces` blocks of `piece_rows` entries, entry j of piece p valid iff j < count(p).
 * kStochastic (16-bit ElemT only): the stores round stochastically with the bits of (rounding.seed, step).
 */
template <typename ElemT, typename IndexT, int N, UpdateRule kRule, int kChunks, bool kStochastic = false>
__global__ void __launch_bounds__(kUpdateBlockThreads)
    SparseRowUpdateKernel(const IndexT* __restrict__ ids, const ElemT* __restrict__ rows, ElemT* __restrict__ table,
                          float* __restrict__ state, const int width, const int lanes_per_row, const int group,
                          const int64_t piece_rows, const int pieces, const UpdateCounts counts, const float lr_value,
                          const float* __restrict__ lr_word, const float eps,
                          const UpdateRounding<kStochastic> rounding = UpdateRounding<kStochastic>()) {
  const UpdateStep<kRule> rule{lr_word != nullptr ? *lr_word : lr_value, eps};
  WalkNamedRows<ElemT, IndexT, N, kChunks, kChunks == 1 ? 2 : 1, kStochastic>(
      ids, rows, table, state, nullptr, width, lanes_per_row, group, piece_rows, pieces, counts, rounding, rule);
}

//! The same step with the state in a place of its own: entry k's weights at table[ids[k], :], its state at row
//! state_ids[k] of `state` (WalkNamedRows' kPlaced).  Round to nearest; SparseRowUpdateNamedKernel rounds stochastically.
template <typename ElemT, typename IndexT, int N, UpdateRule kRule, int kChunks>
__global__ void __launch_bounds__(kUpdateBlockThreads)
    SparseRowUpdatePlacedKernel(const IndexT* __restrict__ ids, const int64_t* __restrict__ state_ids,
                                const ElemT* __restrict__ rows, ElemT* __restrict__ table, float* __restrict__ state,
                                const int width, const int lanes_per_row, const int group, const int64_t piece_rows,
                                const int pieces, const UpdateCounts counts, const float lr_value,
                                const float* __restrict__ lr_word, const float eps) {
  static_assert(kRule != UpdateRule::kSgd, "SGD has no state to place");
  const UpdateStep<kRule> rule{lr_word != nullptr ? *lr_word : lr_value, eps};
  WalkNamedRows<ElemT, IndexT, N, kChunks, kChunks == 1 ? 2 : 1, false, true>(
      ids, rows, table, state, nullptr, width, lanes_per_row, group, piece_rows, pieces, counts, UpdateRounding<false>(),
      rule, state_ids);
}

/**
 * @brief The stochastic step behind the row cache: entry k's weights at table[ids[k], :], its state (a rule that has
 * one) at row state_ids[k] of `state`, and its rounding bits those of table row row_names[k] (WalkNamedRows' kNamed,
 * with kPlaced for every rule but SGD, which has no state and takes state_ids == nullptr).  16-bit tables only.  Same
 * launch and the same entries in flight as SparseRowUpdateKernel.
 */
template <typename ElemT, typename IndexT, int N, UpdateRule kRule, int kChunks>
__global__ void __launch_bounds__(kUpdateBlockThreads)
    SparseRowUpdateNamedKernel(const IndexT* __restrict__ ids, const int64_t* __restrict__ state_ids,
                               const int64_t* __restrict__ row_names, const ElemT* __restrict__ rows,
                               ElemT* __restrict__ table, float* __restrict__ state, const int width,
                               const int lanes_per_row, const int group, const int64_t piece_rows, const int pieces,
                               const UpdateCounts counts, const float lr_value, const float* __restrict__ lr_word,
                               const float eps, const UpdateRounding<true> rounding) {
  const UpdateStep<kRule> rule{lr_word != nullptr ? *lr_word : lr_value, eps};
  WalkNamedRows<ElemT, IndexT, N, kChunks, kChunks == 1 ? 2 : 1, true, kRule != UpdateRule::kSgd, false, true>(
      ids, rows, table, state, nullptr, width, lanes_per_row, group, piece_rows, pieces, counts, rounding, rule,
      state_ids, nullptr, row_names);
}

/**
 * @brief The same step on a GROUP of separate table tensors: ids[k] is a global row of the tables laid end to end, and
 * entry k updates row ids[k] - row_base[t] of tables[t] and of that table's state tensor (WalkNamedRows' kGrouped).
 * Round to nearest.  Same launch as SparseRowUpdateKernel, plus GroupedLdsWords(num_tables, the rule's state tensors)
 * * 8 bytes of dynamic LDS.  grouped.state0 holds the bases of the rule's one state tensor (nullptr for SGD).
 */
template <typename ElemT, typename IndexT, int N, UpdateRule kRule, int kChunks, int kEntriesInFlight>
__global__ void __launch_bounds__(kUpdateBlockThreads)
    SparseRowUpdateGroupedKernel(const IndexT* __restrict__ ids, const ElemT* __restrict__ rows,
                                 const GroupedTables<true> grouped, const int width, const int lanes_per_row,
                                 const int group, const int64_t piece_rows, const int pieces, const UpdateCounts counts,
                                 const float lr_value, const float* __restrict__ lr_word, const float eps) {
  const UpdateStep<kRule> rule{lr_word != nullptr ? *lr_word : lr_value, eps};
  WalkNamedRows<ElemT, IndexT, N, kChunks, kEntriesInFlight, false, false, false, false, true>(
      ids, rows, nullptr, nullptr, nullptr, width, lanes_per_row, group, piece_rows, pieces, counts,
      UpdateRounding<false>(), rule, nullptr, nullptr, nullptr, grouped);
}

/**
 * @brief The grouped step with stochastic rounding (16-bit tables): as SparseRowUpdateGroupedKernel, and the one rounding
 * of entry k draws the bits of (grouped.seeds[t], step, ids[k] - row_base[t], column), t the entry's table: those of
 * SparseRowUpdateKernel<.., kStochastic> on table t alone with seed seeds[t].  rounding.step / step_word are read,
 * rounding.seed is not.  GroupedLdsWords(num_tables, the rule's state tensors, true) * 8 bytes of dynamic LDS.
 */
template <typename ElemT, typename IndexT, int N, UpdateRule kRule, int kChunks, int kEntriesInFlight>
__global__ void __launch_bounds__(kUpdateBlockThreads)
    SparseRowUpdateGroupedStochasticKernel(const IndexT* __restrict__ ids, const ElemT* __restrict__ rows,
                                           const GroupedSeededTables grouped, const int width,
                                           const int lanes_per_row, const int group, const int64_t piece_rows,
                                           const int pieces, const UpdateCounts counts, const float lr_value,
                                           const float* __restrict__ lr_word, const float eps,
                                           const UpdateRounding<true> rounding) {
  static_assert(sizeof(ElemT) == 2, "stochastic rounding is for the 16-bit table types");
  const UpdateStep<kRule> rule{lr_word != nullptr ? *lr_word : lr_value, eps};
  WalkNamedRows<ElemT, IndexT, N, kChunks, kEntriesInFlight, true, false, false, false, true>(
      ids, rows, nullptr, nullptr, nullptr, width, lanes_per_row, group, piece_rows, pieces, counts, rounding, rule,
      nullptr, nullptr, nullptr, grouped);
}

}  // namespace detail
}  // namespace cuembed

#endif  // CUEMBED_INCLUDE_SPARSE_UPDATE_KERNELS_HPP_
