// MI355X (gfx950 / CDNA4) row cache -- host API (an extension: the reference lists an embedding cache as future work).
//
//   cuembed::RowCachePrefetch<IndexT>(cache, indices, nnz, counts, for_update, work, &lwork, stream)
//   cuembed::RowCacheFlush(cache, stream)
//
// make a device buffer of num_sets x 64 rows a set-associative LRU write-back cache of a table that lives outside this
// GPU's HBM.  The cache buffer differs from the table by a whole number of rows, so TranslateIndicesForRowCache +
// EmbeddingForward (or SparseRowUpdate) on the TABLE's base pointer reach the cached rows unchanged.  An optimizer's fp32
// state can ride on the same slots as a second plane (RowCache::state): it is translated with its own row offset and
// handed to SparseRowUpdate as `state_ids`.  The Adam family has two such planes (RowCache::state2): one launch of
// TranslateIndicesForRowCachePlanes translates the ids for all three and SparseRowAdam takes the two state ids.
// Everything is stream-ordered and nothing is read back; the kernels and the state they keep are in row_cache_kernels.hpp.
#ifndef CUEMBED_INCLUDE_ROW_CACHE_HPP_
#define CUEMBED_INCLUDE_ROW_CACHE_HPP_

#include <hip/hip_runtime.h>

#include <cassert>
#include <cstdint>

#include "cuembed/include/cuembed_assert.hpp"
#include "cuembed/include/device_shape.hpp"
#ifdef CUEMBED_ROW_CACHE_SORT_IN_LIBRARY
// (inside libcuembed_amd.so the sort's kernels are compiled once, in the index transforms' translation unit, and
// reached through the C ABI; a header-only user gets them from index_transforms.hpp)
#include "cuembed_amd.h"
#else
#include "cuembed/include/index_transforms.hpp"
#endif
#include "cuembed/include/row_cache_kernels.hpp"
#include "cuembed/include/sparse_update.hpp"

namespace cuembed {

//! The cache: where the table and the cached rows live, and the device state of row_cache_kernels.hpp.
struct RowCache {
  void* table = nullptr;         //!< [num_rows, row_bytes], device-accessible (pinned host memory)
  void* cache_rows = nullptr;    //!< [num_sets * 64, row_bytes] in HBM; (cache_rows - table) % row_bytes == 0
  int64_t row_bytes = 0;         //!< a multiple of 4
  int64_t num_rows = 0;
  int num_sets = 0;
  int64_t* tags = nullptr;       //!< [num_sets * 64], -1 = empty
  uint32_t* stamps = nullptr;    //!< [num_sets * 64], 0 = never used
  uint8_t* dirty = nullptr;      //!< [num_sets * 64]
  int32_t* slot_of_row = nullptr;  //!< [num_rows], -1 = not cached
  unsigned long long* words = nullptr;   //!< [kCacheWords]; words[kCacheClock] starts at 1
  //! The optional state plane: fp32 optimizer state that rides on the cache slots and moves with its row on every
  //! fill (forward-only fills too: a later for_update hit uses the cached state), dirty eviction and flush.
  float* state = nullptr;        //!< [num_rows, width] (Adagrad) or [num_rows] (row-wise Adagrad), pinned host memory
  float* state_cache = nullptr;  //!< [num_sets * 64, ...] in HBM; (state_cache - state) % state_row_bytes == 0
  int64_t state_row_bytes = 0;   //!< 0 = no state plane; else 4 * width or 4
  //! The optional SECOND state plane, moved exactly like the first (the Adam family: `state` is exp_avg, `state2`
  //! exp_avg_sq).  Only together with the first.
  float* state2 = nullptr;        //!< [num_rows, width] (Adam) or [num_rows] (row-wise Adam), pinned host memory
  float* state2_cache = nullptr;  //!< [num_sets * 64, ...] in HBM; (state2_cache - state2) % state2_row_bytes == 0
  int64_t state2_row_bytes = 0;   //!< 0 = no second plane; else 4 * width or 4
};

//! Which lookups of `indices` count: exactly one source, as for SparseRowUpdate.
struct RowCacheCounts {
  int64_t num_valid = -1;        //!< >= 0: host-known
  const void* count = nullptr;   //!< one int32 word on the device, or ...
  bool count_is_int64 = false;   //!< ... one int64 word
  const void* last_id = nullptr; //!< one IndexT word on the device: count = *last_id + 1
};

namespace detail {

inline int BitsFor(const int64_t values) {   // bits that hold every value of [0, values)
  int bits = 0;
  while (bits < 62 && (int64_t{1} << bits) < values) ++bits;
  return bits;
}

//! The library's sort on int64 keys of key_bits bits (work == nullptr: the bytes it needs to *lwork).  `order`
//! receives the positions the sort carries along; nothing reads them.
inline void CacheSortKeys(const int64_t* keys, const int n, int64_t* sorted, int64_t* order, char* work, size_t* lwork,
                          const int key_bits, const hipStream_t stream) {
#ifdef CUEMBED_ROW_CACHE_SORT_IN_LIBRARY
  cuembed_transpose_fixed_hotness(keys, nullptr, n, 1, CUEMBED_I64, CUEMBED_F32, sorted, order, nullptr, work, lwork,
                                  key_bits, reinterpret_cast<cuembed_stream_t>(stream));
#else
  TransposeFixedHotness<int64_t, float>(keys, nullptr, n, 1, sorted, order, nullptr, work, lwork, stream, key_bits);
#endif
}

//! The library's run-head scan: runs[i] = dense id of the run of sorted key i (work == nullptr: the bytes to *lwork).
inline void CacheRunIds(const int64_t* sorted, const int n, int64_t* runs, char* work, size_t* lwork,
                        const hipStream_t stream) {
#ifdef CUEMBED_ROW_CACHE_SORT_IN_LIBRARY
  cuembed_compute_compressed_grad_indices(sorted, n, CUEMBED_I64, runs, work, lwork,
                                          reinterpret_cast<cuembed_stream_t>(stream));
#else
  ComputeCompressedGradIndices<int64_t>(sorted, n, runs, work, lwork, stream);
#endif
}

//! The combined (set, row) sort key: row in the low row_bits, set above, one more bit for the sentinel.
struct CacheKeyLayout {
  int row_bits, key_bits;
  int64_t sentinel;
  CacheKeyLayout(const int64_t num_rows, const int num_sets) {
    row_bits = BitsFor(num_rows) < 1 ? 1 : BitsFor(num_rows);
    const int set_bits = BitsFor(num_sets);
    CUEMBED_ASSERT(row_bits + set_bits + 1 <= 62);
    key_bits = row_bits + set_bits + 1;
    sentinel = int64_t{1} << (row_bits + set_bits);
  }
};

//! The pieces of a prefetch's workspace.
struct RowCachePlan {
  size_t keys, sorted, order, moves, sort, sort_bytes, total;
  RowCachePlan(const int64_t nnz, const CacheKeyLayout& layout) {
    const size_t n = static_cast<size_t>(nnz > 0 ? nnz : 0);
    sort_bytes = 0;
    CacheSortKeys(nullptr, static_cast<int>(n), nullptr, nullptr, nullptr, &sort_bytes, layout.key_bits, 0);
    size_t scan_bytes = 0;   // (the scan runs after the sort, in the same bytes)
    CacheRunIds(nullptr, static_cast<int>(n), nullptr, nullptr, &scan_bytes, 0);
    if (scan_bytes > sort_bytes) sort_bytes = scan_bytes;
    size_t at = 0;
    const auto take = [&](size_t bytes) { const size_t here = at; at += (bytes + 255) / 256 * 256; return here; };
    keys = take(n * sizeof(int64_t));
    sorted = take(n * sizeof(int64_t));
    order = take(n * sizeof(int64_t));
    moves = take(n * sizeof(CacheMove));
    sort = take(sort_bytes);
    total = at;
  }
};

inline void CheckRowCache(const RowCache& c) {
  CUEMBED_ASSERT(c.num_sets >= 1 && c.num_sets <= (1 << 24));
  CUEMBED_ASSERT(c.num_rows >= 1);
  CUEMBED_ASSERT(c.row_bytes > 0 && c.row_bytes % 4 == 0);
  CUEMBED_ASSERT(c.table != nullptr && c.cache_rows != nullptr);
  CUEMBED_ASSERT(reinterpret_cast<uintptr_t>(c.table) % 4 == 0);
  CUEMBED_ASSERT((reinterpret_cast<intptr_t>(c.cache_rows) - reinterpret_cast<intptr_t>(c.table)) % c.row_bytes == 0);
  CUEMBED_ASSERT(c.tags != nullptr && c.stamps != nullptr && c.dirty != nullptr && c.slot_of_row != nullptr &&
                 c.words != nullptr);
  if (c.state_row_bytes != 0) {
    CUEMBED_ASSERT(c.state_row_bytes > 0 && c.state_row_bytes % 4 == 0);
    CUEMBED_ASSERT(c.state != nullptr && c.state_cache != nullptr);
    CUEMBED_ASSERT(reinterpret_cast<uintptr_t>(c.state) % 4 == 0);
    CUEMBED_ASSERT((reinterpret_cast<intptr_t>(c.state_cache) - reinterpret_cast<intptr_t>(c.state)) %
                       c.state_row_bytes == 0);
  }
  if (c.state2_row_bytes != 0) {
    CUEMBED_ASSERT(c.state_row_bytes != 0);   // a second plane only next to a first
    CUEMBED_ASSERT(c.state2_row_bytes > 0 && c.state2_row_bytes % 4 == 0);
    CUEMBED_ASSERT(c.state2 != nullptr && c.state2_cache != nullptr);
    CUEMBED_ASSERT(reinterpret_cast<uintptr_t>(c.state2) % 4 == 0);
    CUEMBED_ASSERT((reinterpret_cast<intptr_t>(c.state2_cache) - reinterpret_cast<intptr_t>(c.state2)) %
                       c.state2_row_bytes == 0);
  }
}

//! The mover on `capacity` entries of one plane (`home`: the plane's rows outside the cache, `cached`: its slots):
//! 16-byte lanes wherever the row size and the plane's base allow, 8 or 4 otherwise (the cached rows are whole rows
//! away from the home rows, so they are aligned alike).  A 4-byte row is one lane.
inline void LaunchPlaneMove(const RowCache& c, void* home, void* cached, const int64_t row_bytes, const bool commit,
                            const CacheMove* moves, const int64_t capacity, const hipStream_t stream) {
  const uintptr_t bits = reinterpret_cast<uintptr_t>(home) | static_cast<uintptr_t>(row_bytes);
  const int bytes = bits % 16 == 0 ? 16 : (bits % 8 == 0 ? 8 : 4);
  const int lanes_per_row = static_cast<int>(row_bytes / bytes);
  const UpdateShape s = PlanUpdate(lanes_per_row, capacity, CurrentDeviceShape());
#define CUEMBED_MOVE(LANE)                                                                                       \
  CacheMoveKernel<LANE><<<dim3(s.grid), dim3(kCacheBlockThreads), 0, stream>>>(                                 \
      moves, capacity, c.tags, c.dirty, static_cast<char*>(home), static_cast<char*>(cached), row_bytes,         \
      lanes_per_row, s.group, commit ? 1 : 0, c.words)
  if (bytes == 16) CUEMBED_MOVE(uint4);
  else if (bytes == 8) CUEMBED_MOVE(uint2);
  else CUEMBED_MOVE(uint32_t);
#undef CUEMBED_MOVE
}

//! The row exchange of every plane: the second state plane, the first, then the table's, in stream order -- the last
//! launch alone commits: it clears the dirty bytes of a flush and counts its write-backs (CacheMoveKernel).
inline void LaunchCacheMove(const RowCache& c, const CacheMove* moves, const int64_t capacity, const hipStream_t stream) {
  if (capacity <= 0) return;
  if (c.state2_row_bytes != 0)
    LaunchPlaneMove(c, c.state2, c.state2_cache, c.state2_row_bytes, false, moves, capacity, stream);
  if (c.state_row_bytes != 0) LaunchPlaneMove(c, c.state, c.state_cache, c.state_row_bytes, false, moves, capacity, stream);
  LaunchPlaneMove(c, c.table, c.cache_rows, c.row_bytes, true, moves, capacity, stream);
}

}  // namespace detail

//! Bytes of workspace a prefetch of up to nnz lookups needs.
inline size_t RowCacheWorkspaceBytes(const int64_t nnz, const int64_t num_rows, const int num_sets) {
  return detail::RowCachePlan(nnz, detail::CacheKeyLayout(num_rows, num_sets)).total;
}

/**
 * @brief Make the distinct table rows that the valid lookups of `indices` name resident, as far as their sets allow.
 *
 * With t the clock and D the distinct rows of the valid lookups inside [0, num_rows):
 *   1. hits first: every resident row of D gets stamp = t (and, for_update, its dirty byte): a row of this batch is
 *      never evicted by this batch;
 *   2. then the misses of each set in ascending row id: each takes the way with the smallest (stamp, way) among ways
 *      with stamp < t; if there is none the row stays uncached and the `unplaced` word is raised by one;
 *   3. placing a row stores a valid dirty victim to the table, clears the victim's slot_of_row, loads the new row from
 *      the table, and sets tag, stamp = t, slot_of_row and dirty = for_update; with a state plane
 *      (c.state_row_bytes != 0) the victim's state row is stored and the new row's state row loaded with them,
 *      whatever for_update says, and likewise the rows of a second state plane (c.state2_row_bytes != 0);
 *   4. clock += 1.
 * Lookups outside the table are ignored.  A count outside [0, nnz] counts as 0.
 *
 * Two-phase: work == nullptr stores the bytes needed to *lwork (RowCacheWorkspaceBytes) and runs nothing.  nnz is the
 * capacity of `indices` and must not exceed INT32_MAX.  Stream-ordered, no read-back.
 */
template <typename IndexT>
void RowCachePrefetch(const RowCache& c,
                      const IndexT* indices,
                      const int64_t nnz,
                      const RowCacheCounts& counts,
                      const bool for_update,
                      char* work,
                      size_t* lwork,
                      const hipStream_t stream = 0) {
  CUEMBED_ASSERT(nnz >= 0 && nnz <= INT32_MAX);
  const detail::CacheKeyLayout layout(c.num_rows, c.num_sets);
  const detail::RowCachePlan plan(nnz, layout);
  if (work == nullptr) {
    *lwork = plan.total;
    return;
  }
  assert(*lwork >= plan.total);
  detail::CheckRowCache(c);
  CUEMBED_ASSERT((counts.num_valid >= 0) + (counts.count != nullptr) + (counts.last_id != nullptr) == 1);
  CUEMBED_ASSERT(counts.num_valid <= nnz);
  if (nnz == 0 || counts.num_valid == 0) {
    detail::CacheEmptyBatchKernel<<<1, 1, 0, stream>>>(c.words);
    detail::CacheClockKernel<<<1, 1, 0, stream>>>(c.words);
    return;
  }
  CUEMBED_ASSERT(indices != nullptr);
  detail::UpdateCounts device_counts;
  device_counts.host_count = counts.num_valid >= 0 ? counts.num_valid : -1;
  device_counts.count_words = counts.count;
  device_counts.count_words_are_64 = counts.count_is_int64 ? 1 : 0;
  device_counts.last_id = counts.last_id;

  int64_t* keys = reinterpret_cast<int64_t*>(work + plan.keys);
  int64_t* sorted = reinterpret_cast<int64_t*>(work + plan.sorted);
  int64_t* order = reinterpret_cast<int64_t*>(work + plan.order);
  detail::CacheMove* moves = reinterpret_cast<detail::CacheMove*>(work + plan.moves);
  const unsigned flat = static_cast<unsigned>((nnz + detail::kCacheBlockThreads - 1) / detail::kCacheBlockThreads);
  const unsigned num_sets = static_cast<unsigned>(c.num_sets);
  const int64_t move_capacity = nnz;   // one entry per distinct row that is not resident

  detail::CacheKeysKernel<IndexT><<<flat, detail::kCacheBlockThreads, 0, stream>>>(
      indices, nnz, device_counts, c.num_rows, num_sets, layout.row_bits, layout.sentinel, keys, c.words);
  // one sort on the combined (set, row) key (the positions it carries along are not used), then the run ids of the
  // sorted keys over those positions; the distinct keys go where the unsorted ones were
  size_t sort_bytes = plan.sort_bytes;
  detail::CacheSortKeys(keys, static_cast<int>(nnz), sorted, order, work + plan.sort, &sort_bytes, layout.key_bits,
                        stream);
  int64_t* runs = order;
  int64_t* distinct = keys;
  detail::CacheRunIds(sorted, static_cast<int>(nnz), runs, work + plan.sort, &sort_bytes, stream);
  detail::CacheHitKernel<<<flat, detail::kCacheBlockThreads, 0, stream>>>(
      sorted, runs, nnz, layout.row_bits, layout.sentinel, distinct, c.slot_of_row, c.stamps, c.dirty, for_update ? 1 : 0,
      c.words);
  detail::CachePlaceKernel<<<(num_sets + detail::kCacheSetsPerBlock - 1) / detail::kCacheSetsPerBlock,
                             detail::kCacheBlockThreads, 0, stream>>>(
      distinct, runs + (nnz - 1), nnz, layout.row_bits, num_sets, c.tags, c.stamps, c.dirty, c.slot_of_row,
      for_update ? 1 : 0, moves, move_capacity, c.words);
  detail::LaunchCacheMove(c, moves, move_capacity, stream);
  detail::CacheClockKernel<<<1, 1, 0, stream>>>(c.words);
}

//! Store every dirty cached row (and its state rows) to the table and clear the dirty bytes (the same mover over all
//! slots).
inline void RowCacheFlush(const RowCache& c, const hipStream_t stream = 0) {
  detail::CheckRowCache(c);
  detail::LaunchCacheMove(c, nullptr, static_cast<int64_t>(c.num_sets) * kRowCacheWays, stream);
}

}  // namespace cuembed

#endif  // CUEMBED_INCLUDE_ROW_CACHE_HPP_
