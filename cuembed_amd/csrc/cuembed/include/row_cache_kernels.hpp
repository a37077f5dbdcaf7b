// MI355X (gfx950 / CDNA4) row cache -- the kernels (an extension: the reference lists an embedding cache as future work).
//
// A set-associative, LRU, write-back cache of table rows in HBM for a table that lives elsewhere (pinned host memory
// read over PCIe).  num_sets sets of 64 ways: ONE WAVEFRONT OWNS ONE SET, lane = way, and that is the whole
// synchronisation story -- no locks, no spin-waits, no waiting between workgroups.  State, all on the device:
//     tags   int64  [num_sets, 64]   table row held by the way, -1 = empty
//     stamps uint32 [num_sets, 64]   clock value of the way's last use, 0 = never used
//     dirty  uint8  [num_sets, 64]   the cached row is newer than the table's
//     slot_of_row int32 [rows]       set * 64 + way of a cached row, -1 otherwise (what TranslateIndicesForRowCache reads)
//     words  uint64 [kCacheWords]    clock, counters, the move list's length (CacheWord)
// One prefetch of a batch is five launches after the library's sort and run-head scan, each a plain grid with nothing
// shared between its workgroups but atomic counters:
//     CacheKeysKernel    key = (set << row_bits) | row for every valid lookup, a sentinel above all keys otherwise
//     (sort, scan)       ascending keys -- the rows of a set contiguous and ascending, duplicates adjacent -- and the
//                        dense id of every key's run (Transpose / ComputeCompressedGradIndices)
//     CacheHitKernel     flat over the sorted keys: the first key of every run goes to distinct[its dense id], and every
//                        distinct resident row gets stamp = clock (and its dirty byte)
//     CachePlaceKernel   a wavefront per set walks its segment of the DISTINCT keys, 64 per step, and places the rows
//                        that are not resident: victim = min (stamp, way) among ways with stamp < clock
//     CacheMoveKernel    flat over the move list: dirty victim cache -> table, then new row table -> cache; with a
//                        state plane (RowCache::state, ::state2) once more per plane before that, for the state rows
//                        of the same entries
//     CacheClockKernel   clock += 1
// Every loop is bounded by a kernel argument (the lookups of the batch, the ways, the lanes of a row) or by a device
// count clamped to the capacity of the buffer it walks.  Rows are addressed in 64 bits throughout.
#ifndef CUEMBED_INCLUDE_ROW_CACHE_KERNELS_HPP_
#define CUEMBED_INCLUDE_ROW_CACHE_KERNELS_HPP_

#include <hip/hip_runtime.h>

#include <cstdint>

#include "cuembed/include/sparse_update_kernels.hpp"

namespace cuembed {

constexpr int kRowCacheWays = 64;

//! The words of the cache's device state (uint64 each).
enum RowCacheWord {
  kCacheClock = 0,       //!< stamp of the running prefetch; first value 1
  kCacheHits = 1,        //!< distinct rows of a batch found resident
  kCacheMisses = 2,      //!< distinct rows of a batch not resident (placed or not)
  kCacheEvictions = 3,   //!< valid rows displaced
  kCacheWriteBacks = 4,  //!< dirty rows stored to the table (evictions and flushes)
  kCacheUnplaced = 5,    //!< misses that found no way: every way of their set was used by the same batch (sticky)
  kCacheMoveCount = 6,   //!< entries of the running prefetch's move list
  kCacheBatchCount = 7,  //!< valid lookups of the last prefetch, as resolved on the device (int64)
  kCacheOverflow = 8,    //!< raised when a device count reached the capacity of its buffer (never, by construction)
  kCacheWords = 16
};

/**
 * @brief The set of a table row: a fixed integer mix (two multiply / xor-shift rounds of the 64-bit row id) reduced to
 * [0, num_sets) by multiply-shift, so that num_sets need not be a power of two and consecutive or strided ids spread.
 *     h = row * 0x9E3779B97F4A7C15;  h ^= h >> 32;  h *= 0xD6E8FEB86659FD93;  h ^= h >> 32      (mod 2^64)
 *     set = ((h >> 32) * num_sets) >> 32
 * cuembed_amd/row_cache.py's cache_set_of is the same function on the host.
 */
__host__ __device__ inline uint32_t CacheSetOf(const int64_t row, const uint32_t num_sets) {
  uint64_t h = static_cast<uint64_t>(row) * 0x9E3779B97F4A7C15ull;
  h ^= h >> 32;
  h *= 0xD6E8FEB86659FD93ull;
  h ^= h >> 32;
  return static_cast<uint32_t>(((h >> 32) * static_cast<uint64_t>(num_sets)) >> 32);
}

namespace detail {

constexpr int kCacheBlockThreads = 256;
constexpr int kCacheSetsPerBlock = kCacheBlockThreads / kRowCacheWays;

//! One placement: row `new_row` (-1: none) goes into `slot`; the row `old_row` it displaces is stored first when
//! write_back is set.
struct CacheMove {
  int64_t new_row;
  int64_t old_row;
  int32_t slot;
  int32_t write_back;
};

//! keys[i] = (set << row_bits) | row of lookup i, or the sentinel 1 << key_bits' top bit for a lookup past the count
//! or outside the table.  Thread 0 also resets the move list and publishes the resolved count.
template <typename IndexT>
__global__ void __launch_bounds__(kCacheBlockThreads)
    CacheKeysKernel(const IndexT* __restrict__ indices, const int64_t n, const UpdateCounts counts, const int64_t num_rows,
                    const uint32_t num_sets, const int row_bits, const int64_t sentinel, int64_t* __restrict__ keys,
                    unsigned long long* __restrict__ words) {
  const int64_t count = PieceCount<IndexT>(counts, 0, n);
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kCacheBlockThreads + threadIdx.x;
  if (i == 0) {
    words[kCacheMoveCount] = 0;
    words[kCacheBatchCount] = static_cast<unsigned long long>(count);
  }
  if (i >= n) return;
  int64_t key = sentinel;
  if (i < count) {
    const int64_t r = static_cast<int64_t>(indices[i]);
    if (r >= 0 && r < num_rows) key = (static_cast<int64_t>(CacheSetOf(r, num_sets)) << row_bits) | r;
  }
  keys[i] = key;
}

//! The count word alone, for a batch without lookups.
__global__ void CacheEmptyBatchKernel(unsigned long long* __restrict__ words) {
  words[kCacheMoveCount] = 0;
  words[kCacheBatchCount] = 0;
}

//! Hits first: every distinct resident row of the batch is stamped with the clock before any way is given away, so
//! that no row of this batch is evicted by this batch.  run_of[i] is the dense id of key i's run (the run-head scan):
//! the first key of a run is copied to distinct[run_of[i]], which compacts the distinct keys in order.
__global__ void __launch_bounds__(kCacheBlockThreads)
    CacheHitKernel(const int64_t* __restrict__ keys, const int64_t* __restrict__ run_of, const int64_t n,
                   const int row_bits, const int64_t sentinel, int64_t* __restrict__ distinct,
                   const int32_t* __restrict__ slot_of_row, uint32_t* __restrict__ stamps, uint8_t* __restrict__ dirty,
                   const int for_update, unsigned long long* __restrict__ words) {
  const uint32_t now = static_cast<uint32_t>(words[kCacheClock]);
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kCacheBlockThreads + threadIdx.x;
  bool hit = false, miss = false;
  if (i < n) {
    const int64_t key = keys[i];
    const bool head = i == 0 || keys[i - 1] != key;
    if (head) {   // (run ids count up from 0 through the sorted keys: below n)
      const int64_t run = run_of[i];
      if (run >= 0 && run < n) distinct[run] = key;
    }
    if (head && key < sentinel) {
      const int64_t row = key & ((int64_t{1} << row_bits) - 1);
      const int32_t slot = slot_of_row[row];
      if (slot >= 0) {
        stamps[slot] = now;
        if (for_update) dirty[slot] = 1;
        hit = true;
      } else {
        miss = true;
      }
    }
  }
  const unsigned long long hits = __ballot(hit), misses = __ballot(miss);
  if ((threadIdx.x & 63) == 0) {
    if (hits) atomicAdd(&words[kCacheHits], static_cast<unsigned long long>(__popcll(hits)));
    if (misses) atomicAdd(&words[kCacheMisses], static_cast<unsigned long long>(__popcll(misses)));
  }
}

//! First position of keys[0, n) that holds a value >= key (at most 64 halvings).
__device__ __forceinline__ int64_t CacheLowerBound(const int64_t* __restrict__ keys, const int64_t n, const int64_t key) {
  int64_t lo = 0, hi = n;
  for (int step = 0; step < 64 && lo < hi; ++step) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (keys[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ int64_t ShuffleWord(const int64_t v, const int lane) {
  const int lo = __shfl(static_cast<int>(v & 0xFFFFFFFFll), lane);
  const int hi = __shfl(static_cast<int>(v >> 32), lane);
  return (static_cast<int64_t>(hi) << 32) | static_cast<int64_t>(static_cast<uint32_t>(lo));
}

/**
 * @brief Then the misses of each set, in ascending row id.  Wavefront w of workgroup b owns set b * 4 + w; lane = way.
 * The set's tags, stamps and dirty bytes are loaded once (one coalesced load per array), kept in registers and stored
 * once.  `keys` holds the distinct keys of the batch, *last_run + 1 of them (clamped to `capacity`); the segment of the
 * set is found by two binary searches and walked 64 keys per step: a lane's key is a miss when slot_of_row says not
 * resident, the misses of a step reserve their entries of the move list with one atomic and are served bit by bit.  A
 * miss takes the way with the smallest (stamp, way) among ways with stamp < clock -- a min over the wave's stamps, then
 * the lowest lane that holds it -- and fills one CacheMove; without such a way the row stays uncached, `unplaced` is
 * raised and its entry moves nothing.
 */
__global__ void __launch_bounds__(kCacheBlockThreads)
    CachePlaceKernel(const int64_t* __restrict__ keys, const int64_t* __restrict__ last_run, const int64_t capacity,
                     const int row_bits, const uint32_t num_sets,
                     int64_t* __restrict__ tags, uint32_t* __restrict__ stamps, uint8_t* __restrict__ dirty,
                     int32_t* __restrict__ slot_of_row, const int for_update, CacheMove* __restrict__ moves,
                     const int64_t move_capacity, unsigned long long* __restrict__ words) {
  const int lane = static_cast<int>(threadIdx.x) & (kRowCacheWays - 1);
  const uint32_t set = blockIdx.x * kCacheSetsPerBlock + (threadIdx.x >> 6);
  if (set >= num_sets) return;   // (the same for every lane of a wavefront)
  const uint32_t now = static_cast<uint32_t>(words[kCacheClock]);
  int64_t n = *last_run + 1;   // the distinct keys, the sentinel's run included; never more than the lookups
  n = n < 0 ? 0 : (n > capacity ? capacity : n);
  const int64_t lo = CacheLowerBound(keys, n, static_cast<int64_t>(set) << row_bits);
  const int64_t hi = CacheLowerBound(keys, n, (static_cast<int64_t>(set) + 1) << row_bits);
  if (lo >= hi) return;
  const int64_t row_mask = (int64_t{1} << row_bits) - 1;
  const int32_t slot = static_cast<int32_t>(set) * kRowCacheWays + lane;
  int64_t tag = tags[slot];
  uint32_t stamp = stamps[slot];
  int is_dirty = dirty[slot];
  int evictions = 0, write_backs = 0, unplaced = 0, overflow = 0;
  bool changed = false;

  for (int64_t base = lo; base < hi; base += kRowCacheWays) {
    const int64_t i = base + lane;
    const bool in = i < hi;
    const int64_t key = in ? keys[i] : -1;
    const int64_t row = key & row_mask;
    const bool miss = in && slot_of_row[row] < 0;
    unsigned long long todo = __ballot(miss);
    if (todo == 0) continue;
    // room in the move list for every miss of the window, reserved with one atomic
    const int wanted = __popcll(todo);
    unsigned long long at = 0;
    if (lane == 0) at = atomicAdd(&words[kCacheMoveCount], static_cast<unsigned long long>(wanted));
    at = static_cast<unsigned long long>(ShuffleWord(static_cast<int64_t>(at), 0));
    if (static_cast<int64_t>(at) + wanted > move_capacity) {   // no room to record the moves: the rows stay uncached
      if (lane < wanted && static_cast<int64_t>(at) + lane < move_capacity) {   // (what the mover will read moves nothing)
        CacheMove none;
        none.new_row = -1;
        none.old_row = -1;
        none.slot = 0;
        none.write_back = 0;
        moves[at + lane] = none;
      }
      unplaced += wanted;
      overflow = 1;
      continue;
    }
    while (todo != 0) {   // (at most 64 turns: one per bit)
      const int j = __ffsll(static_cast<long long>(todo)) - 1;
      todo &= todo - 1;
      const int64_t new_row = ShuffleWord(row, j);
      const bool free_way = stamp < now;
      uint32_t oldest = free_way ? stamp : 0xFFFFFFFFu;
      for (int d = kRowCacheWays / 2; d > 0; d >>= 1) {
        const uint32_t other = static_cast<uint32_t>(__shfl_xor(static_cast<int>(oldest), d));
        oldest = other < oldest ? other : oldest;
      }
      const unsigned long long candidates = __ballot(free_way && stamp == oldest);
      if (candidates == 0) {   // every way was used by this batch: the reserved entry moves nothing
        ++unplaced;
        if (lane == 0) {
          CacheMove none;
          none.new_row = -1;
          none.old_row = -1;
          none.slot = 0;
          none.write_back = 0;
          moves[at] = none;
        }
        ++at;
        continue;
      }
      const int way = __ffsll(static_cast<long long>(candidates)) - 1;
      const int64_t old_row = ShuffleWord(tag, way);
      const int old_dirty = __shfl(is_dirty, way);
      const int write_back = (old_row >= 0 && old_dirty) ? 1 : 0;
      if (lane == way) {
        CacheMove m;
        m.new_row = new_row;
        m.old_row = old_row;
        m.slot = slot;
        m.write_back = write_back;
        moves[at] = m;
        if (old_row >= 0) slot_of_row[old_row] = -1;
        slot_of_row[new_row] = slot;
        tag = new_row;
        stamp = now;
        is_dirty = for_update ? 1 : 0;
      }
      ++at;
      evictions += old_row >= 0 ? 1 : 0;
      write_backs += write_back;
      changed = true;
    }
  }
  if (changed) {
    tags[slot] = tag;
    stamps[slot] = stamp;
    dirty[slot] = static_cast<uint8_t>(is_dirty);
  }
  if (lane == 0) {
    if (evictions) atomicAdd(&words[kCacheEvictions], static_cast<unsigned long long>(evictions));
    if (write_backs) atomicAdd(&words[kCacheWriteBacks], static_cast<unsigned long long>(write_backs));
    if (unplaced) atomicAdd(&words[kCacheUnplaced], static_cast<unsigned long long>(unplaced));
    if (overflow) atomicMax(&words[kCacheOverflow], 1ull);
  }
}

/**
 * @brief The row exchange.  One lane group (a power of two <= 64) per entry, every lane moves LaneT (16, 8 or 4 bytes)
 * slices lane, lane + group, ... of the row.
 *   moves != nullptr: the entries of the move list, count = min(words[kCacheMoveCount], capacity).  A dirty victim goes
 *       cache -> table, then the new row table -> cache: both loads are issued before both stores, and a lane stores
 *       over the cache bytes it has itself just read.  No row is both written back and fetched in one prefetch, so the
 *       entries need no order among themselves.
 *   moves == nullptr (flush): entry k is slot k of `capacity` slots; a valid dirty slot goes cache -> table and its
 *       dirty byte is cleared.
 * The kernel moves ONE PLANE of the cache: the table's rows, or the optimizer state that rides on the same slots
 * (`table` / `cache` / `row_bytes` are then the state's; a 4-byte state row is one uint32_t lane, group = 1).  A flush
 * decides from dirty[k], so the planes are flushed one launch after the other in stream order and only the last one --
 * `commit` != 0, the table's -- clears the dirty bytes and counts the write-backs: one dirty byte covers all planes
 * (there may be two state planes) and the counters count rows, not planes.  The move list is read-only here, so a prefetch needs no such switch.
 */
template <typename LaneT>
__global__ void __launch_bounds__(kCacheBlockThreads)
    CacheMoveKernel(const CacheMove* __restrict__ moves, const int64_t capacity, const int64_t* __restrict__ tags,
                    uint8_t* __restrict__ dirty, char* __restrict__ table, char* __restrict__ cache,
                    const int64_t row_bytes, const int lanes_per_row, const int group, const int commit,
                    unsigned long long* __restrict__ words) {
  const int lane = static_cast<int>(threadIdx.x) & (group - 1);
  const int groups_per_block = kCacheBlockThreads / group;
  const int64_t first = static_cast<int64_t>(blockIdx.x) * groups_per_block + static_cast<int>(threadIdx.x) / group;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * groups_per_block;
  int64_t count = capacity;
  if (moves != nullptr) {
    const unsigned long long listed = words[kCacheMoveCount];
    count = listed < static_cast<unsigned long long>(capacity) ? static_cast<int64_t>(listed) : capacity;
  }
  int flushed = 0;
  for (int64_t k = first; k < count; k += stride) {
    int64_t new_row = -1, old_row;
    int64_t slot = k;
    bool write_back;
    if (moves != nullptr) {
      const CacheMove m = moves[k];
      new_row = m.new_row;
      old_row = m.old_row;
      slot = m.slot;
      write_back = m.write_back != 0;
    } else {
      old_row = tags[k];
      // (lane 0 reads the byte it clears below; the others get its value)
      write_back = __shfl(lane == 0 ? static_cast<int>(dirty[k]) : 0, 0, group) != 0 && old_row >= 0;
      if (lane == 0 && write_back && commit) {
        dirty[k] = 0;
        ++flushed;
      }
    }
    LaneT* cached = reinterpret_cast<LaneT*>(cache + slot * row_bytes);
    LaneT* victim = reinterpret_cast<LaneT*>(table + old_row * row_bytes);
    const LaneT* wanted = reinterpret_cast<const LaneT*>(table + new_row * row_bytes);
    for (int c = lane; c < lanes_per_row; c += group) {
      LaneT out, in;
      if (write_back) out = cached[c];
      if (new_row >= 0) in = wanted[c];
      if (write_back) victim[c] = out;
      if (new_row >= 0) cached[c] = in;
    }
  }
  if (flushed) atomicAdd(&words[kCacheWriteBacks], static_cast<unsigned long long>(flushed));
}

__global__ void CacheClockKernel(unsigned long long* __restrict__ words) { words[kCacheClock] += 1; }

}  // namespace detail
}  // namespace cuembed

#endif  // CUEMBED_INCLUDE_ROW_CACHE_KERNELS_HPP_
