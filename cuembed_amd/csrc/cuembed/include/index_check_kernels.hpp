// Device side of cuembed::CheckIndices (an extension; the reference trusts its indices and offsets, like every
// row-addressing kernel here): is a batch safe to hand to the kernels that address table rows, and, optionally, a
// repaired copy that is safe by construction.  Nothing here reads a table, nothing is read back, and no memory is ever
// addressed with an unchecked value: `indices` is walked by position, `offsets` by bag number, and the table of a
// position comes from the REPAIRED offsets only.  Definitions: index_check.hpp.
//
//   OffsetsTileMaxKernel   CSR, launch 1: the raw maximum and the last raw value of every tile of offsets[0 .. n]; its
//                          first workgroup also initialises the report;
//   OffsetsRepairKernel    CSR, launch 2: every workgroup folds the maxima of the earlier tiles itself, scans its tile
//                          (running maximum, clamped into [0, nnz]), counts the local violations, writes offsets_out
//                          and the num_tables + 1 cuts r[t * B] for the index pass;
//   ClearIndexReportKernel fixed hotness: the report's initial words (no offsets, so neither launch above);
//   IndexCheckKernel       one coalesced pass over indices, one 16-byte (or narrower) piece per lane, the tail by
//                          predication; the table of a lane's first position by one division (fixed hotness) or one
//                          binary search over the cuts staged in LDS (CSR), then by stepping.
//
// Counting is a wavefront ballot + popcount: a wavefront that saw something bad sends ONE 64-bit atomic add and ONE 64-bit
// atomic min (the first position; "first" = smallest, so the report is a function of the input, not of scheduling); a
// clean batch sends no atomic at all.  The loads are ordinary ones, not non-temporal: the forward that the check protects
// reads the same indices next, out of L2.
#ifndef CUEMBED_INCLUDE_INDEX_CHECK_KERNELS_HPP_
#define CUEMBED_INCLUDE_INDEX_CHECK_KERNELS_HPP_

#include <hip/hip_runtime.h>

#include <cstdint>

namespace cuembed {
namespace detail {

constexpr int kCheckThreads = 256;
constexpr int kCheckWaves = kCheckThreads / 64;
constexpr int kCheckMaxTables = 1023;        // cuts and row counts of a group are staged in 16 KiB of LDS
constexpr int kCheckScanItems = 4;           // offsets per thread and chunk of the scan
constexpr int kCheckScanChunk = kCheckThreads * kCheckScanItems;
constexpr int kCheckMaxTiles = 1024;         // the fold of the earlier tiles' maxima: at most 4 words per thread
// The index pass is one launch of ceil(nnz / (kCheckThreads * kLane)) workgroups, kLane = 1 for the least aligned
// arrays: 2^38 lookups are 2^30 workgroups, inside the grid's limit of 2^31 - 1 with room to spare (and 1 TiB of int32 ids).
constexpr int64_t kCheckMaxLookups = int64_t{1} << 38;

__device__ __forceinline__ int64_t CheckMax(const int64_t a, const int64_t b) { return a > b ? a : b; }

//! The report's words before anything is counted: no bad index, no bad offset, no first position.
__device__ __forceinline__ void InitIndexReport(unsigned long long* __restrict__ report) {
  report[0] = 0ull;
  report[1] = ~0ull;      // (-1; the first positions are lowered by UNSIGNED atomic minima)
  report[2] = 0ull;
  report[3] = ~0ull;
}

//! One wavefront's findings into the report: `bad` is this lane's verdict on the element at `position`; `count` /
//! `first` (the same in every lane) gather them over the wavefront's elements.
__device__ __forceinline__ void WaveTally(const bool bad, const int64_t position_of_lane0, const int64_t lane_stride,
                                          const int64_t item, unsigned long long& count, int64_t& first) {
  const unsigned long long votes = __ballot(bad);
  if (votes != 0ull) {
    count += static_cast<unsigned long long>(__popcll(votes));
    const int64_t at = position_of_lane0 + static_cast<int64_t>(__ffsll(votes) - 1) * lane_stride + item;
    first = at < first ? at : first;
  }
}

__device__ __forceinline__ void WaveReport(const unsigned long long count, const int64_t first,
                                           unsigned long long* __restrict__ count_word,
                                           unsigned long long* __restrict__ first_word) {
  if (count != 0ull && (threadIdx.x & 63) == 0) {
    atomicAdd(count_word, count);
    atomicMin(first_word, static_cast<unsigned long long>(first));
  }
}

template <int kUnused = 0>   // (a template so that the header can be included from several translation units)
__global__ void ClearIndexReportKernel(unsigned long long* __restrict__ report) {
  if (threadIdx.x == 0 && blockIdx.x == 0) InitIndexReport(report);
}

// ---------------------------------------------------------------------------
// Offsets, launch 1.  Tile w = positions [w * tile_len, min((w + 1) * tile_len, positions)) of offsets[0 .. n]
// (positions = n + 1; tile_len a multiple of kCheckScanChunk, at most kCheckMaxTiles tiles).  tile_last is what launch 2
// compares a tile's first offset with: launch 2 may overwrite `offsets` (repair in place), launch 1 never writes it.
// ---------------------------------------------------------------------------
template <typename OffsetT>
__global__ void __launch_bounds__(kCheckThreads)
OffsetsTileMaxKernel(const OffsetT* offsets, const int64_t positions, const int64_t tile_len,
                     int64_t* __restrict__ tile_max, int64_t* __restrict__ tile_last,
                     unsigned long long* __restrict__ report) {
  __shared__ int64_t wave_max[kCheckWaves];
  const int64_t begin = static_cast<int64_t>(blockIdx.x) * tile_len;
  const int64_t end = begin + tile_len < positions ? begin + tile_len : positions;
  int64_t m = INT64_MIN;
  for (int64_t i = begin + threadIdx.x; i < end; i += kCheckThreads) m = CheckMax(m, static_cast<int64_t>(offsets[i]));
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) m = CheckMax(m, __shfl_xor(m, d));
  if ((threadIdx.x & 63) == 0) wave_max[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < kCheckWaves; ++w) m = CheckMax(m, wave_max[w]);
    tile_max[blockIdx.x] = m;
    tile_last[blockIdx.x] = static_cast<int64_t>(offsets[end - 1]);      // (begin < positions: end - 1 >= begin)
    if (blockIdx.x == 0) InitIndexReport(report);
  }
}

// ---------------------------------------------------------------------------
// Offsets, launch 2.  r[i] = min(nnz, max(0, max_{k <= i} o[k])); position i is bad iff o[i] < 0, o[i] > nnz or (i > 0 and)
// o[i] < o[i - 1] -- on the RAW values, whose neighbours across threads, chunks and tiles travel through LDS, a
// register and tile_last: never through `offsets`, which offsets_out may be.  A chunk's loads all precede its stores.
// ---------------------------------------------------------------------------
template <typename OffsetT>
__global__ void __launch_bounds__(kCheckThreads)
OffsetsRepairKernel(const OffsetT* offsets, const int64_t positions, const int64_t nnz, const int64_t tile_len,
                    const int64_t* __restrict__ tile_max, const int64_t* __restrict__ tile_last, const int num_tables,
                    const int batch_per_table, OffsetT* offsets_out, int64_t* __restrict__ cuts,
                    unsigned long long* __restrict__ report) {
  __shared__ int64_t wave_max[kCheckWaves];
  __shared__ int64_t last_raw[kCheckThreads];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tile = static_cast<int>(blockIdx.x);
  int64_t carry_max = INT64_MIN;
  for (int k = tid; k < tile; k += kCheckThreads) carry_max = CheckMax(carry_max, tile_max[k]);
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) carry_max = CheckMax(carry_max, __shfl_xor(carry_max, d));
  if (lane == 0) wave_max[wave] = carry_max;
  __syncthreads();
#pragma unroll
  for (int w = 0; w < kCheckWaves; ++w) carry_max = CheckMax(carry_max, wave_max[w]);
  int64_t carry_last = tile > 0 ? tile_last[tile - 1] : 0;
  __syncthreads();                                   // (wave_max is written again below)
  const int64_t begin = static_cast<int64_t>(tile) * tile_len;
  const int64_t end = begin + tile_len < positions ? begin + tile_len : positions;
  unsigned long long count = 0ull;
  int64_t first = INT64_MAX;
  for (int64_t chunk = begin; chunk < end; chunk += kCheckScanChunk) {     // (the same trips for the whole workgroup)
    const int64_t i0 = chunk + static_cast<int64_t>(tid) * kCheckScanItems;
    int64_t v[kCheckScanItems], m[kCheckScanItems];
#pragma unroll
    for (int j = 0; j < kCheckScanItems; ++j) v[j] = i0 + j < end ? static_cast<int64_t>(offsets[i0 + j]) : INT64_MIN;
    m[0] = v[0];
#pragma unroll
    for (int j = 1; j < kCheckScanItems; ++j) m[j] = CheckMax(m[j - 1], v[j]);
    int64_t incl = m[kCheckScanItems - 1];
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int64_t up = __shfl_up(incl, d);
      if (lane >= d) incl = CheckMax(incl, up);
    }
    const int64_t lanes_before = __shfl_up(incl, 1);
    if (lane == 63) wave_max[wave] = incl;
    last_raw[tid] = v[kCheckScanItems - 1];          // (read by the next thread only when it has an item: mine are then all real)
    __syncthreads();
    int64_t base = carry_max, chunk_max = carry_max;
#pragma unroll
    for (int w = 0; w < kCheckWaves; ++w) {
      if (w < wave) base = CheckMax(base, wave_max[w]);
      chunk_max = CheckMax(chunk_max, wave_max[w]);
    }
    if (lane > 0) base = CheckMax(base, lanes_before);
    const int64_t before_me = tid > 0 ? last_raw[tid - 1] : carry_last;
    const int64_t chunk_last = last_raw[kCheckThreads - 1];
    int64_t prev = before_me;                        // the raw offset in front of item j
#pragma unroll
    for (int j = 0; j < kCheckScanItems; ++j) {
      const int64_t i = i0 + j;
      const bool real = i < end;
      const int64_t run = CheckMax(base, m[j]);
      const int64_t repaired = run < 0 ? 0 : (run > nnz ? nnz : run);
      const bool bad = real && (v[j] < 0 || v[j] > nnz || (i > 0 && v[j] < prev));
      prev = v[j];
      if (real) {
        if (offsets_out != nullptr) offsets_out[i] = static_cast<OffsetT>(repaired);
        if (batch_per_table > 0) {
          const unsigned bag = static_cast<unsigned>(i), per = static_cast<unsigned>(batch_per_table);   // (i <= n <= INT_MAX)
          if (bag % per == 0u) cuts[bag / per] = repaired;
        } else {                                     // (no bags: position 0 is all there is, and every cut)
          for (int t = 0; t <= num_tables; ++t) cuts[t] = repaired;
        }
      }
      WaveTally(bad, chunk + static_cast<int64_t>(wave) * (64 * kCheckScanItems), kCheckScanItems, j, count, first);
    }
    carry_max = chunk_max;
    carry_last = chunk_last;
    __syncthreads();                                 // (wave_max and last_raw are written again in the next trip)
  }
  WaveReport(count, first, report + 2, report + 3);
}

// ---------------------------------------------------------------------------
// The index pass.  Lane l of workgroup w owns the kLane consecutive positions from (w * kCheckThreads + l) * kLane on;
// kLane * sizeof(IndexT) = 16 bytes where indices and indices_out are 16-byte aligned, 8 or 4 otherwise; a lane whose
// piece crosses nnz takes its elements one by one.  kCsr: `cuts` holds the num_tables + 1 values r[t * B] (ascending, in
// [0, nnz]); position p is checked iff cuts[0] <= p < cuts[num_tables], against the rows of the table t with cuts[t] <= p <
// cuts[t + 1].  Otherwise (fixed hotness) table t = p / per_table, per_table = B * num_hots, and every position is checked.
// Ids are compared in 64 bits.  indices_out may be null, indices itself (a lane reads and writes only its own piece;
// clean pieces are then not written at all) or a separate array: positions outside the checked range are copied through.
// ---------------------------------------------------------------------------
template <typename IndexT, int kLane>
struct alignas(sizeof(IndexT) * kLane) IndexPiece {
  IndexT e[kLane];
};

template <typename IndexT, int kLane, bool kCsr>
__global__ void __launch_bounds__(kCheckThreads)
IndexCheckKernel(const IndexT* indices, const int64_t nnz, const int64_t* __restrict__ row_base, const int64_t num_rows,
                 const int num_tables, const int64_t per_table, const int64_t* __restrict__ cuts, IndexT* indices_out,
                 unsigned long long* __restrict__ report) {
  __shared__ int64_t s_rows[kCheckMaxTables + 1];
  __shared__ int64_t s_cuts[kCsr ? kCheckMaxTables + 1 : 1];
  using Piece = IndexPiece<IndexT, kLane>;
  const int tid = threadIdx.x;
  const int64_t p0 = (static_cast<int64_t>(blockIdx.x) * kCheckThreads + tid) * kLane;
  // this lane's piece first: its load is in flight while the row counts and cuts are staged
  const bool whole = p0 + kLane <= nnz;
  Piece piece;
  if (whole) {
    piece = *reinterpret_cast<const Piece*>(indices + p0);
  } else {
#pragma unroll
    for (int j = 0; j < kLane; ++j) piece.e[j] = p0 + j < nnz ? indices[p0 + j] : IndexT(0);
  }
  for (int t = tid; t < num_tables; t += kCheckThreads) s_rows[t] = row_base != nullptr ? row_base[t + 1] - row_base[t] : num_rows;
  if constexpr (kCsr) {
    for (int t = tid; t <= num_tables; t += kCheckThreads) s_cuts[t] = cuts[t];
  }
  __syncthreads();
  int t = 0;
  int64_t within = 0;            // fixed hotness: p - t * per_table
  int64_t checked_from = 0, checked_to = nnz;
  if constexpr (kCsr) {
    checked_from = s_cuts[0];
    checked_to = s_cuts[num_tables];
    int lo = 1, hi = num_tables;                     // t = how many of cuts[1 .. num_tables - 1] are <= p0
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (s_cuts[mid] <= p0) lo = mid + 1;
      else hi = mid;
    }
    t = lo - 1;
  } else if (p0 < nnz) {                             // (t < num_tables: nnz = num_tables * per_table)
    if (nnz <= static_cast<int64_t>(0xffffffffu))
      t = static_cast<int>(static_cast<unsigned>(p0) / static_cast<unsigned>(per_table));
    else
      t = static_cast<int>(p0 / per_table);
    within = p0 - static_cast<int64_t>(t) * per_table;
  }
  bool bad[kLane];
  bool any_bad = false;
#pragma unroll
  for (int j = 0; j < kLane; ++j) {
    const int64_t p = p0 + j;
    if constexpr (kCsr) {
      while (t + 1 < num_tables && s_cuts[t + 1] <= p) ++t;
    }
    const int64_t rows = s_rows[t < num_tables ? t : num_tables - 1];
    const int64_t id = static_cast<int64_t>(piece.e[j]);
    bad[j] = p < nnz && p >= checked_from && p < checked_to && (id < 0 || id >= rows);
    any_bad = any_bad || bad[j];
    if (bad[j]) piece.e[j] = IndexT(0);
    if constexpr (!kCsr) {
      if (++within == per_table) {
        within = 0;
        ++t;
      }
    }
  }
  if (indices_out != nullptr && (indices_out != indices || any_bad)) {
    if (whole) {
      *reinterpret_cast<Piece*>(indices_out + p0) = piece;
    } else {
#pragma unroll
      for (int j = 0; j < kLane; ++j)
        if (p0 + j < nnz) indices_out[p0 + j] = piece.e[j];
    }
  }
  unsigned long long count = 0ull;
  int64_t first = INT64_MAX;
  const int64_t wave_p0 = (static_cast<int64_t>(blockIdx.x) * kCheckThreads + (tid & ~63)) * kLane;
#pragma unroll
  for (int j = 0; j < kLane; ++j) WaveTally(bad[j], wave_p0, kLane, j, count, first);
  WaveReport(count, first, report + 0, report + 1);
}

}  // namespace detail
}  // namespace cuembed

#endif  // CUEMBED_INCLUDE_INDEX_CHECK_KERNELS_HPP_
