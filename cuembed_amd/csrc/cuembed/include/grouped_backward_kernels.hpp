// MI355X (gfx950 / CDNA4) small integer kernels behind grouped_backward.hpp (an extension: the reference's backward
// takes one table).  All results are integers and bit-exact.
//
// A GROUP of T tables is trained through ONE sort and ONE scatter-add by giving every lookup of bag g = t * B + b
//   the key        row_base[t] + id      a row of the tables laid end to end (row_base: exclusive prefix sum of the row counts)
//   the sample id  b * T + t             its row in out[B, T, W] viewed as [B * T, W]
// GroupedKeysCsrKernel / GroupedKeysFixedKernel build both arrays in one launch; GroupedTableCutsKernel finds the
// table boundaries in the compressed gradient that comes out of the pipeline.
#ifndef CUEMBED_INCLUDE_GROUPED_BACKWARD_KERNELS_HPP_
#define CUEMBED_INCLUDE_GROUPED_BACKWARD_KERNELS_HPP_

#include <hip/hip_runtime.h>

#include <cstdint>

#include "cuembed/include/index_kernels.hpp"

namespace cuembed {
namespace detail {

//! Consecutive lookups one thread writes (one 16-byte store per output for 32-bit keys, 32 bytes for 64-bit ones).
constexpr int kGroupedKeysItemsPerThread = 4;

//! i / d for 0 <= i < 2^31 by QuotientMagic's multiply-shift.
__device__ __forceinline__ int GroupedQuotient(const int i, const unsigned magic, const int shift) {
  return static_cast<int>((static_cast<unsigned long long>(static_cast<unsigned>(i)) * magic) >> shift);
}

//! CSR: keys[p] = row_base[g / B] + indices[p], sample_ids[p] = (g % B) * T + g / B for p in [offsets[g], offsets[g+1]).
//! ExpandCsrKernel's shape: a workgroup owns `bags_per_block` consecutive bags, stages their offsets in LDS and, next
//! to them, once per bag, the bag's key base and output row (one division per BAG).  It then walks its contiguous
//! slice of the lookups in aligned groups of kGroupedKeysItemsPerThread: one binary search in LDS for the first
//! lookup of a group, a forward walk over the (possibly empty) bags for the others, one vector load of the indices
//! and one vector store per output.  The ragged ends of the slice (it begins where the previous workgroup's ends,
//! at any position) and unaligned buffers (`vector_ok` == 0) take scalar loads and stores.  Positions are clamped
//! to [0, nnz): offsets that leave it are a contract violation that writes nothing out of bounds.
template <typename IndexT, typename OffsetT, typename KeyT>
__global__ void __launch_bounds__(256)
GroupedKeysCsrKernel(const IndexT* __restrict__ indices, const OffsetT* __restrict__ offsets,
                     const int64_t* __restrict__ row_base, const int num_tables, const int batch, const int num_bags,
                     const unsigned batch_magic, const int batch_shift, const int64_t nnz, KeyT* __restrict__ keys,
                     KeyT* __restrict__ sample_ids, const int bags_per_block /* <= kCsrSamplesPerBlock */,
                     const int vector_ok) {
  constexpr int kItems = kGroupedKeysItemsPerThread;
  __shared__ int64_t bounds[kCsrSamplesPerBlock + 1];
  __shared__ int64_t key_base[kCsrSamplesPerBlock];
  __shared__ int32_t out_row[kCsrSamplesPerBlock];
  const int first_bag = blockIdx.x * bags_per_block;
  const int nbags = (num_bags - first_bag < bags_per_block) ? num_bags - first_bag : bags_per_block;
  for (int s = threadIdx.x; s <= nbags; s += blockDim.x) {
    bounds[s] = static_cast<int64_t>(offsets[first_bag + s]);
    if (s < nbags) {
      const int g = first_bag + s;
      const int t = GroupedQuotient(g, batch_magic, batch_shift);
      const int b = g - t * batch;
      key_base[s] = row_base[t];
      out_row[s] = b * num_tables + t;       // < num_tables * batch <= INT_MAX
    }
  }
  __syncthreads();
  int64_t lo_pos = bounds[0], hi_pos = bounds[nbags];
  lo_pos = lo_pos < 0 ? 0 : lo_pos;
  hi_pos = hi_pos > nnz ? nnz : hi_pos;
  const int64_t first_group = lo_pos & ~static_cast<int64_t>(kItems - 1);
  for (int64_t p0 = first_group + static_cast<int64_t>(threadIdx.x) * kItems; p0 < hi_pos;
       p0 += static_cast<int64_t>(blockDim.x) * kItems) {
    const int64_t begin = p0 < lo_pos ? lo_pos : p0;
    // largest s with bounds[s] <= begin  (empty bags have bounds[s] == bounds[s+1])
    int lo = 0, hi = nbags;  // invariant: bounds[lo] <= begin < bounds[hi]
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (bounds[mid] <= begin) lo = mid;
      else hi = mid;
    }
    if (vector_ok && p0 >= lo_pos && p0 + kItems <= hi_pos) {
      typedef IndexT __attribute__((ext_vector_type(kItems))) in_t;
      typedef KeyT __attribute__((ext_vector_type(kItems))) out_t;
      const in_t id = *reinterpret_cast<const in_t*>(indices + p0);
      out_t k, r;
#pragma unroll
      for (int j = 0; j < kItems; ++j) {
        while (lo + 1 < nbags && bounds[lo + 1] <= p0 + j) ++lo;
        k[j] = static_cast<KeyT>(key_base[lo] + static_cast<int64_t>(id[j]));
        r[j] = static_cast<KeyT>(out_row[lo]);
      }
      *reinterpret_cast<out_t*>(keys + p0) = k;             // (p0 is a multiple of 4 items: 16- / 32-byte aligned)
      *reinterpret_cast<out_t*>(sample_ids + p0) = r;
    } else {
      const int64_t end = p0 + kItems < hi_pos ? p0 + kItems : hi_pos;
      for (int64_t p = begin; p < end; ++p) {
        while (lo + 1 < nbags && bounds[lo + 1] <= p) ++lo;
        keys[p] = static_cast<KeyT>(key_base[lo] + static_cast<int64_t>(indices[p]));
        sample_ids[p] = static_cast<KeyT>(out_row[lo]);
      }
    }
  }
}

//! Fixed hotness: lookup p belongs to bag g = p / H, table t = g / B, sample b = g - t * B.  FillQuotientKernel's
//! shape: every thread takes kGroupedKeysItemsPerThread CONSECUTIVE lookups (one vector load, one vector store per
//! output), both divisions by multiply-shift (count < 2^31).
template <typename IndexT, typename KeyT>
__global__ void __launch_bounds__(256)
GroupedKeysFixedKernel(const IndexT* __restrict__ indices, const int64_t* __restrict__ row_base, const int num_tables,
                       const int batch, const unsigned hot_magic, const int hot_shift, const unsigned batch_magic,
                       const int batch_shift, const int count, KeyT* __restrict__ keys, KeyT* __restrict__ sample_ids,
                       const int vector_ok) {
  constexpr int kItems = kGroupedKeysItemsPerThread;
  const int64_t p0 = (static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) * kItems;
  if (p0 >= count) return;
  const bool full = vector_ok && p0 + kItems <= count;
  IndexT id[kItems];
  if (full) {
    typedef IndexT __attribute__((ext_vector_type(kItems))) in_t;
    const in_t v = *reinterpret_cast<const in_t*>(indices + p0);
#pragma unroll
    for (int j = 0; j < kItems; ++j) id[j] = v[j];
  } else {
#pragma unroll
    for (int j = 0; j < kItems; ++j) id[j] = p0 + j < count ? indices[p0 + j] : IndexT{0};
  }
  KeyT k[kItems], r[kItems];
#pragma unroll
  for (int j = 0; j < kItems; ++j) {
    const int p = static_cast<int>(p0 + j < count ? p0 + j : p0);
    const int g = GroupedQuotient(p, hot_magic, hot_shift);
    const int t = GroupedQuotient(g, batch_magic, batch_shift);
    const int b = g - t * batch;
    k[j] = static_cast<KeyT>(row_base[t] + static_cast<int64_t>(id[j]));
    r[j] = static_cast<KeyT>(b * num_tables + t);
  }
  if (full) {
    typedef KeyT __attribute__((ext_vector_type(kItems))) out_t;
    out_t kv, rv;
#pragma unroll
    for (int j = 0; j < kItems; ++j) {
      kv[j] = k[j];
      rv[j] = r[j];
    }
    *reinterpret_cast<out_t*>(keys + p0) = kv;              // (p0 is a multiple of 4 items: 16- / 32-byte aligned)
    *reinterpret_cast<out_t*>(sample_ids + p0) = rv;
  } else {
#pragma unroll
    for (int j = 0; j < kItems; ++j)
      if (p0 + j < count) {
        keys[p0 + j] = k[j];
        sample_ids[p0 + j] = r[j];
      }
  }
}

//! cuts[t] = the number of valid entries of the ascending `ids` that are < row_base[t], t in [0, num_tables]: one
//! workgroup, one binary search per thread.  The entry count is `host_count` (>= 0), or read on the device: one
//! int32 / int64 word (`count_word`), or one word of the ids' type holding the last id, count = last_id + 1
//! (`last_id`: transpose_remapped_indices[nnz - 1]).  A count below zero or above `capacity` gives all-zero cuts.
template <typename IndexT>
__global__ void __launch_bounds__(256)
GroupedTableCutsKernel(const IndexT* __restrict__ ids, const int64_t capacity, const int64_t host_count,
                       const void* __restrict__ count_word, const int count_word_is_64,
                       const IndexT* __restrict__ last_id, const int64_t* __restrict__ row_base, const int num_tables,
                       int64_t* __restrict__ cuts) {
  int64_t count = host_count;
  if (count_word != nullptr) {
    count = count_word_is_64 ? *static_cast<const int64_t*>(count_word)
                             : static_cast<int64_t>(*static_cast<const int32_t*>(count_word));
  } else if (last_id != nullptr) {
    count = static_cast<int64_t>(*last_id) + 1;
  }
  if (count < 0 || count > capacity) count = 0;
  for (int t = threadIdx.x; t <= num_tables; t += blockDim.x) {
    const int64_t bound = row_base[t];
    int64_t lo = 0, hi = count;   // the first entry in [lo, hi) that is >= bound
    while (lo < hi) {
      const int64_t mid = lo + ((hi - lo) >> 1);
      if (static_cast<int64_t>(ids[mid]) < bound) lo = mid + 1;
      else hi = mid;
    }
    cuts[t] = lo;
  }
}

}  // namespace detail
}  // namespace cuembed

#endif  // CUEMBED_INCLUDE_GROUPED_BACKWARD_KERNELS_HPP_
