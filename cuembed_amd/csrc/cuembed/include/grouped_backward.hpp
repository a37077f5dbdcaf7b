// MI355X (gfx950 / CDNA4) embedding lookup -- the backward of a GROUP of tables (host API; an extension: the
// reference's backward takes one table).
//
// The group of grouped_lookup.hpp -- T tables of one width, bag g = t * B + b, out [B, T, W] -- is trained through the
// single-table pipeline, once for all tables:
//
//   GroupedBackwardKeys(...)                   keys[p] = row_base[t] + indices[p], sample_ids[p] = b * T + t
//   Transpose(sample_ids, keys, weights, ...)  index_bits = ceil(log2(total_rows)): the sort skips the zero digits
//   ComputeCompressedGradIndices(...)          (compressed gradient only; or Transpose's transpose_remapped_indices)
//   EmbeddingBackward(grad_y as [B * T, W], ...)
//   GroupedTableCuts(...)                      where each table's entries begin in the compressed gradient
//
// row_base[T + 1] is the exclusive prefix sum of the tables' row counts (int64, DEVICE memory, built once by the
// caller): the keys are rows of the tables laid end to end, so the gradient comes out sorted by table, then by row,
// and for tables that ARE row slices of one allocation the keys are directly rows of that allocation -- the sparse
// optimizer step (sparse_update.hpp, sparse_adam.hpp) applies to it unchanged.  The sort is stable, so inside one
// table row the lookups keep the order of the single-table pipeline.
// Every function runs on the caller's stream, allocates nothing and reads nothing back.
#ifndef CUEMBED_INCLUDE_GROUPED_BACKWARD_HPP_
#define CUEMBED_INCLUDE_GROUPED_BACKWARD_HPP_

#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "cuembed/include/cuembed_assert.hpp"
#include "cuembed/include/grouped_backward_kernels.hpp"

namespace cuembed {

/**
 * @brief Keys and sample ids of a group's lookups, in one launch.
 *
 * For lookup p of bag g = t * batch_per_table + b:  keys[p] = row_base[t] + indices[p],  sample_ids[p] = b * num_tables + t.
 * CSR: offsets[num_tables * batch_per_table + 1] over indices[nnz]; fixed hotness: offsets == nullptr, num_hots > 0,
 * indices [num_tables, batch_per_table, num_hots] (nnz is then their product).  KeyT is the index type of the backward
 * pipeline and independent of IndexT: int32_t whenever the group has fewer than 2^31 rows in all (the kernel writes
 * fresh arrays, so narrowing int64 ids costs nothing), int64_t otherwise -- keys that do not fit KeyT are the
 * caller's error.  Ids outside [0, rows_t) are a contract violation, as in the forward.  nnz <= INT_MAX (the
 * pipeline's own limit) and num_tables * batch_per_table <= INT_MAX.
 */
template <typename IndexT, typename OffsetT, typename KeyT>
void GroupedBackwardKeys(const IndexT* indices,
                         const OffsetT* offsets,
                         const int64_t* row_base,
                         const int num_tables,
                         const int batch_per_table,
                         const int num_hots,
                         const int64_t nnz,
                         KeyT* keys,
                         KeyT* sample_ids,
                         const hipStream_t stream = 0) {
  CUEMBED_ASSERT(num_tables >= 1);
  CUEMBED_ASSERT(batch_per_table >= 0);
  CUEMBED_ASSERT(static_cast<int64_t>(num_tables) * batch_per_table <= INT_MAX);
  CUEMBED_ASSERT((offsets != nullptr && num_hots == 0) || (offsets == nullptr && num_hots > 0));
  CUEMBED_ASSERT(nnz >= 0 && nnz <= INT_MAX);
  const int num_bags = num_tables * batch_per_table;
  if (offsets == nullptr) CUEMBED_ASSERT(nnz == static_cast<int64_t>(num_bags) * num_hots);
  if (num_bags == 0 || nnz == 0) return;
  constexpr int kItems = detail::kGroupedKeysItemsPerThread;
  const uintptr_t bits = (reinterpret_cast<uintptr_t>(indices) % (kItems * sizeof(IndexT))) |
                         (reinterpret_cast<uintptr_t>(keys) % (kItems * sizeof(KeyT))) |
                         (reinterpret_cast<uintptr_t>(sample_ids) % (kItems * sizeof(KeyT)));
  const int vector_ok = bits == 0 ? 1 : 0;
  const detail::QuotientMagic by_batch(batch_per_table);
  const int threads = 256;
  if (offsets != nullptr) {
    const int per_block = detail::CsrSamplesPerBlock(num_bags);
    const int blocks = (num_bags + per_block - 1) / per_block;
    detail::GroupedKeysCsrKernel<IndexT, OffsetT, KeyT><<<blocks, threads, 0, stream>>>(
        indices, offsets, row_base, num_tables, batch_per_table, num_bags, by_batch.magic, by_batch.shift, nnz, keys,
        sample_ids, per_block, vector_ok);
    return;
  }
  const detail::QuotientMagic by_hots(num_hots);
  const int64_t per_block = static_cast<int64_t>(threads) * kItems;
  detail::GroupedKeysFixedKernel<IndexT, KeyT><<<static_cast<unsigned>((nnz + per_block - 1) / per_block), threads, 0, stream>>>(
      indices, row_base, num_tables, batch_per_table, by_hots.magic, by_hots.shift, by_batch.magic, by_batch.shift,
      static_cast<int>(nnz), keys, sample_ids, vector_ok);
}

/**
 * @brief Table boundaries of a group's compressed gradient: cuts[t] = the number of valid entries of the ascending
 * global ids `inverse_mapping` that are < row_base[t], for t in [0, num_tables] (int64, device memory) -- cuts[0] = 0,
 * cuts[num_tables] = the count; table t owns the entries [cuts[t], cuts[t + 1]), its local ids are
 * inverse_mapping[k] - row_base[t].
 *
 * The entry count, in SparseRowUpdate's conventions: `count_word` (device, one int32 / int64 word, `count_word_is_64`),
 * else `last_id` (device, one IndexT word, count = last_id + 1: transpose_remapped_indices + nnz - 1), else the host
 * value `count`.  `capacity` is the number of entries `inverse_mapping` has room for; a count below zero or above it
 * gives all-zero cuts (the scatter-add then wrote nothing).  One workgroup, one binary search per table.
 */
template <typename IndexT>
void GroupedTableCuts(const IndexT* inverse_mapping,
                      const int64_t capacity,
                      const int64_t count,
                      const void* count_word,
                      const bool count_word_is_64,
                      const IndexT* last_id,
                      const int64_t* row_base,
                      const int num_tables,
                      int64_t* cuts,
                      const hipStream_t stream = 0) {
  CUEMBED_ASSERT(num_tables >= 1);
  CUEMBED_ASSERT(capacity >= 0);
  detail::GroupedTableCutsKernel<IndexT><<<1, 256, 0, stream>>>(inverse_mapping, capacity, count, count_word,
                                                               count_word_is_64 ? 1 : 0, last_id, row_base, num_tables,
                                                               cuts);
}

}  // namespace cuembed

#endif  // CUEMBED_INCLUDE_GROUPED_BACKWARD_HPP_
