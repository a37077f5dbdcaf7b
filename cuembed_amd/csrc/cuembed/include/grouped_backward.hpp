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
//
// That pipeline is the backward of SUM pooling with respect to the tables.  Two more launches cover the rest
// (grouped_train_kernels.hpp):
//
//   GroupedMeanScale(grad_y, ...)              mean pooling: grad_y times each bag's mean factor, then the pipeline above
//   EmbeddingWeightGradGrouped(...)            the gradient of a weighted sum with respect to the per-lookup weights
//
// Every function runs on the caller's stream, allocates nothing and reads nothing back.
#ifndef CUEMBED_INCLUDE_GROUPED_BACKWARD_HPP_
#define CUEMBED_INCLUDE_GROUPED_BACKWARD_HPP_

#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "cuembed/include/cuembed_assert.hpp"
#include "cuembed/include/group_host_plan.hpp"
#include "cuembed/include/grouped_backward_kernels.hpp"
#include "cuembed/include/grouped_lookup.hpp"
#include "cuembed/include/grouped_train_kernels.hpp"

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
 * pipeline's own limit) and num_tables * batch_per_table <= INT_MAX.  (cuembed::CheckIndices, index_check.hpp, finds
 * and repairs such ids and offsets on the device, in front of this call.)
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

/**
 * @brief Gradient of a weighted sum-forward of a GROUP with respect to the per-lookup weights, in one launch:
 * for lookup p of bag t * batch_per_table + b, grad_weights[p] = dot(tables[t][indices[p], :], grad_y[b, t, :]) in fp32,
 * rounded once.  Bit-identical to num_tables calls of EmbeddingWeightGrad on grad_y[:, t, :] made contiguous.
 *
 * The argument contract is EmbeddingForwardGrouped's: `tables_host` (HOST memory, read here: the least aligned table
 * and grad_y decide the access width) and `tables_device` (the same pointers in DEVICE memory, read by the kernel);
 * CSR (offsets[num_tables * batch_per_table + 1], num_hots == 0) or fixed hotness (offsets == nullptr, indices
 * [num_tables, batch_per_table, num_hots]); grad_y [batch_per_table, num_tables, embed_width] contiguous; grad_weights
 * has the layout of indices.  Asynchronous on `stream`, allocates nothing, reads nothing back.
 */
template <typename InputT, typename IndexT, typename OffsetT>
void EmbeddingWeightGradGrouped(const InputT* const* tables_host,
                                const InputT* const* tables_device,
                                const int num_tables,
                                const int embed_width,
                                const IndexT* indices,
                                const OffsetT* offsets,
                                const InputT* grad_y,
                                const int batch_per_table,
                                const int num_hots,
                                InputT* grad_weights,
                                const hipStream_t stream = 0) {
  using ElemT = detail::DeviceElemT<GetElemT<InputT>>;
  CUEMBED_ASSERT(tables_host != nullptr && tables_device != nullptr);
  CUEMBED_ASSERT((offsets != nullptr && num_hots == 0) || (offsets == nullptr && num_hots > 0));
  const int batch = detail::GroupedBatch(num_tables, batch_per_table);
  if (batch <= 0) return;
  CUEMBED_ASSERT(indices != nullptr && grad_y != nullptr && grad_weights != nullptr);
  const void* bits = detail::GroupAlignmentBits(reinterpret_cast<const void* const*>(tables_host), num_tables);
  const detail::RowSplit split = detail::SplitRow<ElemT>(embed_width, bits, grad_y);
  const detail::LaneGroupShape shape = detail::PlanLaneGroups(split.lanes_per_row, batch);
  const dim3 block = shape.block, grid = shape.grid;
  const ElemT* const* tables = reinterpret_cast<const ElemT* const*>(tables_device);
  const ElemT* gy = reinterpret_cast<const ElemT*>(grad_y);
  ElemT* gw = reinterpret_cast<ElemT*>(grad_weights);
  detail::WithLaneWidth<ElemT>(split.elems_per_lane, [&](auto n) {
    detail::WeightGradGroupedKernel<ElemT, IndexT, OffsetT, decltype(n)::value><<<grid, block, 0, stream>>>(
        tables, batch_per_table, num_tables, embed_width, batch, indices, offsets, num_hots, gy, gw);
  });
}

/**
 * @brief grad_y of a MEAN-pooled group -> grad_y of the equivalent sum-pooled one, in one launch:
 * out[b, t, :] = InputT(float(grad_y[b, t, :]) * f), f the forward's own mean factor of bag t * batch_per_table + b --
 * 1 / length, or with `weights` 1 / the fp32 sum of the bag's weights; 0 when that denominator is 0.  The backward
 * of a sum-pooled group (GroupedBackwardKeys ... EmbeddingBackward) on `out` is then the backward of the mean.
 *
 * CSR (offsets[num_tables * batch_per_table + 1], num_hots == 0) or fixed hotness (offsets == nullptr, num_hots > 0:
 * every bag has num_hots lookups; weighted bags still sum their weights).  weights: the layout of the indices, or
 * nullptr.  grad_y and out are [batch_per_table, num_tables, embed_width] contiguous; out may be grad_y.
 * Asynchronous on `stream`, allocates nothing, reads nothing back.
 */
template <typename InputT, typename OffsetT>
void GroupedMeanScale(const InputT* grad_y,
                      const OffsetT* offsets,
                      const InputT* weights,
                      const int num_tables,
                      const int batch_per_table,
                      const int embed_width,
                      const int num_hots,
                      InputT* out,
                      const hipStream_t stream = 0) {
  using ElemT = detail::DeviceElemT<GetElemT<InputT>>;
  CUEMBED_ASSERT((offsets != nullptr && num_hots == 0) || (offsets == nullptr && num_hots > 0));
  const int rows = detail::GroupedBatch(num_tables, batch_per_table);
  if (rows <= 0) return;
  CUEMBED_ASSERT(grad_y != nullptr && out != nullptr);
  const detail::RowSplit split = detail::SplitRow<ElemT>(embed_width, grad_y, out);
  const detail::LaneGroupShape shape = detail::PlanLaneGroups(split.lanes_per_row, rows);
  const dim3 block = shape.block, grid = shape.grid;
  const ElemT* gy = reinterpret_cast<const ElemT*>(grad_y);
  const ElemT* w = reinterpret_cast<const ElemT*>(weights);
  ElemT* o = reinterpret_cast<ElemT*>(out);
  detail::WithLaneWidth<ElemT>(split.elems_per_lane, [&](auto n) {
    constexpr int N = decltype(n)::value;
    if (w != nullptr)
      detail::GroupedMeanScaleKernel<ElemT, OffsetT, N, true><<<grid, block, 0, stream>>>(
          gy, offsets, w, batch_per_table, num_tables, embed_width, rows, num_hots, o);
    else
      detail::GroupedMeanScaleKernel<ElemT, OffsetT, N, false><<<grid, block, 0, stream>>>(
          gy, offsets, w, batch_per_table, num_tables, embed_width, rows, num_hots, o);
  });
}

}  // namespace cuembed

#endif  // CUEMBED_INCLUDE_GROUPED_BACKWARD_HPP_
