// MI355X (gfx950 / CDNA4) embedding lookup -- the backward of a group of tables of DIFFERENT widths (host API; an
// extension: the reference's backward takes one table, grouped_backward.hpp is the same-width group).
//
// The group of mixed_group_lookup.hpp -- T tables of any widths, bag g = t * B + b, out [B, D], table t at columns
// [c_t, c_t + W_t) -- is trained through the same-width group's pipeline; only the scatter-add is new:
//
//   GroupedBackwardKeys(...)                   keys[p] = row_base[t] + indices[p], sample_ids[p] = b * T + t   (unchanged)
//   Transpose(sample_ids, keys, weights, ...)  with transpose_remapped_indices                                  (unchanged)
//   EmbeddingBackwardMixedGroup(grad_y [B, D], ...)   one scatter-add for all widths
//   GroupedTableCuts(...)                      where each table's entries begin                                 (unchanged)
//
//   MixedGroupMeanScale(grad_y, ...)           mean pooling: grad_y times each bag's mean factor, in front of the above
//
// The result is a COMPRESSED gradient PADDED to the widest table: inverse_mapping[k] ascending global row ids, the
// gradient of entry k in grad_embedding[k * W_max, k * W_max + W_t) for the table t its id falls in.  Columns >= W_t of
// an entry are unspecified (untouched or zero, see mixed_group_scatter_kernels.hpp); nothing in the library reads them.
// The count is device-side only: transpose_remapped_indices[nnz - 1] + 1.
//
// Lane width: ONE value for the launch, the widest of 16 / 8 / 4 bytes that the grad_y base, the grad_embedding base,
// D * sizeof, every c_t * sizeof, every W_t * sizeof and W_max * sizeof allow.
// Limits (CUEMBED_ASSERT): T * B <= INT_MAX, nnz <= INT_MAX, W_max / N <= 1024 lanes, and B * D / N < 2^31 -- a staged
// lookup carries its source offset in lane units in 31 bits.  The per-table (c_t, W_t) array is read from device
// memory through L1, not staged in LDS: there is no bound on T beyond those.
// Every function runs on the caller's stream, allocates nothing, reads nothing back and can be captured.
#ifndef CUEMBED_INCLUDE_MIXED_GROUP_BACKWARD_HPP_
#define CUEMBED_INCLUDE_MIXED_GROUP_BACKWARD_HPP_

#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>
#include <type_traits>

#include "cuembed/include/cuembed_assert.hpp"
#include "cuembed/include/embedding_backward.hpp"
#include "cuembed/include/group_host_plan.hpp"
#include "cuembed/include/index_kernels.hpp"
#include "cuembed/include/mixed_group_scatter_kernels.hpp"

namespace cuembed {

namespace detail {

//! Launch shape of MixedGroupScatterAddKernel: PlanScatter's for W_max (so SetBackwardTuning applies), with the LDS
//! of MixedScatterStage.
struct MixedScatterShape {
  ScatterShape scatter;
  RowSplit split;
  size_t lds;
  int block_len;   //!< lookups per workgroup
};

inline MixedScatterShape PlanMixedScatter(const MixedGroupColumns& columns, const int64_t nnz, const bool weighted,
                                          const int elem_bytes, const DeviceShape& dev) {
  MixedScatterShape m;
  m.split.elems_per_lane = columns.lane_bytes / elem_bytes;
  m.split.lanes_per_row = columns.max_width / m.split.elems_per_lane;
  CUEMBED_ASSERT(m.split.lanes_per_row <= kMaxBlockThreads);
  m.split.rows_per_block = m.split.lanes_per_row >= kDefaultBlockThreads ? 1 : kDefaultBlockThreads / m.split.lanes_per_row;
  m.scatter = PlanScatter(columns.max_width, nnz, m.split, weighted, elem_bytes, dev);
  m.lds = MixedScatterStage::Of(m.scatter.segments_per_block, m.scatter.segment_len, m.scatter.lanes,
                                m.split.elems_per_lane, weighted, elem_bytes)
              .bytes;
  m.block_len = m.scatter.segments_per_block * m.scatter.segment_len;
  return m;
}

}  // namespace detail

/**
 * @brief The scatter-add of a mixed-width group: from the index-sorted lookups of ALL tables (Transpose's output on
 * GroupedBackwardKeys' keys and sample ids, with the remapped ids) to the compressed, padded gradient.
 *
 * @param grad_y                      [batch_per_table, D] contiguous, D = sum of widths_host
 * @param widths_host                 [num_tables] elements per row of each table, HOST memory
 * @param table_columns_device        [num_tables][2] int32 = (c_t, W_t) in elements, DEVICE memory, 8-byte aligned; built once
 * @param nnz                         lookups of the batch; nnz <= 0 launches nothing
 * @param transpose_indices           [nnz] sorted global row ids
 * @param transpose_sample_ids        [nnz] b * num_tables + t of each
 * @param transpose_remapped_indices  [nnz] dense ascending ids (the count is the last one + 1)
 * @param transpose_weights           [nnz] or nullptr
 * @param grad_embedding              [capacity, W_max]; rows at and past the count are untouched
 * @param inverse_mapping             [capacity] receives the global row id of every entry
 * @param capacity_rows               > 0: rows the outputs hold -- if the device-side count exceeds it NOTHING is written
 *                                    and *capacity_overflow (a device word the caller zeroed; may be null) is OR-ed with
 *                                    1.  0 = unchecked (nnz rows always suffice).
 *
 * Arithmetic: EmbeddingBackward's default (fp32 partial sums per segment, one rounding per flush, float atomics only
 * for runs that cross a workgroup).  The launch shape is PlanScatter's for W_max: SetBackwardTuning applies.
 */
template <typename GradT, typename IndexT>
void EmbeddingBackwardMixedGroup(const GradT* grad_y,
                                 const int* widths_host,
                                 const void* table_columns_device,
                                 const int num_tables,
                                 const int batch_per_table,
                                 const int nnz,
                                 const IndexT* transpose_indices,
                                 const IndexT* transpose_sample_ids,
                                 const IndexT* transpose_remapped_indices,
                                 const GradT* transpose_weights,
                                 GradT* grad_embedding,
                                 IndexT* inverse_mapping,
                                 const hipStream_t stream = 0,
                                 const int64_t capacity_rows = 0,
                                 uint32_t* capacity_overflow = nullptr) {
  static_assert(std::is_same<GradT, float>::value || std::is_same<GradT, __half>::value ||
                    std::is_same<GradT, __hip_bfloat16>::value,
                "EmbeddingBackwardMixedGroup: gradients must be float, __half or __hip_bfloat16");
  using ElemT = detail::DeviceElemT<GradT>;
  constexpr int kElemBytes = static_cast<int>(sizeof(ElemT));
  CUEMBED_ASSERT(widths_host != nullptr && num_tables >= 1 && batch_per_table >= 0);
  CUEMBED_ASSERT(static_cast<int64_t>(num_tables) * batch_per_table <= INT_MAX);
  CUEMBED_ASSERT(capacity_rows >= 0);
  if (nnz <= 0) return;
  CUEMBED_ASSERT(grad_y != nullptr && grad_embedding != nullptr && inverse_mapping != nullptr);
  CUEMBED_ASSERT(table_columns_device != nullptr && reinterpret_cast<uintptr_t>(table_columns_device) % 8 == 0);
  CUEMBED_ASSERT(transpose_indices != nullptr && transpose_sample_ids != nullptr && transpose_remapped_indices != nullptr);
  const detail::MixedGroupColumns columns = detail::PlanMixedGroupColumns(
      widths_host, num_tables, kElemBytes, reinterpret_cast<uintptr_t>(grad_y) | reinterpret_cast<uintptr_t>(grad_embedding));
  const int lane_elems = columns.lane_bytes / kElemBytes;
  // a staged lookup's source offset, in lane units, shares a word with kRunEndBit
  CUEMBED_ASSERT(static_cast<int64_t>(batch_per_table) * (columns.out_width / lane_elems) < (int64_t{1} << 31));
  const detail::DeviceShape dev = detail::CurrentDeviceShape();
  const bool weighted = transpose_weights != nullptr;
  const detail::MixedScatterShape m = detail::PlanMixedScatter(columns, nnz, weighted, kElemBytes, dev);
  const detail::ScatterShape& s = m.scatter;
  const ElemT* gy = reinterpret_cast<const ElemT*>(grad_y);
  const ElemT* w = reinterpret_cast<const ElemT*>(transpose_weights);
  ElemT* out = reinterpret_cast<ElemT*>(grad_embedding);
  // only the rows that can receive atomics -- the first and the last of every workgroup -- are zeroed, over all W_max columns
  detail::ZeroSharedAndTailRowsKernel<ElemT, IndexT><<<static_cast<unsigned>(s.nz_blocks), 256, 0, stream>>>(
      transpose_remapped_indices, nnz, m.block_len, s.nz_blocks, nnz, 1, columns.max_width, 0, out, nullptr, capacity_rows);
  int seg_shift = -1;
  if ((s.segment_len & (s.segment_len - 1)) == 0)
    for (seg_shift = 0; (1 << seg_shift) < s.segment_len; ++seg_shift) {}
  const detail::QuotientMagic by_tables(num_tables);
  const dim3 block(s.lanes, s.segments_per_block, 1);
  const dim3 grid(static_cast<unsigned>(s.grid_blocks), 1, 1);
  const int2* table_columns = static_cast<const int2*>(table_columns_device);
  const uint32_t row_lanes = static_cast<uint32_t>(columns.out_width / lane_elems);
  detail::WithLaneWidth<ElemT>(lane_elems, [&](auto n) {
    constexpr int N = decltype(n)::value;
    const auto launch = [&](auto weighted_tag, auto window) {
      detail::MixedGroupScatterAddKernel<ElemT, IndexT, N, decltype(weighted_tag)::value, decltype(window)::value>
          <<<grid, block, m.lds, stream>>>(gy, table_columns, static_cast<uint32_t>(num_tables), by_tables.magic,
                                           by_tables.shift, row_lanes, columns.max_width, transpose_remapped_indices,
                                           transpose_sample_ids, w, nnz, s.segment_len, seg_shift, out, s.slices, s.xcds,
                                           transpose_indices, inverse_mapping, capacity_rows, capacity_overflow);
    };
    // window depth as LaunchScatterAdd picks it: column-sliced launches gather mostly from L2, unsliced ones miss
    using Hits = std::integral_constant<int, detail::kBackwardWindowHits>;
    using Misses = std::integral_constant<int, detail::kBackwardWindowMisses>;
    if (weighted) {
      if (s.slices > 1) launch(std::true_type{}, Hits{});
      else launch(std::true_type{}, Misses{});
    } else {
      if (s.slices > 1) launch(std::false_type{}, Hits{});
      else launch(std::false_type{}, Misses{});
    }
  });
}

/**
 * @brief grad_y of a MEAN-pooled mixed group -> grad_y of the equivalent sum-pooled one, in one launch:
 * out[b, c_t + j] = InputT(float(grad_y[b, c_t + j]) * f), f the forward's own mean factor of bag t * batch_per_table + b
 * -- 1 / length, or with `weights` 1 / the fp32 sum of the bag's weights; 0 when that denominator is 0.  Bit-identical
 * to num_tables calls of GroupedMeanScale on one-table groups (aligned buffers), concatenated on dimension 1.
 *
 * CSR (offsets[num_tables * batch_per_table + 1], num_hots == 0) or fixed hotness (offsets == nullptr, num_hots > 0).
 * grad_y and out are [batch_per_table, D] contiguous; out may be grad_y.  table_columns_device as in
 * EmbeddingBackwardMixedGroup.  Asynchronous on `stream`, allocates nothing, reads nothing back.
 */
template <typename InputT, typename OffsetT>
void MixedGroupMeanScale(const InputT* grad_y,
                         const int* widths_host,
                         const void* table_columns_device,
                         const OffsetT* offsets,
                         const InputT* weights,
                         const int num_tables,
                         const int batch_per_table,
                         const int num_hots,
                         InputT* out,
                         const hipStream_t stream = 0) {
  using ElemT = detail::DeviceElemT<GetElemT<InputT>>;
  constexpr int kElemBytes = static_cast<int>(sizeof(ElemT));
  CUEMBED_ASSERT((offsets != nullptr && num_hots == 0) || (offsets == nullptr && num_hots > 0));
  CUEMBED_ASSERT(widths_host != nullptr && num_tables >= 1 && batch_per_table >= 0);
  CUEMBED_ASSERT(static_cast<int64_t>(num_tables) * batch_per_table <= INT_MAX);
  const int rows = num_tables * batch_per_table;
  if (rows <= 0) return;
  CUEMBED_ASSERT(grad_y != nullptr && out != nullptr);
  CUEMBED_ASSERT(table_columns_device != nullptr && reinterpret_cast<uintptr_t>(table_columns_device) % 8 == 0);
  const detail::MixedGroupColumns columns = detail::PlanMixedGroupColumns(
      widths_host, num_tables, kElemBytes, reinterpret_cast<uintptr_t>(grad_y) | reinterpret_cast<uintptr_t>(out));
  const int lane_elems = columns.lane_bytes / kElemBytes;
  const detail::LaneGroupShape shape = detail::PlanLaneGroups(columns.max_width / lane_elems, rows);
  const dim3 block = shape.block, grid = shape.grid;
  const ElemT* gy = reinterpret_cast<const ElemT*>(grad_y);
  const ElemT* w = reinterpret_cast<const ElemT*>(weights);
  ElemT* o = reinterpret_cast<ElemT*>(out);
  const int2* table_columns = static_cast<const int2*>(table_columns_device);
  detail::WithLaneWidth<ElemT>(lane_elems, [&](auto n) {
    constexpr int N = decltype(n)::value;
    if (w != nullptr)
      detail::MixedGroupMeanScaleKernel<ElemT, OffsetT, N, true><<<grid, block, 0, stream>>>(
          gy, table_columns, offsets, w, batch_per_table, num_tables, columns.out_width, rows, num_hots, o);
    else
      detail::MixedGroupMeanScaleKernel<ElemT, OffsetT, N, false><<<grid, block, 0, stream>>>(
          gy, table_columns, offsets, w, batch_per_table, num_tables, columns.out_width, rows, num_hots, o);
  });
}

}  // namespace cuembed

#endif  // CUEMBED_INCLUDE_MIXED_GROUP_BACKWARD_HPP_
