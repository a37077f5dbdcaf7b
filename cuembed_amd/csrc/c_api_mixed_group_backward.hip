// C ABI: the backward of a group of tables of DIFFERENT widths = explicit instantiations of
// cuembed::EmbeddingBackwardMixedGroup and cuembed::MixedGroupMeanScale (an extension: the reference's backward takes one
// table), and the host arithmetic of the launch shape.  The keys, the sort and the table cuts around the scatter-add are
// the same-width group's entry points (c_api_grouped_backward.hip, c_api_transforms.hip).
#include "c_api_common.hpp"
#include "cuembed/include/mixed_group_backward.hpp"

using cuembed_c_api::Stream;

namespace {
template <typename ElemT, typename IndexT>
void Backward(const void* grad_y, const int* widths_host, const void* table_columns_device, int num_tables,
              int batch_per_table, int64_t nnz, const void* transpose_indices, const void* transpose_sample_ids,
              const void* transpose_remapped_indices, const void* transpose_weights, void* grad_embedding,
              void* inverse_mapping, int64_t capacity_rows, uint32_t* capacity_overflow, cuembed_stream_t stream) {
  cuembed::EmbeddingBackwardMixedGroup<ElemT, IndexT>(
      static_cast<const ElemT*>(grad_y), widths_host, table_columns_device, num_tables, batch_per_table,
      static_cast<int>(nnz), static_cast<const IndexT*>(transpose_indices), static_cast<const IndexT*>(transpose_sample_ids),
      static_cast<const IndexT*>(transpose_remapped_indices), static_cast<const ElemT*>(transpose_weights),
      static_cast<ElemT*>(grad_embedding), static_cast<IndexT*>(inverse_mapping), Stream(stream), capacity_rows,
      capacity_overflow);
}

template <typename ElemT, typename OffsetT>
void MeanScale(const void* grad_y, const int* widths_host, const void* table_columns_device, const void* offsets,
               const void* weights, int num_tables, int batch_per_table, int num_hots, void* out, cuembed_stream_t stream) {
  cuembed::MixedGroupMeanScale<ElemT, OffsetT>(static_cast<const ElemT*>(grad_y), widths_host, table_columns_device,
                                               static_cast<const OffsetT*>(offsets), static_cast<const ElemT*>(weights),
                                               num_tables, batch_per_table, num_hots, static_cast<ElemT*>(out),
                                               Stream(stream));
}
}  // namespace

extern "C" {

void cuembed_embedding_backward_mixed_group(const void* grad_y, int elem_type, const int* widths_host,
                                            const void* table_columns_device, int num_tables, int batch_per_table,
                                            int64_t nnz, const void* transpose_indices, const void* transpose_sample_ids,
                                            const void* transpose_remapped_indices, int index_type,
                                            const void* transpose_weights, void* grad_embedding, void* inverse_mapping,
                                            int64_t capacity_rows, uint32_t* capacity_overflow, cuembed_stream_t stream) {
  CUEMBED_ASSERT(nnz >= 0 && nnz <= INT_MAX);
  const bool ok = cuembed_c_api::DispatchTypes<true>(elem_type, index_type, [&](auto elem, auto index) {
    Backward<typename decltype(elem)::type, typename decltype(index)::type>(
        grad_y, widths_host, table_columns_device, num_tables, batch_per_table, nnz, transpose_indices,
        transpose_sample_ids, transpose_remapped_indices, transpose_weights, grad_embedding, inverse_mapping, capacity_rows,
        capacity_overflow, stream);
  });
  if (!ok) CUEMBED_C_API_BAD_TYPE();
}

void cuembed_mixed_group_mean_scale(const void* grad_y, int elem_type, const int* widths_host,
                                    const void* table_columns_device, const void* offsets, int offset_type,
                                    const void* weights, int num_tables, int batch_per_table, int num_hots, void* out,
                                    cuembed_stream_t stream) {
  CUEMBED_ASSERT(offsets == nullptr || offset_type == CUEMBED_I32 || offset_type == CUEMBED_I64);
#define MS(E, O) \
  MeanScale<E, O>(grad_y, widths_host, table_columns_device, offsets, weights, num_tables, batch_per_table, num_hots, out, stream)
  switch ((elem_type << 1) | (offsets ? offset_type : 0)) {
    case 0: MS(float, int32_t); break;
    case 1: MS(float, int64_t); break;
    case 2: MS(__half, int32_t); break;
    case 3: MS(__half, int64_t); break;
    case 4: MS(__hip_bfloat16, int32_t); break;
    case 5: MS(__hip_bfloat16, int64_t); break;
    default: CUEMBED_C_API_BAD_TYPE();
  }
#undef MS
}

void cuembed_mixed_group_backward_launch_shape(const int* widths_host, int num_tables, int elem_type, int64_t nnz,
                                               int is_weighted, size_t pointer_bits, int compute_units, int xcds,
                                               int* out) {
  namespace d = cuembed::detail;
  CUEMBED_ASSERT(elem_type == CUEMBED_F32 || elem_type == CUEMBED_F16 || elem_type == CUEMBED_BF16);
  CUEMBED_ASSERT(out != nullptr && nnz >= 0 && nnz <= INT_MAX);
  const int elem_bytes = elem_type == CUEMBED_F32 ? 4 : 2;
  d::DeviceShape dev = compute_units > 0 ? d::Mi355xShape() : d::CurrentDeviceShape();
  if (compute_units > 0) dev.compute_units = compute_units;
  if (xcds > 0) dev.xcds = xcds;
  const d::MixedGroupColumns columns =
      d::PlanMixedGroupColumns(widths_host, num_tables, elem_bytes, static_cast<uintptr_t>(pointer_bits));
  const d::MixedScatterShape m = d::PlanMixedScatter(columns, nnz, is_weighted != 0, elem_bytes, dev);
  out[0] = m.split.elems_per_lane;
  out[1] = m.scatter.lanes;
  out[2] = m.scatter.segments_per_block;
  out[3] = m.scatter.segment_len;
  out[4] = m.scatter.slices;
  out[5] = static_cast<int>(m.scatter.grid_blocks);
  out[6] = static_cast<int>(m.lds);
  out[7] = m.block_len;
  out[8] = columns.max_width;
  out[9] = columns.out_width;
}

}  // extern "C"
