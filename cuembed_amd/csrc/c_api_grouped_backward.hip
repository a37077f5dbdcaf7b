// C ABI: the index work of a GROUP's backward = explicit instantiations of cuembed::GroupedBackwardKeys and
// cuembed::GroupedTableCuts (an extension: the reference's backward takes one table).  The sort, the remap and the
// scatter-add between them are the single-table entry points of c_api_transforms.hip / c_api_backward.hip.
// Beside them: cuembed::EmbeddingWeightGradGrouped (the per-lookup weight gradient of a group) and
// cuembed::GroupedMeanScale (grad_y of a mean-pooled group -> grad_y of the sum-pooled one).
#include "c_api_common.hpp"
#include "cuembed/include/grouped_backward.hpp"

using cuembed_c_api::Stream;

namespace {
template <typename IndexT, typename OffsetT, typename KeyT>
void Keys(const void* indices, const void* offsets, const int64_t* row_base, int num_tables, int batch_per_table,
          int num_hots, int64_t nnz, void* keys, void* sample_ids, cuembed_stream_t stream) {
  cuembed::GroupedBackwardKeys<IndexT, OffsetT, KeyT>(static_cast<const IndexT*>(indices),
                                                      static_cast<const OffsetT*>(offsets), row_base, num_tables,
                                                      batch_per_table, num_hots, nnz, static_cast<KeyT*>(keys),
                                                      static_cast<KeyT*>(sample_ids), Stream(stream));
}

template <typename ElemT, typename IndexT, typename OffsetT>
void WeightGrad(const void* const* tables_host, const void* const* tables_device, int num_tables, int embed_width,
                const void* indices, const void* offsets, const void* grad_y, int batch_per_table, int num_hots,
                void* grad_weights, cuembed_stream_t stream) {
  cuembed::EmbeddingWeightGradGrouped<ElemT, IndexT, OffsetT>(
      reinterpret_cast<const ElemT* const*>(tables_host), reinterpret_cast<const ElemT* const*>(tables_device), num_tables,
      embed_width, static_cast<const IndexT*>(indices), static_cast<const OffsetT*>(offsets),
      static_cast<const ElemT*>(grad_y), batch_per_table, num_hots, static_cast<ElemT*>(grad_weights), Stream(stream));
}

template <typename ElemT, typename OffsetT>
void MeanScale(const void* grad_y, const void* offsets, const void* weights, int num_tables, int batch_per_table,
               int embed_width, int num_hots, void* out, cuembed_stream_t stream) {
  cuembed::GroupedMeanScale<ElemT, OffsetT>(static_cast<const ElemT*>(grad_y), static_cast<const OffsetT*>(offsets),
                                            static_cast<const ElemT*>(weights), num_tables, batch_per_table, embed_width,
                                            num_hots, static_cast<ElemT*>(out), Stream(stream));
}
}  // namespace

extern "C" {

void cuembed_embedding_weight_grad_grouped(const void* const* tables_host, const void* const* tables_device,
                                           int num_tables, int elem_type, int embed_width, const void* indices,
                                           int index_type, const void* offsets, int offset_type, const void* grad_y,
                                           int batch_per_table, int num_hots, void* grad_weights,
                                           cuembed_stream_t stream) {
  CUEMBED_ASSERT(index_type == CUEMBED_I32 || index_type == CUEMBED_I64);
  CUEMBED_ASSERT(offsets == nullptr || offset_type == CUEMBED_I32 || offset_type == CUEMBED_I64);
#define WG(E, I, O)                                                                                                 \
  WeightGrad<E, I, O>(tables_host, tables_device, num_tables, embed_width, indices, offsets, grad_y, batch_per_table, \
                      num_hots, grad_weights, stream)
  switch ((elem_type << 2) | (index_type << 1) | (offsets ? offset_type : 0)) {
    case 0: WG(float, int32_t, int32_t); break;
    case 1: WG(float, int32_t, int64_t); break;
    case 2: WG(float, int64_t, int32_t); break;
    case 3: WG(float, int64_t, int64_t); break;
    case 4: WG(__half, int32_t, int32_t); break;
    case 5: WG(__half, int32_t, int64_t); break;
    case 6: WG(__half, int64_t, int32_t); break;
    case 7: WG(__half, int64_t, int64_t); break;
    case 8: WG(__hip_bfloat16, int32_t, int32_t); break;
    case 9: WG(__hip_bfloat16, int32_t, int64_t); break;
    case 10: WG(__hip_bfloat16, int64_t, int32_t); break;
    case 11: WG(__hip_bfloat16, int64_t, int64_t); break;
    default: CUEMBED_C_API_BAD_TYPE();
  }
#undef WG
}

void cuembed_grouped_mean_scale(const void* grad_y, int elem_type, int embed_width, const void* offsets,
                                int offset_type, const void* weights, int num_tables, int batch_per_table, int num_hots,
                                void* out, cuembed_stream_t stream) {
  CUEMBED_ASSERT(offsets == nullptr || offset_type == CUEMBED_I32 || offset_type == CUEMBED_I64);
#define MS(E, O) \
  MeanScale<E, O>(grad_y, offsets, weights, num_tables, batch_per_table, embed_width, num_hots, out, stream)
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

void cuembed_grouped_backward_keys(const void* indices, int index_type, const void* offsets, int offset_type,
                                   const int64_t* row_base, int num_tables, int batch_per_table, int num_hots,
                                   int64_t nnz, void* keys, void* sample_ids, int key_type, cuembed_stream_t stream) {
  CUEMBED_ASSERT(index_type == CUEMBED_I32 || index_type == CUEMBED_I64);
  CUEMBED_ASSERT(key_type == CUEMBED_I32 || key_type == CUEMBED_I64);
  CUEMBED_ASSERT(offsets == nullptr || offset_type == CUEMBED_I32 || offset_type == CUEMBED_I64);
#define KEYS(I, O, K) \
  Keys<I, O, K>(indices, offsets, row_base, num_tables, batch_per_table, num_hots, nnz, keys, sample_ids, stream)
  switch ((key_type << 2) | (index_type << 1) | (offsets ? offset_type : 0)) {
    case 0: KEYS(int32_t, int32_t, int32_t); break;
    case 1: KEYS(int32_t, int64_t, int32_t); break;
    case 2: KEYS(int64_t, int32_t, int32_t); break;
    case 3: KEYS(int64_t, int64_t, int32_t); break;
    case 4: KEYS(int32_t, int32_t, int64_t); break;
    case 5: KEYS(int32_t, int64_t, int64_t); break;
    case 6: KEYS(int64_t, int32_t, int64_t); break;
    case 7: KEYS(int64_t, int64_t, int64_t); break;
    default: CUEMBED_C_API_BAD_TYPE();
  }
#undef KEYS
}

void cuembed_grouped_table_cuts(const void* inverse_mapping, int index_type, int64_t capacity, int64_t count,
                                const void* count_word, int count_word_is_64, const void* last_id,
                                const int64_t* row_base, int num_tables, int64_t* cuts, cuembed_stream_t stream) {
  if (index_type == CUEMBED_I32) {
    cuembed::GroupedTableCuts<int32_t>(static_cast<const int32_t*>(inverse_mapping), capacity, count, count_word,
                                       count_word_is_64 != 0, static_cast<const int32_t*>(last_id), row_base, num_tables,
                                       cuts, Stream(stream));
  } else if (index_type == CUEMBED_I64) {
    cuembed::GroupedTableCuts<int64_t>(static_cast<const int64_t*>(inverse_mapping), capacity, count, count_word,
                                       count_word_is_64 != 0, static_cast<const int64_t*>(last_id), row_base, num_tables,
                                       cuts, Stream(stream));
  } else {
    CUEMBED_C_API_BAD_TYPE();
  }
}

}  // extern "C"
