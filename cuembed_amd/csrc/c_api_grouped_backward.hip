// C ABI: the index work of a GROUP's backward = explicit instantiations of cuembed::GroupedBackwardKeys and
// cuembed::GroupedTableCuts (an extension: the reference's backward takes one table).  The sort, the remap and the
// scatter-add between them are the single-table entry points of c_api_transforms.hip / c_api_backward.hip.
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
}  // namespace

extern "C" {

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
