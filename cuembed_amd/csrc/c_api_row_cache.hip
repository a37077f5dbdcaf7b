// C ABI: the device-managed row cache = cuembed::RowCachePrefetch / RowCacheFlush (an extension: the reference lists an
// embedding cache as future work).
#include "c_api_common.hpp"
#define CUEMBED_ROW_CACHE_SORT_IN_LIBRARY
#include "cuembed/include/row_cache.hpp"

using cuembed_c_api::Stream;

namespace {

cuembed::RowCache CacheOf(void* table, void* cache_rows, int64_t row_bytes, int64_t num_rows, int num_sets,
                          int64_t* tags, uint32_t* stamps, void* dirty, int32_t* slot_of_row, uint64_t* words,
                          float* state = nullptr, float* state_cache = nullptr, int64_t state_row_bytes = 0,
                          float* state2 = nullptr, float* state2_cache = nullptr, int64_t state2_row_bytes = 0) {
  cuembed::RowCache c;
  c.table = table;
  c.cache_rows = cache_rows;
  c.row_bytes = row_bytes;
  c.num_rows = num_rows;
  c.num_sets = num_sets;
  c.tags = tags;
  c.stamps = stamps;
  c.dirty = static_cast<uint8_t*>(dirty);
  c.slot_of_row = slot_of_row;
  c.words = reinterpret_cast<unsigned long long*>(words);
  c.state = state;
  c.state_cache = state_cache;
  c.state_row_bytes = state_row_bytes;
  c.state2 = state2;
  c.state2_cache = state2_cache;
  c.state2_row_bytes = state2_row_bytes;
  return c;
}

void Prefetch(const cuembed::RowCache& c, const void* indices, int index_type, int64_t nnz, int64_t num_valid,
              const void* count, int count_is_int64, const void* last_id, int for_update, char* work, size_t* lwork,
              cuembed_stream_t stream) {
  cuembed::RowCacheCounts counts;
  counts.num_valid = num_valid;
  counts.count = count;
  counts.count_is_int64 = count_is_int64 != 0;
  counts.last_id = last_id;
  if (index_type == CUEMBED_I32)
    cuembed::RowCachePrefetch<int32_t>(c, static_cast<const int32_t*>(indices), nnz, counts, for_update != 0, work, lwork,
                                       Stream(stream));
  else if (index_type == CUEMBED_I64)
    cuembed::RowCachePrefetch<int64_t>(c, static_cast<const int64_t*>(indices), nnz, counts, for_update != 0, work, lwork,
                                       Stream(stream));
  else
    CUEMBED_C_API_BAD_TYPE();
}

}  // namespace

extern "C" {

size_t cuembed_row_cache_workspace_bytes(int64_t nnz, int64_t num_rows, int num_sets) {
  return cuembed::RowCacheWorkspaceBytes(nnz, num_rows, num_sets);
}

void cuembed_row_cache_prefetch(void* table, void* cache_rows, int64_t row_bytes, int64_t num_rows, int num_sets,
                                int64_t* tags, uint32_t* stamps, void* dirty, int32_t* slot_of_row, uint64_t* words,
                                const void* indices, int index_type, int64_t nnz, int64_t num_valid, const void* count,
                                int count_is_int64, const void* last_id, int for_update, char* work, size_t* lwork,
                                cuembed_stream_t stream) {
  Prefetch(CacheOf(table, cache_rows, row_bytes, num_rows, num_sets, tags, stamps, dirty, slot_of_row, words), indices,
           index_type, nnz, num_valid, count, count_is_int64, last_id, for_update, work, lwork, stream);
}

void cuembed_row_cache_prefetch_with_state(void* table, void* cache_rows, int64_t row_bytes, int64_t num_rows,
                                           int num_sets, int64_t* tags, uint32_t* stamps, void* dirty,
                                           int32_t* slot_of_row, uint64_t* words, const void* indices, int index_type,
                                           int64_t nnz, int64_t num_valid, const void* count, int count_is_int64,
                                           const void* last_id, int for_update, char* work, size_t* lwork,
                                           cuembed_stream_t stream, float* state, float* state_cache,
                                           int64_t state_row_bytes) {
  Prefetch(CacheOf(table, cache_rows, row_bytes, num_rows, num_sets, tags, stamps, dirty, slot_of_row, words, state,
                   state_cache, state_row_bytes),
           indices, index_type, nnz, num_valid, count, count_is_int64, last_id, for_update, work, lwork, stream);
}

void cuembed_row_cache_flush(void* table, void* cache_rows, int64_t row_bytes, int64_t num_rows, int num_sets,
                             int64_t* tags, uint32_t* stamps, void* dirty, int32_t* slot_of_row, uint64_t* words,
                             cuembed_stream_t stream) {
  cuembed::RowCacheFlush(CacheOf(table, cache_rows, row_bytes, num_rows, num_sets, tags, stamps, dirty, slot_of_row,
                                 words),
                         Stream(stream));
}

void cuembed_row_cache_flush_with_state(void* table, void* cache_rows, int64_t row_bytes, int64_t num_rows, int num_sets,
                                        int64_t* tags, uint32_t* stamps, void* dirty, int32_t* slot_of_row,
                                        uint64_t* words, cuembed_stream_t stream, float* state, float* state_cache,
                                        int64_t state_row_bytes) {
  cuembed::RowCacheFlush(CacheOf(table, cache_rows, row_bytes, num_rows, num_sets, tags, stamps, dirty, slot_of_row,
                                 words, state, state_cache, state_row_bytes),
                         Stream(stream));
}

void cuembed_row_cache_prefetch_with_states(void* table, void* cache_rows, int64_t row_bytes, int64_t num_rows,
                                            int num_sets, int64_t* tags, uint32_t* stamps, void* dirty,
                                            int32_t* slot_of_row, uint64_t* words, const void* indices, int index_type,
                                            int64_t nnz, int64_t num_valid, const void* count, int count_is_int64,
                                            const void* last_id, int for_update, char* work, size_t* lwork,
                                            cuembed_stream_t stream, float* state, float* state_cache,
                                            int64_t state_row_bytes, float* state2, float* state2_cache,
                                            int64_t state2_row_bytes) {
  Prefetch(CacheOf(table, cache_rows, row_bytes, num_rows, num_sets, tags, stamps, dirty, slot_of_row, words, state,
                   state_cache, state_row_bytes, state2, state2_cache, state2_row_bytes),
           indices, index_type, nnz, num_valid, count, count_is_int64, last_id, for_update, work, lwork, stream);
}

void cuembed_row_cache_flush_with_states(void* table, void* cache_rows, int64_t row_bytes, int64_t num_rows,
                                         int num_sets, int64_t* tags, uint32_t* stamps, void* dirty,
                                         int32_t* slot_of_row, uint64_t* words, cuembed_stream_t stream, float* state,
                                         float* state_cache, int64_t state_row_bytes, float* state2,
                                         float* state2_cache, int64_t state2_row_bytes) {
  cuembed::RowCacheFlush(CacheOf(table, cache_rows, row_bytes, num_rows, num_sets, tags, stamps, dirty, slot_of_row,
                                 words, state, state_cache, state_row_bytes, state2, state2_cache, state2_row_bytes),
                         Stream(stream));
}

int cuembed_cache_set_of(int64_t row, int num_sets) {
  return static_cast<int>(cuembed::CacheSetOf(row, static_cast<uint32_t>(num_sets)));
}

}  // extern "C"
