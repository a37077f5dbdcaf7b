// C ABI: the device-side index check = explicit instantiations of cuembed::CheckIndices (an extension; the reference
// trusts its indices and offsets).
#include "c_api_common.hpp"
#include "cuembed/include/index_check.hpp"

using cuembed_c_api::Stream;

namespace {
template <typename IndexT, typename OffsetT>
void Check(const void* indices, const void* offsets, int64_t nnz, const int64_t* row_base, int64_t num_rows,
           int num_tables, int batch_per_table, int num_hots, int64_t* report, void* indices_out, void* offsets_out,
           char* work, size_t* lwork, cuembed_stream_t stream) {
  cuembed::CheckIndices<IndexT, OffsetT>(static_cast<const IndexT*>(indices), static_cast<const OffsetT*>(offsets), nnz,
                                         row_base, num_rows, num_tables, batch_per_table, num_hots, report,
                                         static_cast<IndexT*>(indices_out), static_cast<OffsetT*>(offsets_out), work,
                                         lwork, Stream(stream));
}
}  // namespace

extern "C" {

void cuembed_check_indices(const void* indices, int index_type, const void* offsets, int offset_type, int64_t nnz,
                           const int64_t* row_base, int64_t num_rows, int num_tables, int batch_per_table, int num_hots,
                           int64_t* report, void* indices_out, void* offsets_out, char* work, size_t* lwork,
                           cuembed_stream_t stream) {
#define CUEMBED_CHECK(INDEX, OFFSET)                                                                                 \
  Check<INDEX, OFFSET>(indices, offsets, nnz, row_base, num_rows, num_tables, batch_per_table, num_hots, report,     \
                       indices_out, offsets_out, work, lwork, stream)
  if (index_type != CUEMBED_I32 && index_type != CUEMBED_I64) CUEMBED_C_API_BAD_TYPE();
  if (offset_type != CUEMBED_I32 && offset_type != CUEMBED_I64) CUEMBED_C_API_BAD_TYPE();
  if (index_type == CUEMBED_I32) {
    if (offset_type == CUEMBED_I32) CUEMBED_CHECK(int32_t, int32_t);
    else CUEMBED_CHECK(int32_t, int64_t);
  } else {
    if (offset_type == CUEMBED_I32) CUEMBED_CHECK(int64_t, int32_t);
    else CUEMBED_CHECK(int64_t, int64_t);
  }
#undef CUEMBED_CHECK
}

}  // extern "C"
