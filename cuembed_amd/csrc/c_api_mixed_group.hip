// C ABI: the forward on a group of tables of DIFFERENT widths in one launch = explicit instantiations of
// cuembed::EmbeddingForwardMixedGroup (an extension: the reference's entry points take one table), and the host
// arithmetic that goes with it (descriptor size and contents, launch shape).
#include "c_api_common.hpp"
#include "cuembed/include/mixed_group_lookup.hpp"

using cuembed::CombineMode;
using cuembed_c_api::Stream;

namespace {
template <typename ElemT, typename IndexT, typename OffsetT>
void Forward(const void* const* tables_host, const void* const* tables_device, const int* widths_host,
             const void* descriptor_device, int num_tables, const void* indices, const void* offsets, const void* weights,
             int batch_per_table, int num_hots, CombineMode mode, void* ret, const cuembed::ForwardOptions& options,
             cuembed_stream_t stream) {
  cuembed::EmbeddingForwardMixedGroup<ElemT, ElemT, IndexT, OffsetT>(
      reinterpret_cast<const ElemT* const*>(tables_host), reinterpret_cast<const ElemT* const*>(tables_device), widths_host,
      descriptor_device, num_tables, static_cast<const IndexT*>(indices), static_cast<const OffsetT*>(offsets),
      static_cast<const ElemT*>(weights), batch_per_table, num_hots, mode, static_cast<ElemT*>(ret), Stream(stream),
      options);
}

int ElemBytes(int elem_type) {
  CUEMBED_ASSERT(elem_type == CUEMBED_F32 || elem_type == CUEMBED_F16 || elem_type == CUEMBED_BF16);
  return elem_type == CUEMBED_F32 ? 4 : 2;
}
}  // namespace

extern "C" {

void cuembed_embedding_forward_mixed_group(const void* const* tables_host, const void* const* tables_device,
                                           const int* widths_host, const void* descriptor_device, int num_tables,
                                           int elem_type, const void* indices, int index_type, const void* offsets,
                                           int offset_type, const void* weights, int batch_per_table, int num_hots,
                                           int mode, void* ret, int row_load_policy, cuembed_stream_t stream) {
  cuembed::ForwardOptions options;   // (not the process-wide defaults: one order, no device decision, no sample order)
  options.row_loads = cuembed::GetForwardRowLoadPolicy();
  CUEMBED_ASSERT(row_load_policy <= 1);
  if (row_load_policy >= 0) options.row_loads = static_cast<cuembed::RowLoadPolicy>(row_load_policy);
  CUEMBED_ASSERT(mode == CUEMBED_SUM || mode == CUEMBED_MEAN);
  const CombineMode m = mode == CUEMBED_SUM ? CombineMode::kSum : CombineMode::kMean;
  CUEMBED_ASSERT(index_type == CUEMBED_I32 || index_type == CUEMBED_I64);
  CUEMBED_ASSERT(offsets == nullptr || offset_type == CUEMBED_I32 || offset_type == CUEMBED_I64);
#define FWD(E, I, O)                                                                                               \
  Forward<E, I, O>(tables_host, tables_device, widths_host, descriptor_device, num_tables, indices, offsets, weights, \
                   batch_per_table, num_hots, m, ret, options, stream)
  switch ((elem_type << 2) | (index_type << 1) | (offsets ? offset_type : 0)) {
    case 0: FWD(float, int32_t, int32_t); break;
    case 1: FWD(float, int32_t, int64_t); break;
    case 2: FWD(float, int64_t, int32_t); break;
    case 3: FWD(float, int64_t, int64_t); break;
    case 4: FWD(__half, int32_t, int32_t); break;
    case 5: FWD(__half, int32_t, int64_t); break;
    case 6: FWD(__half, int64_t, int32_t); break;
    case 7: FWD(__half, int64_t, int64_t); break;
    case 8: FWD(__hip_bfloat16, int32_t, int32_t); break;
    case 9: FWD(__hip_bfloat16, int32_t, int64_t); break;
    case 10: FWD(__hip_bfloat16, int64_t, int32_t); break;
    case 11: FWD(__hip_bfloat16, int64_t, int64_t); break;
    default: CUEMBED_C_API_BAD_TYPE();
  }
#undef FWD
}

size_t cuembed_mixed_group_descriptor_bytes(int num_tables) { return cuembed::MixedGroupDescriptorBytes(num_tables); }

int cuembed_fill_mixed_group_descriptor(const int* widths_host, int num_tables, int elem_bytes, int lane_bytes,
                                        int batch_per_table, int block_threads, void* host_blob) {
  return cuembed::FillMixedGroupDescriptor(widths_host, num_tables, elem_bytes, lane_bytes, batch_per_table,
                                           block_threads, host_blob);
}

void cuembed_mixed_group_launch_shape(const int* widths_host, int num_tables, int elem_type, int index_type,
                                      int batch_per_table, int num_hots, int is_weighted, size_t pointer_bits, int* out) {
  namespace d = cuembed::detail;
  const int elem_bytes = ElemBytes(elem_type);
  CUEMBED_ASSERT(index_type == CUEMBED_I32 || index_type == CUEMBED_I64);
  CUEMBED_ASSERT(num_hots >= 0 && out != nullptr);
  const int lane_bytes = d::MixedGroupLaneBytesOfBits(static_cast<uintptr_t>(pointer_bits), widths_host, num_tables, elem_bytes);
  const d::MixedGroupPlan plan =
      d::PlanMixedGroup(widths_host, num_tables, elem_bytes, lane_bytes, batch_per_table, d::kMixedGroupBlockThreads, nullptr);
  const size_t stage_bytes = d::MixedGroupStageBytes(plan, num_hots == 0, num_hots, index_type == CUEMBED_I32 ? 4 : 8,
                                                     is_weighted ? elem_bytes : 0);
  out[0] = lane_bytes / elem_bytes;
  out[1] = d::kMixedGroupBlockThreads;
  out[2] = plan.grid;
  out[3] = plan.out_width;
  out[4] = static_cast<int>(stage_bytes);
  out[5] = stage_bytes > 0 ? 1 : 0;
  out[6] = plan.max_slots;
}

}  // extern "C"
