// C ABI: the forward on a group of fused 4-bit tables of DIFFERENT widths in one launch = explicit instantiations of
// cuembed::EmbeddingForwardQuantized4BitMixedGroup (an extension), and the host arithmetic that goes with it (codes per
// lane, descriptor contents, launch shape).  The descriptor's size is cuembed_mixed_group_descriptor_bytes.
#include "c_api_common.hpp"
#include "cuembed/include/quantized_4bit_mixed_group_lookup.hpp"

using cuembed::CombineMode;
using cuembed_c_api::Stream;

namespace {
template <typename OutT, typename IndexT, typename OffsetT>
void Forward(const void* const* tables_host, const void* const* tables_device, const int* widths_host,
             const void* descriptor_device, int num_tables, const void* indices, const void* offsets, const void* weights,
             int batch_per_table, int num_hots, CombineMode mode, void* ret, const cuembed::ForwardOptions& options,
             cuembed_stream_t stream) {
  cuembed::EmbeddingForwardQuantized4BitMixedGroup<OutT, IndexT, OffsetT>(
      reinterpret_cast<const uint8_t* const*>(tables_host), reinterpret_cast<const uint8_t* const*>(tables_device),
      widths_host, descriptor_device, num_tables, static_cast<const IndexT*>(indices),
      static_cast<const OffsetT*>(offsets), static_cast<const OutT*>(weights), batch_per_table, num_hots, mode,
      static_cast<OutT*>(ret), Stream(stream), options);
}
}  // namespace

extern "C" {

void cuembed_embedding_forward_quantized_mixed_group_4bit(const void* const* tables_host,
                                                          const void* const* tables_device, const int* widths_host,
                                                          const void* descriptor_device, int num_tables,
                                                          const void* indices, int index_type, const void* offsets,
                                                          int offset_type, const void* weights, int batch_per_table,
                                                          int num_hots, int mode, void* ret, int out_type,
                                                          int row_load_policy, cuembed_stream_t stream) {
  cuembed::ForwardOptions options;   // (not the process-wide defaults: one order, no device decision, no sample order)
  options.row_loads = cuembed::GetForwardRowLoadPolicy();
  CUEMBED_ASSERT(row_load_policy <= 1);
  if (row_load_policy >= 0) options.row_loads = static_cast<cuembed::RowLoadPolicy>(row_load_policy);
  CUEMBED_ASSERT(mode == CUEMBED_SUM || mode == CUEMBED_MEAN);
  const CombineMode m = mode == CUEMBED_SUM ? CombineMode::kSum : CombineMode::kMean;
  CUEMBED_ASSERT(out_type == CUEMBED_F32 || out_type == CUEMBED_F16);
  CUEMBED_ASSERT(index_type == CUEMBED_I32 || index_type == CUEMBED_I64);
  CUEMBED_ASSERT(offsets == nullptr || offset_type == CUEMBED_I32 || offset_type == CUEMBED_I64);
#define FWD(E, I, O)                                                                                               \
  Forward<E, I, O>(tables_host, tables_device, widths_host, descriptor_device, num_tables, indices, offsets, weights, \
                   batch_per_table, num_hots, m, ret, options, stream)
  switch ((out_type << 2) | (index_type << 1) | (offsets ? offset_type : 0)) {
    case 0: FWD(float, int32_t, int32_t); break;
    case 1: FWD(float, int32_t, int64_t); break;
    case 2: FWD(float, int64_t, int32_t); break;
    case 3: FWD(float, int64_t, int64_t); break;
    case 4: FWD(__half, int32_t, int32_t); break;
    case 5: FWD(__half, int32_t, int64_t); break;
    case 6: FWD(__half, int64_t, int32_t); break;
    case 7: FWD(__half, int64_t, int64_t); break;
    default: CUEMBED_C_API_BAD_TYPE();
  }
#undef FWD
}

int cuembed_quantized_mixed_group_codes_per_lane_4bit(const void* const* tables_host, const int* widths_host,
                                                      int num_tables) {
  return cuembed::Quantized4BitMixedGroupCodesPerLane(tables_host, widths_host, num_tables);
}

int cuembed_fill_quantized_mixed_group_descriptor_4bit(const int* widths_host, int num_tables, int codes_per_lane,
                                                       int batch_per_table, int block_threads, void* host_blob) {
  return cuembed::FillQuantized4BitMixedGroupDescriptor(widths_host, num_tables, codes_per_lane, batch_per_table,
                                                        block_threads, host_blob);
}

void cuembed_quantized_mixed_group_launch_shape_4bit(const int* widths_host, int num_tables, int out_type, int index_type,
                                                     int batch_per_table, int num_hots, int is_weighted,
                                                     size_t pointer_bits, int* out) {
  namespace d = cuembed::detail;
  CUEMBED_ASSERT(out_type == CUEMBED_F32 || out_type == CUEMBED_F16);
  CUEMBED_ASSERT(index_type == CUEMBED_I32 || index_type == CUEMBED_I64);
  CUEMBED_ASSERT(num_hots >= 0 && out != nullptr);
  const int codes =
      d::Quantized4BitMixedGroupCodesPerLaneOfBits(static_cast<uintptr_t>(pointer_bits), widths_host, num_tables);
  const d::MixedGroupPlan plan =
      d::PlanMixedGroupLanes(widths_host, num_tables, codes, batch_per_table, d::kMixedGroupBlockThreads, nullptr);
  const size_t stage_bytes = d::MixedGroupStageBytes(plan, num_hots == 0, num_hots, index_type == CUEMBED_I32 ? 4 : 8,
                                                     is_weighted ? (out_type == CUEMBED_F32 ? 4 : 2) : 0);
  out[0] = codes;
  out[1] = d::kMixedGroupBlockThreads;
  out[2] = plan.grid;
  out[3] = plan.out_width;
  out[4] = static_cast<int>(stage_bytes);
  out[5] = stage_bytes > 0 ? 1 : 0;
  out[6] = plan.max_slots;
}

}  // extern "C"
