// C ABI: the forward on a GROUP of tables in one launch = explicit instantiations of cuembed::EmbeddingForwardGrouped
// and cuembed::EmbeddingForwardQuantizedGrouped (an extension: the reference's entry points take one table).  The
// instantiation set is that of c_api_forward.hip / c_api_quantized.hip without fp16_math.
#include "c_api_common.hpp"
#include "cuembed/include/grouped_lookup.hpp"

using cuembed::CombineMode;
using cuembed_c_api::Stream;

namespace {
cuembed::ForwardOptions Options(int row_load_policy, const int32_t* sample_order) {
  cuembed::ForwardOptions options;   // (not the process-wide defaults: the group has one order, and no device decision)
  options.row_loads = cuembed::GetForwardRowLoadPolicy();
  options.sample_order = sample_order;
  CUEMBED_ASSERT(row_load_policy <= 1);
  if (row_load_policy >= 0) options.row_loads = static_cast<cuembed::RowLoadPolicy>(row_load_policy);
  return options;
}

CombineMode Mode(int mode) {
  CUEMBED_ASSERT(mode == CUEMBED_SUM || mode == CUEMBED_MEAN);
  return mode == CUEMBED_SUM ? CombineMode::kSum : CombineMode::kMean;
}

template <typename ElemT, typename IndexT, typename OffsetT>
void Forward(const void* const* tables_host, const void* const* tables_device, int num_tables, int embed_width,
             const void* indices, const void* offsets, const void* weights, int batch_per_table, int num_hots,
             CombineMode mode, void* ret, const cuembed::ForwardOptions& options, cuembed_stream_t stream) {
  cuembed::EmbeddingForwardGrouped<ElemT, ElemT, IndexT, OffsetT>(
      reinterpret_cast<const ElemT* const*>(tables_host), reinterpret_cast<const ElemT* const*>(tables_device), num_tables,
      embed_width, static_cast<const IndexT*>(indices), static_cast<const OffsetT*>(offsets),
      static_cast<const ElemT*>(weights), batch_per_table, num_hots, mode, static_cast<ElemT*>(ret), Stream(stream),
      options);
}

template <typename OutT, typename IndexT, typename OffsetT>
void ForwardQuantized(const void* const* tables_host, const void* const* tables_device, int num_tables, int embed_width,
                      const void* indices, const void* offsets, const void* weights, int batch_per_table, int num_hots,
                      CombineMode mode, void* ret, const cuembed::ForwardOptions& options, cuembed_stream_t stream) {
  cuembed::EmbeddingForwardQuantizedGrouped<OutT, IndexT, OffsetT>(
      reinterpret_cast<const uint8_t* const*>(tables_host), reinterpret_cast<const uint8_t* const*>(tables_device),
      num_tables, embed_width, static_cast<const IndexT*>(indices), static_cast<const OffsetT*>(offsets),
      static_cast<const OutT*>(weights), batch_per_table, num_hots, mode, static_cast<OutT*>(ret), Stream(stream), options);
}
}  // namespace

extern "C" {

void cuembed_embedding_forward_grouped(const void* const* tables_host, const void* const* tables_device, int num_tables,
                                       int elem_type, int embed_width, const void* indices, int index_type,
                                       const void* offsets, int offset_type, const void* weights, int batch_per_table,
                                       int num_hots, int mode, void* ret, int row_load_policy,
                                       const int32_t* sample_order, cuembed_stream_t stream) {
  const cuembed::ForwardOptions options = Options(row_load_policy, sample_order);
  const CombineMode m = Mode(mode);
  CUEMBED_ASSERT(index_type == CUEMBED_I32 || index_type == CUEMBED_I64);
  CUEMBED_ASSERT(offsets == nullptr || offset_type == CUEMBED_I32 || offset_type == CUEMBED_I64);
#define FWD(E, I, O)                                                                                                 \
  Forward<E, I, O>(tables_host, tables_device, num_tables, embed_width, indices, offsets, weights, batch_per_table, \
                   num_hots, m, ret, options, stream)
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

void cuembed_embedding_forward_quantized_grouped(const void* const* tables_host, const void* const* tables_device,
                                                 int num_tables, int embed_width, const void* indices, int index_type,
                                                 const void* offsets, int offset_type, const void* weights,
                                                 int batch_per_table, int num_hots, int mode, void* ret, int out_type,
                                                 int row_load_policy, const int32_t* sample_order,
                                                 cuembed_stream_t stream) {
  const cuembed::ForwardOptions options = Options(row_load_policy, sample_order);
  const CombineMode m = Mode(mode);
  CUEMBED_ASSERT(out_type == CUEMBED_F32 || out_type == CUEMBED_F16);
  CUEMBED_ASSERT(index_type == CUEMBED_I32 || index_type == CUEMBED_I64);
  CUEMBED_ASSERT(offsets == nullptr || offset_type == CUEMBED_I32 || offset_type == CUEMBED_I64);
#define FWD(E, I, O)                                                                                               \
  ForwardQuantized<E, I, O>(tables_host, tables_device, num_tables, embed_width, indices, offsets, weights,       \
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

void cuembed_grouped_forward_launch_shape(int quantized, int elem_type, int index_type, int embed_width, int num_tables,
                                          int batch_per_table, int num_hots, int is_csr, int is_weighted,
                                          int compute_units, int xcds, int* out) {
  namespace d = cuembed::detail;
  const int batch = d::GroupedBatch(num_tables, batch_per_table);
  int lanes = 0;
  bool staged = false;
  if (quantized) {
    d::DeviceShape dev = compute_units > 0 ? d::Mi355xShape() : d::CurrentDeviceShape();
    if (compute_units > 0) {
      dev.compute_units = compute_units;
      dev.xcds = xcds > 0 ? xcds : 1;
    }
    const int codes = d::QuantizedForwardCodesPerLane(embed_width, nullptr);   // (aligned buffers)
    const d::QuantizedForwardLaunch f =
        d::PlanQuantizedForward(embed_width, codes, batch, num_hots, is_csr != 0, is_weighted != 0,
                                index_type == CUEMBED_I32 ? 4 : 8, elem_type == CUEMBED_F32 ? 4 : 2, dev);
    out[0] = f.codes_per_lane;
    out[1] = lanes = f.lanes_per_row;
    out[2] = f.rows_per_block;
    out[3] = static_cast<int>(f.grid);
    out[4] = static_cast<int>(f.stage_bytes);
    staged = f.staged;
  } else {
    d::ForwardLaunch f;
    if (elem_type == CUEMBED_F32) {
      f = index_type == CUEMBED_I32
              ? d::PlanForward<float, int32_t>(embed_width, nullptr, nullptr, batch, num_hots, is_csr, is_weighted, false)
              : d::PlanForward<float, int64_t>(embed_width, nullptr, nullptr, batch, num_hots, is_csr, is_weighted, false);
    } else {  // 2-byte elements (fp16 and bf16 plan identically)
      f = index_type == CUEMBED_I32
              ? d::PlanForward<_Float16, int32_t>(embed_width, nullptr, nullptr, batch, num_hots, is_csr, is_weighted, false)
              : d::PlanForward<_Float16, int64_t>(embed_width, nullptr, nullptr, batch, num_hots, is_csr, is_weighted, false);
    }
    out[0] = f.split.elems_per_lane;
    out[1] = lanes = f.split.lanes_per_row;
    out[2] = f.split.rows_per_block;
    out[3] = static_cast<int>(f.grid);
    out[4] = static_cast<int>(f.stage_bytes);
    staged = f.staged;
  }
  out[5] = staged ? 1 : 0;
  // the index source WithIndexSource dispatches on: 0 = staged in LDS, 1 = cross-lane reads, 2 = global loads
  out[6] = staged ? 0 : (d::LanesDivideWave(lanes) ? 1 : 2);
}

}  // extern "C"
