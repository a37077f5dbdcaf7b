// C ABI: 8-bit row-wise quantized tables = explicit instantiations of cuembed::QuantizeRows, DequantizeRows and
// EmbeddingForwardQuantized (an extension: the reference has fp32 / fp16 tables only).
#include "c_api_common.hpp"
#include "cuembed/include/quantized_lookup.hpp"

using cuembed::CombineMode;
using cuembed_c_api::Stream;

namespace {
template <typename OutT, typename IndexT, typename OffsetT>
void Forward(const void* table, int embed_width, const void* indices, const void* offsets, const void* weights,
             int batch_size, int num_hots, CombineMode mode, void* ret, const cuembed::ForwardOptions& options,
             cuembed_stream_t stream) {
  cuembed::EmbeddingForwardQuantized<OutT, IndexT, OffsetT>(
      static_cast<const uint8_t*>(table), embed_width, static_cast<const IndexT*>(indices),
      static_cast<const OffsetT*>(offsets), static_cast<const OutT*>(weights), batch_size, num_hots, mode,
      static_cast<OutT*>(ret), Stream(stream), options);
}

template <typename OutT, typename IndexT>
void Dequantize(const void* table, int embed_width, const void* ids, int64_t n, void* out, cuembed_stream_t stream) {
  cuembed::DequantizeRows<OutT, IndexT>(static_cast<const uint8_t*>(table), embed_width,
                                        static_cast<const IndexT*>(ids), n, static_cast<OutT*>(out), Stream(stream));
}
}  // namespace

extern "C" {

int64_t cuembed_quantized_row_bytes(int embed_width) { return cuembed::QuantizedRowBytes(embed_width); }

void cuembed_quantize_rows(const void* in, int elem_type, int embed_width, int64_t rows, void* out,
                           cuembed_stream_t stream) {
  uint8_t* dst = static_cast<uint8_t*>(out);
  switch (elem_type) {
    case CUEMBED_F32:
      cuembed::QuantizeRows<float>(static_cast<const float*>(in), embed_width, rows, dst, Stream(stream));
      break;
    case CUEMBED_F16:
      cuembed::QuantizeRows<__half>(static_cast<const __half*>(in), embed_width, rows, dst, Stream(stream));
      break;
    case CUEMBED_BF16:
      cuembed::QuantizeRows<__hip_bfloat16>(static_cast<const __hip_bfloat16*>(in), embed_width, rows, dst,
                                            Stream(stream));
      break;
    default: CUEMBED_C_API_BAD_TYPE();
  }
}

void cuembed_dequantize_rows(const void* qtable, int embed_width, const void* ids, int index_type, int64_t n, void* out,
                             int out_type, cuembed_stream_t stream) {
  CUEMBED_ASSERT(out_type == CUEMBED_F32 || out_type == CUEMBED_F16);
  CUEMBED_ASSERT(index_type == CUEMBED_I32 || index_type == CUEMBED_I64);
  switch ((out_type << 1) | index_type) {
    case 0: Dequantize<float, int32_t>(qtable, embed_width, ids, n, out, stream); break;
    case 1: Dequantize<float, int64_t>(qtable, embed_width, ids, n, out, stream); break;
    case 2: Dequantize<__half, int32_t>(qtable, embed_width, ids, n, out, stream); break;
    case 3: Dequantize<__half, int64_t>(qtable, embed_width, ids, n, out, stream); break;
    default: CUEMBED_C_API_BAD_TYPE();
  }
}

void cuembed_embedding_forward_quantized(const void* qtable, int embed_width, const void* indices, int index_type,
                                         const void* offsets, int offset_type, const void* weights, int batch_size,
                                         int num_hots, int mode, void* ret, int out_type, int row_load_policy,
                                         const int32_t* sample_order, const uint32_t* row_loads_device,
                                         cuembed_stream_t stream) {
  cuembed::ForwardOptions options = cuembed::DefaultForwardOptions();
  options.sample_order = sample_order;
  options.row_loads_device = row_loads_device;
  CUEMBED_ASSERT(row_load_policy <= 1);
  if (row_load_policy >= 0) options.row_loads = static_cast<cuembed::RowLoadPolicy>(row_load_policy);
  CUEMBED_ASSERT(mode == CUEMBED_SUM || mode == CUEMBED_MEAN || mode == CUEMBED_CONCAT);
  const CombineMode m = mode == CUEMBED_SUM    ? CombineMode::kSum
                        : mode == CUEMBED_MEAN ? CombineMode::kMean
                                               : CombineMode::kConcat;
  CUEMBED_ASSERT(out_type == CUEMBED_F32 || out_type == CUEMBED_F16);
  CUEMBED_ASSERT(index_type == CUEMBED_I32 || index_type == CUEMBED_I64);
  CUEMBED_ASSERT(offsets == nullptr || offset_type == CUEMBED_I32 || offset_type == CUEMBED_I64);
#define FWD(E, I, O) \
  Forward<E, I, O>(qtable, embed_width, indices, offsets, weights, batch_size, num_hots, m, ret, options, stream)
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

void cuembed_quantized_forward_launch_shape(int index_type, int out_type, int embed_width, int batch_size, int num_hots,
                                            int is_csr, int is_weighted, int compute_units, int xcds, int* out) {
  cuembed::detail::DeviceShape dev =
      compute_units > 0 ? cuembed::detail::Mi355xShape() : cuembed::detail::CurrentDeviceShape();
  if (compute_units > 0) {
    dev.compute_units = compute_units;
    dev.xcds = xcds > 0 ? xcds : 1;
  }
  const int codes = cuembed::detail::QuantizedForwardCodesPerLane(embed_width, nullptr);   // (aligned buffers)
  const cuembed::detail::QuantizedForwardLaunch f = cuembed::detail::PlanQuantizedForward(
      embed_width, codes, batch_size, num_hots, is_csr != 0, is_weighted != 0, index_type == CUEMBED_I32 ? 4 : 8,
      out_type == CUEMBED_F32 ? 4 : 2, dev);
  out[0] = f.codes_per_lane;
  out[1] = f.lanes_per_row;
  out[2] = f.rows_per_block;
  out[3] = static_cast<int>(f.grid);
  out[4] = static_cast<int>(f.stage_bytes);
  out[5] = f.staged ? 1 : 0;
}

}  // extern "C"
