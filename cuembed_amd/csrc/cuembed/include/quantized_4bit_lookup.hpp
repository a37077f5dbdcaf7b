// MI355X (gfx950 / CDNA4) lookup on fused 4-bit row-wise quantized tables -- header-only host API (an extension: the
// reference has no quantized tables).  The sibling of quantized_lookup.hpp (8-bit rows).
//
//   Quantized4BitRowBytes(width)     bytes of one fused row: width / 2 code bytes + fp16 scale + fp16 bias
//   QuantizeRows4Bit                 fp32 / fp16 / bf16 [rows, width] -> fused rows (the bytes torch's
//                                    quantized::embedding_bag_4bit_prepack writes on the CPU)
//   DequantizeRows4Bit               fused rows, all or those a list of ids names -> fp32 / fp16 [n, width]
//   EmbeddingForwardQuantized4Bit    EmbeddingForward on a fused table: sum / mean / concat, fixed hotness or CSR,
//                                    optional per-lookup weights (in the output's type), fp32 or fp16 output
//
// Inference only.  The library's conventions hold: asynchronous on `stream` (last argument), no allocation, no state,
// device pointers owned by the caller, CUEMBED_ASSERT (print and abort) on misuse.
#ifndef CUEMBED_INCLUDE_QUANTIZED_4BIT_LOOKUP_HPP_
#define CUEMBED_INCLUDE_QUANTIZED_4BIT_LOOKUP_HPP_

#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "cuembed/include/cuembed_assert.hpp"
#include "cuembed/include/device_shape.hpp"
#include "cuembed/include/embedding_lookup.hpp"
#include "cuembed/include/quantized_4bit_rows_kernels.hpp"
#include "cuembed/include/quantized_lookup.hpp"   // QuantizedForwardLaunch, PlanQuantizedForward

namespace cuembed {

//! Bytes of one fused 4-bit row of `width` values.
inline int64_t Quantized4BitRowBytes(const int width) {
  return static_cast<int64_t>(width) / 2 + detail::kQuantized4BitTrailerBytes;
}

namespace detail {

//! The format as served here: whole dwords of codes (a row pitch that is a multiple of 4 bytes) at a 4-byte aligned base.
inline void CheckQuantized4BitTable(const int width, const void* table) {
  CUEMBED_ASSERT(width > 0 && width % kQuantized4BitPack == 0);   // "width is a multiple of 8"
  CUEMBED_ASSERT(reinterpret_cast<uintptr_t>(table) % 4 == 0);
}

//! Codes per lane of the pooled forward: 32 (one 16-byte load; a 256-value row is 8 lanes, a wavefront pools EIGHT
//! samples) when the row divides into 32s and fits a 256-thread workgroup, 16 (W % 16 == 0, one 8-byte load) or 8 (one
//! dword).  Every load needs 4-byte alignment only, which the format gives: the choice depends on the width alone.
inline int Quantized4BitForwardCodesPerLane(const int width) {
  if (width % 32 == 0 && width / 32 <= kQuantized4BitWideLaneThreads) return 32;
  return width % 16 == 0 ? 16 : 8;
}

template <typename OutT, typename IndexT, typename OffsetT, int N>
inline void LaunchGatherReduceQuantized4Bit(const uint8_t* table, const int width, const IndexT* indices,
                                            const OffsetT* offsets, const OutT* weights, const int batch,
                                            const int num_hots, const bool is_mean, OutT* out,
                                            const QuantizedForwardLaunch& f, hipStream_t stream,
                                            const ForwardOptions& options) {
  const bool weighted = weights != nullptr;
  const bool stream_rows = options.row_loads == RowLoadPolicy::kStreaming;
  const dim3 block(f.lanes_per_row, f.rows_per_block, 1);
  const dim3 grid(f.grid, 1, 1);
  WithIndexSource(f.staged, f.lanes_per_row, weighted, [&](auto w, auto source) {
    GatherReduceQuantized4BitKernel<OutT, IndexT, OffsetT, N, decltype(w)::value, decltype(source)::value>
        <<<grid, block, f.stage_bytes, stream>>>(table, width, batch, indices, offsets, num_hots, weights, is_mean, out,
                                                 stream_rows, offsets != nullptr ? options.sample_order : nullptr,
                                                 options.row_loads_device);
  });
}

}  // namespace detail

/**
 * @brief Launch description of one 4-bit sum / mean forward: PlanQuantizedForward's heuristics (256-thread workgroups,
 * small grids cut into smaller workgroups, CSR one wavefront per workgroup, fixed-hotness indices (+ weights) staged in
 * LDS) on lanes of 32 / 16 / 8 codes.  Rows of more than 1,024 such lanes abort.
 */
inline detail::QuantizedForwardLaunch PlanQuantized4BitForward(const int width, const int batch, const int num_hots,
                                                               const bool is_csr, const bool weighted,
                                                               const size_t index_bytes, const size_t weight_bytes,
                                                               const detail::DeviceShape& dev) {
  CUEMBED_ASSERT(width > 0 && width % detail::kQuantized4BitPack == 0);
  return detail::PlanQuantizedForward(width, detail::Quantized4BitForwardCodesPerLane(width), batch, num_hots, is_csr,
                                      weighted, index_bytes, weight_bytes, dev);
}

/**
 * @brief Quantizes `rows` rows of `width` values to fused 4-bit rows: out[r] = width / 2 bytes of codes (element 2i in
 * the low nibble of byte i), fp16 scale, fp16 bias, with bias = half(min), scale = half((max - bias) / 15) (1 for a
 * constant row), code = clamp(rint((x - bias) * (1 / scale)), 0, 15), every step one fp32 operation (16-bit input is
 * widened first) -- the bytes torch's CPU prepack writes.
 *
 * @tparam InputT float, __half or __hip_bfloat16
 * @param in     [rows x width], 16-byte aligned
 * @param width  values per row, a multiple of 8
 * @param out    [rows x (width / 2 + 4)] bytes, 4-byte aligned
 */
template <typename InputT>
void QuantizeRows4Bit(const InputT* in, const int width, const int64_t rows, uint8_t* out, const hipStream_t stream = 0) {
  using ElemT = detail::DeviceElemT<InputT>;
  static_assert(std::is_same<InputT, float>::value || std::is_same<InputT, __half>::value ||
                    std::is_same<InputT, __hip_bfloat16>::value,
                "QuantizeRows4Bit: input must be float, __half or __hip_bfloat16");
  detail::CheckQuantized4BitTable(width, out);
  CUEMBED_ASSERT(reinterpret_cast<uintptr_t>(in) % 16 == 0);
  CUEMBED_ASSERT(rows >= 0);
  if (rows == 0) return;
  const int packs = width / detail::kQuantized4BitPack;
  int group = 1;
  while (group < packs && group < 64) group *= 2;
  const int rows_per_block = detail::kQuantizeThreads / group;
  const int64_t blocks = (rows + rows_per_block - 1) / rows_per_block;
  CUEMBED_ASSERT(blocks <= 0x7fffffff);
  const dim3 block(group, rows_per_block, 1);
  const dim3 grid(static_cast<unsigned>(blocks), 1, 1);
  detail::QuantizeRows4BitKernel<ElemT><<<grid, block, 0, stream>>>(reinterpret_cast<const ElemT*>(in), width, rows, out);
}

/**
 * @brief out[i, :] = value of row ids[i] (ids == nullptr: row i) of a fused 4-bit table: float(code) * scale + bias in
 * two rounded fp32 operations (scale and bias widened exactly from fp16), then one rounding to OutputT.
 *
 * @tparam OutputT float or __half
 * @param table  fused rows, [? x (width / 2 + 4)] bytes, 4-byte aligned
 * @param width  values per row, a multiple of 8, at most 8,192 (1,024 lanes of 8 codes)
 * @param ids    n row ids or nullptr
 * @param out    [n x width], 16-byte aligned
 */
template <typename OutputT, typename IndexT>
void DequantizeRows4Bit(const uint8_t* table, const int width, const IndexT* ids, const int64_t n, OutputT* out,
                        const hipStream_t stream = 0) {
  using OutT = detail::DeviceElemT<OutputT>;
  static_assert(std::is_same<OutputT, float>::value || std::is_same<OutputT, __half>::value,
                "DequantizeRows4Bit: output must be float or __half");
  detail::CheckQuantized4BitTable(width, table);
  CUEMBED_ASSERT(reinterpret_cast<uintptr_t>(out) % 16 == 0);
  CUEMBED_ASSERT(n >= 0);
  if (n == 0) return;
  const int lanes = width / detail::kQuantized4BitPack;
  CUEMBED_ASSERT(lanes <= detail::kMaxBlockThreads);
  const int rows_per_block = lanes >= detail::kDefaultBlockThreads ? 1 : detail::kDefaultBlockThreads / lanes;
  const int64_t blocks = (n + rows_per_block - 1) / rows_per_block;
  CUEMBED_ASSERT(blocks <= 0x7fffffff);
  const dim3 block(lanes, rows_per_block, 1);
  const dim3 grid(static_cast<unsigned>(blocks), 1, 1);
  detail::DequantizeRows4BitKernel<OutT, IndexT><<<grid, block, 0, stream>>>(table, width, ids, n,
                                                                             reinterpret_cast<OutT*>(out));
}

/**
 * @brief EmbeddingForward on a fused 4-bit table.  Same index layouts and combine modes as EmbeddingForward
 * (embedding_lookup.hpp); `weights` are in the output's type; accumulation is fp32 in lookup order; empty bags give
 * zeros; mean scales by the reciprocal of the weight sum (zeros when that is 0); concat (fixed hotness, unweighted) is
 * DequantizeRows4Bit on the batch's indices.  Of `options`, row_loads, row_loads_device and sample_order are honoured
 * (scheduling hints: no bit of the result depends on them); reduction_order is not (there is one order).
 *
 * @tparam OutputT float or __half
 * @param table        fused rows, [num_categories x (embed_width / 2 + 4)] bytes, 4-byte aligned
 * @param embed_width  values per row, a multiple of 8
 * @param ret          [batch x width] (sum / mean) or [batch x num_hots x width] (concat), 16-byte aligned
 */
template <typename OutputT, typename IndexT, typename OffsetT>
void EmbeddingForwardQuantized4Bit(const uint8_t* table,
                                   const int embed_width,
                                   const IndexT* indices,
                                   const OffsetT* offsets,
                                   const OutputT* weights,
                                   const int batch_size,
                                   const int num_hots,
                                   const CombineMode mode,
                                   OutputT* ret,
                                   const hipStream_t stream,
                                   const ForwardOptions& options) {
  using OutT = detail::DeviceElemT<OutputT>;
  static_assert(std::is_same<OutputT, float>::value || std::is_same<OutputT, __half>::value,
                "EmbeddingForwardQuantized4Bit: output must be float or __half");
  CUEMBED_ASSERT(weights == nullptr || mode != CombineMode::kConcat);
  CUEMBED_ASSERT((offsets != nullptr && num_hots == 0) || (offsets == nullptr && num_hots > 0));
  CUEMBED_ASSERT(offsets == nullptr || mode != CombineMode::kConcat);
  CUEMBED_ASSERT(options.sample_order == nullptr || offsets != nullptr);
  if (batch_size <= 0) return;
  if (mode == CombineMode::kConcat) {
    DequantizeRows4Bit<OutputT, IndexT>(table, embed_width, indices, static_cast<int64_t>(batch_size) * num_hots, ret,
                                        stream);
    return;
  }
  detail::CheckQuantized4BitTable(embed_width, table);
  CUEMBED_ASSERT(reinterpret_cast<uintptr_t>(ret) % 16 == 0);
  const detail::QuantizedForwardLaunch f =
      PlanQuantized4BitForward(embed_width, batch_size, num_hots, offsets != nullptr, weights != nullptr, sizeof(IndexT),
                               sizeof(OutT), detail::CurrentDeviceShape());
  const OutT* w = reinterpret_cast<const OutT*>(weights);
  OutT* out = reinterpret_cast<OutT*>(ret);
  const bool is_mean = mode == CombineMode::kMean;
  if (f.codes_per_lane == 32)
    detail::LaunchGatherReduceQuantized4Bit<OutT, IndexT, OffsetT, 32>(table, embed_width, indices, offsets, w, batch_size,
                                                                       num_hots, is_mean, out, f, stream, options);
  else if (f.codes_per_lane == 16)
    detail::LaunchGatherReduceQuantized4Bit<OutT, IndexT, OffsetT, 16>(table, embed_width, indices, offsets, w, batch_size,
                                                                       num_hots, is_mean, out, f, stream, options);
  else
    detail::LaunchGatherReduceQuantized4Bit<OutT, IndexT, OffsetT, 8>(table, embed_width, indices, offsets, w, batch_size,
                                                                      num_hots, is_mean, out, f, stream, options);
}

//! ... with the process-wide default options (DefaultForwardOptions()).
template <typename OutputT, typename IndexT, typename OffsetT>
void EmbeddingForwardQuantized4Bit(const uint8_t* table,
                                   const int embed_width,
                                   const IndexT* indices,
                                   const OffsetT* offsets,
                                   const OutputT* weights,
                                   const int batch_size,
                                   const int num_hots,
                                   const CombineMode mode,
                                   OutputT* ret,
                                   const hipStream_t stream = 0) {
  EmbeddingForwardQuantized4Bit<OutputT, IndexT, OffsetT>(table, embed_width, indices, offsets, weights, batch_size,
                                                          num_hots, mode, ret, stream, DefaultForwardOptions());
}

}  // namespace cuembed

#endif  // CUEMBED_INCLUDE_QUANTIZED_4BIT_LOOKUP_HPP_
