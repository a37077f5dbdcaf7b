// MI355X (gfx950 / CDNA4) lookup on 8-bit row-wise quantized tables -- header-only host API (an extension: the
// reference has no quantized tables).
//
//   QuantizedRowBytes(width)     bytes of one fused row: width codes + fp32 scale + fp32 bias
//   QuantizeRows                 fp32 / fp16 / bf16 [rows, width] -> fused rows (bit-identical to torch's
//                                quantized::embedding_bag_byte_prepack on the CPU)
//   DequantizeRows               fused rows, all or those a list of ids names -> fp32 / fp16 [n, width]
//   EmbeddingForwardQuantized    EmbeddingForward on a fused table: sum / mean / concat, fixed hotness or CSR,
//                                optional per-lookup weights (in the output's type), fp32 or fp16 output
//
// Inference only.  The library's conventions hold: asynchronous on `stream` (last argument), no allocation, no state,
// device pointers owned by the caller, CUEMBED_ASSERT (print and abort) on misuse.
#ifndef CUEMBED_INCLUDE_QUANTIZED_LOOKUP_HPP_
#define CUEMBED_INCLUDE_QUANTIZED_LOOKUP_HPP_

#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "cuembed/include/cuembed_assert.hpp"
#include "cuembed/include/device_shape.hpp"
#include "cuembed/include/embedding_lookup.hpp"
#include "cuembed/include/quantized_rows_kernels.hpp"

namespace cuembed {

//! Bytes of one fused row of `width` values.
inline int64_t QuantizedRowBytes(const int width) { return static_cast<int64_t>(width) + detail::kQuantizedTrailerBytes; }

namespace detail {

//! Codes per lane: 8 (one 8-byte load) when rows and table are 8-byte aligned, else 4.
inline int QuantizedCodesPerLane(const int width, const void* table) {
  CUEMBED_ASSERT(width > 0 && width % 4 == 0);                       // "row size is a multiple of 4 bytes"
  CUEMBED_ASSERT(reinterpret_cast<uintptr_t>(table) % 4 == 0);
  return (width % 8 == 0 && reinterpret_cast<uintptr_t>(table) % 8 == 0) ? 8 : 4;
}
//! ... of the pooled forward: 16 (one 16-byte load at an 8-byte aligned address; a 256-value row is 16 lanes, a
//! wavefront pools FOUR samples) when the row also divides into 16s and fits a 256-thread workgroup.
inline int QuantizedForwardCodesPerLane(const int width, const void* table) {
  const int n = QuantizedCodesPerLane(width, table);
  return (n == 8 && width % 16 == 0 && width / 16 <= kQuantizedWideLaneThreads) ? 16 : n;
}

//! Complete launch description of one quantized sum / mean forward.
struct QuantizedForwardLaunch {
  int codes_per_lane;   //!< N: 16, 8 or 4
  int lanes_per_row;    //!< width / N (<= 1024)
  int rows_per_block;   //!< samples per workgroup
  size_t stage_bytes;   //!< dynamic LDS: staged indices (+ weights)
  bool staged;          //!< fixed-hotness indices staged in LDS
  unsigned grid;
};

//! Launch heuristics; they never change a result (every sample is pooled by its own lanes in lookup order).
//!   * 256-thread workgroups of 256 / lanes_per_row samples;
//!   * a grid that would leave compute units idle (fewer than two workgroups per CU) is cut into smaller workgroups,
//!     down to one wavefront each: batch 1,024 of 256-value rows is 512 single-wave workgroups on a 256-CU device
//!     instead of 128 four-wave ones, and stays at 128 on a 32-CU partition;
//!   * CSR with lanes_per_row | 64: one wavefront per workgroup (a slot is free as soon as ITS bags are pooled:
//!     PlanForward, embedding_lookup.hpp);
//!   * fixed hotness: indices (+ weights) staged in LDS when the workgroup's share fits kMaxStageBytes, halving the
//!     samples per workgroup first.
inline QuantizedForwardLaunch PlanQuantizedForward(const int width, const int codes_per_lane, const int batch,
                                                   const int num_hots, const bool is_csr, const bool weighted,
                                                   const size_t index_bytes, const size_t weight_bytes,
                                                   const DeviceShape& dev) {
  QuantizedForwardLaunch f;
  f.codes_per_lane = codes_per_lane;
  f.lanes_per_row = width / codes_per_lane;
  CUEMBED_ASSERT(f.lanes_per_row <= kMaxBlockThreads);
  const int lanes = f.lanes_per_row;
  const bool lanes_fit_wave = LanesDivideWave(lanes);
  const int wave_rows = lanes_fit_wave ? 64 / lanes : 1;
  int rows = lanes >= kDefaultBlockThreads ? 1 : kDefaultBlockThreads / lanes;
  if (is_csr && lanes_fit_wave) rows = wave_rows;
  const int64_t want = 2 * static_cast<int64_t>(dev.compute_units);
  while (rows > wave_rows && (batch + rows - 1) / rows < want) rows = rows / 2 > wave_rows ? rows / 2 : wave_rows;
  f.stage_bytes = 0;
  f.staged = false;
  if (!is_csr) {
    const size_t per_sample = static_cast<size_t>(num_hots) * (index_bytes + (weighted ? weight_bytes : 0));
    if (const int fewer = StagedSamplesPerBlock(rows, per_sample)) {
      f.staged = true;
      rows = fewer;
      f.stage_bytes = rows * per_sample;
    }
  }
  f.rows_per_block = rows;
  f.grid = static_cast<unsigned>((batch + rows - 1) / rows);
  return f;
}

template <typename OutT, typename IndexT, typename OffsetT, int N>
inline void LaunchGatherReduceQuantized(const uint8_t* table, const int width, const IndexT* indices,
                                        const OffsetT* offsets, const OutT* weights, const int batch, const int num_hots,
                                        const bool is_mean, OutT* out, const QuantizedForwardLaunch& f,
                                        hipStream_t stream, const ForwardOptions& options) {
  const bool weighted = weights != nullptr;
  const bool stream_rows = options.row_loads == RowLoadPolicy::kStreaming;
  const dim3 block(f.lanes_per_row, f.rows_per_block, 1);
  const dim3 grid(f.grid, 1, 1);
  WithIndexSource(f.staged, f.lanes_per_row, weighted, [&](auto w, auto source) {
    GatherReduceQuantizedKernel<OutT, IndexT, OffsetT, N, decltype(w)::value, decltype(source)::value>
        <<<grid, block, f.stage_bytes, stream>>>(table, width, batch, indices, offsets, num_hots, weights, is_mean, out,
                                                 stream_rows, offsets != nullptr ? options.sample_order : nullptr,
                                                 options.row_loads_device);
  });
}

}  // namespace detail

/**
 * @brief Quantizes `rows` rows of `width` values to fused 8-bit rows: out[r] = width codes, fp32 scale, fp32 bias,
 * with scale = (max - min) / 255, bias = min, code = rint((x - min) * (255 / (max - min + 1e-8))), every step one
 * fp32 operation (16-bit input is widened first) -- the bytes torch's CPU prepack writes.
 *
 * @tparam InputT float, __half or __hip_bfloat16
 * @param in     [rows x width], 16-byte aligned
 * @param width  values per row, a multiple of 4
 * @param out    [rows x (width + 8)] bytes, 4-byte aligned
 */
template <typename InputT>
void QuantizeRows(const InputT* in, const int width, const int64_t rows, uint8_t* out, const hipStream_t stream = 0) {
  using ElemT = detail::DeviceElemT<InputT>;
  static_assert(std::is_same<InputT, float>::value || std::is_same<InputT, __half>::value ||
                    std::is_same<InputT, __hip_bfloat16>::value,
                "QuantizeRows: input must be float, __half or __hip_bfloat16");
  const int n = detail::QuantizedCodesPerLane(width, out);
  CUEMBED_ASSERT(reinterpret_cast<uintptr_t>(in) % 16 == 0);
  CUEMBED_ASSERT(rows >= 0);
  if (rows == 0) return;
  const int packs = width / n;
  int group = 1;
  while (group < packs && group < 64) group *= 2;
  const int rows_per_block = detail::kQuantizeThreads / group;
  const int64_t blocks = (rows + rows_per_block - 1) / rows_per_block;
  CUEMBED_ASSERT(blocks <= 0x7fffffff);
  const dim3 block(group, rows_per_block, 1);
  const dim3 grid(static_cast<unsigned>(blocks), 1, 1);
  const ElemT* src = reinterpret_cast<const ElemT*>(in);
  if (n == 8) detail::QuantizeRowsKernel<ElemT, 8><<<grid, block, 0, stream>>>(src, width, rows, out);
  else detail::QuantizeRowsKernel<ElemT, 4><<<grid, block, 0, stream>>>(src, width, rows, out);
}

/**
 * @brief out[i, :] = value of row ids[i] (ids == nullptr: row i) of a fused table: float(code) * scale + bias in two
 * rounded fp32 operations, then one rounding to OutputT.
 *
 * @tparam OutputT float or __half
 * @param table  fused rows, [? x (width + 8)] bytes
 * @param ids    n row ids or nullptr
 * @param out    [n x width], 16-byte aligned
 */
template <typename OutputT, typename IndexT>
void DequantizeRows(const uint8_t* table, const int width, const IndexT* ids, const int64_t n, OutputT* out,
                    const hipStream_t stream = 0) {
  using OutT = detail::DeviceElemT<OutputT>;
  static_assert(std::is_same<OutputT, float>::value || std::is_same<OutputT, __half>::value,
                "DequantizeRows: output must be float or __half");
  const int codes = detail::QuantizedCodesPerLane(width, table);
  CUEMBED_ASSERT(reinterpret_cast<uintptr_t>(out) % 16 == 0);
  CUEMBED_ASSERT(n >= 0);
  if (n == 0) return;
  const int lanes = width / codes;
  CUEMBED_ASSERT(lanes <= detail::kMaxBlockThreads);
  const int rows_per_block = lanes >= detail::kDefaultBlockThreads ? 1 : detail::kDefaultBlockThreads / lanes;
  const int64_t blocks = (n + rows_per_block - 1) / rows_per_block;
  CUEMBED_ASSERT(blocks <= 0x7fffffff);
  const dim3 block(lanes, rows_per_block, 1);
  const dim3 grid(static_cast<unsigned>(blocks), 1, 1);
  OutT* dst = reinterpret_cast<OutT*>(out);
  if (codes == 8) detail::DequantizeRowsKernel<OutT, IndexT, 8><<<grid, block, 0, stream>>>(table, width, ids, n, dst);
  else detail::DequantizeRowsKernel<OutT, IndexT, 4><<<grid, block, 0, stream>>>(table, width, ids, n, dst);
}

/**
 * @brief EmbeddingForward on a fused 8-bit table.  Same index layouts and combine modes as EmbeddingForward
 * (embedding_lookup.hpp); `weights` are in the output's type; accumulation is fp32 in lookup order; empty bags give
 * zeros; mean scales by the reciprocal of the weight sum (zeros when that is 0); concat (fixed hotness, unweighted) is
 * DequantizeRows on the batch's indices.  Of `options`, row_loads, row_loads_device and sample_order are honoured
 * (scheduling hints: no bit of the result depends on them); reduction_order is not (there is one order).
 *
 * @tparam OutputT float or __half
 * @param table        fused rows, [num_categories x (embed_width + 8)] bytes
 * @param embed_width  values per row, a multiple of 4
 * @param ret          [batch x width] (sum / mean) or [batch x num_hots x width] (concat), 16-byte aligned
 */
template <typename OutputT, typename IndexT, typename OffsetT>
void EmbeddingForwardQuantized(const uint8_t* table,
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
                "EmbeddingForwardQuantized: output must be float or __half");
  CUEMBED_ASSERT(weights == nullptr || mode != CombineMode::kConcat);
  CUEMBED_ASSERT((offsets != nullptr && num_hots == 0) || (offsets == nullptr && num_hots > 0));
  CUEMBED_ASSERT(offsets == nullptr || mode != CombineMode::kConcat);
  CUEMBED_ASSERT(options.sample_order == nullptr || offsets != nullptr);
  if (batch_size <= 0) return;
  if (mode == CombineMode::kConcat) {
    DequantizeRows<OutputT, IndexT>(table, embed_width, indices, static_cast<int64_t>(batch_size) * num_hots, ret, stream);
    return;
  }
  const int codes = detail::QuantizedForwardCodesPerLane(embed_width, table);
  CUEMBED_ASSERT(reinterpret_cast<uintptr_t>(ret) % 16 == 0);
  const detail::QuantizedForwardLaunch f = detail::PlanQuantizedForward(
      embed_width, codes, batch_size, num_hots, offsets != nullptr, weights != nullptr, sizeof(IndexT), sizeof(OutT),
      detail::CurrentDeviceShape());
  const OutT* w = reinterpret_cast<const OutT*>(weights);
  OutT* out = reinterpret_cast<OutT*>(ret);
  const bool is_mean = mode == CombineMode::kMean;
  if (codes == 16)
    detail::LaunchGatherReduceQuantized<OutT, IndexT, OffsetT, 16>(table, embed_width, indices, offsets, w, batch_size,
                                                                   num_hots, is_mean, out, f, stream, options);
  else if (codes == 8)
    detail::LaunchGatherReduceQuantized<OutT, IndexT, OffsetT, 8>(table, embed_width, indices, offsets, w, batch_size,
                                                                  num_hots, is_mean, out, f, stream, options);
  else
    detail::LaunchGatherReduceQuantized<OutT, IndexT, OffsetT, 4>(table, embed_width, indices, offsets, w, batch_size,
                                                                  num_hots, is_mean, out, f, stream, options);
}

//! ... with the process-wide default options (DefaultForwardOptions()).
template <typename OutputT, typename IndexT, typename OffsetT>
void EmbeddingForwardQuantized(const uint8_t* table,
                               const int embed_width,
                               const IndexT* indices,
                               const OffsetT* offsets,
                               const OutputT* weights,
                               const int batch_size,
                               const int num_hots,
                               const CombineMode mode,
                               OutputT* ret,
                               const hipStream_t stream = 0) {
  EmbeddingForwardQuantized<OutputT, IndexT, OffsetT>(table, embed_width, indices, offsets, weights, batch_size,
                                                      num_hots, mode, ret, stream, DefaultForwardOptions());
}

}  // namespace cuembed

#endif  // CUEMBED_INCLUDE_QUANTIZED_LOOKUP_HPP_
