// MI355X (gfx950 / CDNA4) kernels for fused 4-bit row-wise quantized tables (an extension: the reference has fp32 /
// fp16 tables only).  Siblings of the 8-bit kernels (quantized_rows_kernels.hpp), which stay as they are.
//
// The format is PyTorch's / FBGEMM's "fused 4-bit row-wise" layout (quantized::embedding_bag_4bit_prepack): a row of W
// values (W % 8 == 0 here) is W / 2 + 4 bytes -- byte i holds element 2i in its low nibble and element 2i + 1 in its
// high nibble, then the row's fp16 scale and fp16 bias -- and a value is code * scale + bias.  A looked-up row of 256
// values is 132 bytes (about two 128-byte cache lines) instead of 264 (8-bit) or 512 (fp16).
//
//   QuantizeRows4BitKernel            fp32 / fp16 / bf16 [rows, W] -> fused rows, the bytes torch's CPU prepack writes
//   DequantizeRows4BitKernel          fused rows (all, or the rows a list of ids names) -> fp32 / fp16 [n, W]
//   GatherReduceQuantized4BitKernel   sum / mean of looked-up rows, fixed hotness or CSR, optionally weighted
//
// The gather is GatherReduceKernel's sample walk (WalkSample, gather_reduce_kernels.hpp) on 16-byte loads of CODES: one
// lane owns 32 codes (one global_load_dwordx4 at a 4-byte aligned address), a 256-value row is 8 lanes, a wavefront
// pools EIGHT samples, and four lookups per sample are in flight before the first is consumed (16 or 8 codes per lane,
// one dwordx2 / dword, where the row does not divide into 32s: eight and four in flight, Quantized4BitUnroll).
//   * scale and bias reach the lanes by ONE extra 4-byte load per lookup at an address all lanes of the row share; its
//     address is the code address plus a per-lane constant, so a lookup costs one id x row_bytes multiply;
//   * nibbles are not extracted one by one: per dword d, lo = d & 0x0F0F0F0F holds the four EVEN elements as bytes and
//     hi = (d >> 4) & 0x0F0F0F0F the four ODD ones; v_cvt_f32_ubyte0..3 converts each byte.  Two integer operations
//     per dword, one conversion and one fma per element.  The accumulators are therefore held in even / odd order and
//     the epilogue interleaves them back when it forms the output packs;
//   * acc[e] = fma(code[e], w * scale, acc[e]) pools the codes, bias_sum = fma(w, bias, bias_sum) pools the biases of
//     the bag, and the epilogue adds bias_sum once -- the 8-bit kernel's arithmetic with scale and bias widened
//     (exactly) from fp16.  fp32 throughout, strictly in lookup order: a bag's result depends on nothing but the bag;
//   * row-load policy and sample order are scheduling hints: no bit changes.
#ifndef CUEMBED_INCLUDE_QUANTIZED_4BIT_ROWS_KERNELS_HPP_
#define CUEMBED_INCLUDE_QUANTIZED_4BIT_ROWS_KERNELS_HPP_

#include <cstdint>

#include "cuembed/include/embedding_types.hpp"
#include "cuembed/include/gather_reduce_kernels.hpp"
#include "cuembed/include/quantized_rows_kernels.hpp"   // LoadWide, StoreWideStreaming, ScaleBias, kQuantize...

namespace cuembed {
namespace detail {

constexpr int kQuantized4BitTrailerBytes = 4;   //!< fp16 scale + fp16 bias behind the codes of a row
constexpr int kQuantized4BitPack = 8;           //!< codes of one dword: what the quantizer and dequantizer lanes move
constexpr uint32_t kNibbleMask = 0x0F0F0F0Fu;

//! Bytes of the codes of `width` values.
__host__ __device__ __forceinline__ int CodeBytes4Bit(const int width) { return width / 2; }

//! Byte k of `x` as a float (v_cvt_f32_ubyte<k>).
template <int k>
__device__ __forceinline__ float ByteToFloat(const uint32_t x) {
  return static_cast<float>((x >> (8 * k)) & 0xFFu);
}

//! The trailer dword of a row: fp16 scale in the low half, fp16 bias in the high half, widened exactly.
__device__ __forceinline__ ScaleBias DecodeTrailer4Bit(const uint32_t t) {
  typedef _Float16 half2_t __attribute__((ext_vector_type(2)));
  const half2_t h = __builtin_bit_cast(half2_t, t);
  ScaleBias sb;
  sb.scale = static_cast<float>(h.x);
  sb.bias = static_cast<float>(h.y);
  return sb;
}

template <bool kStream>
__device__ __forceinline__ uint32_t LoadDword(const uint8_t* p) {
  const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
  return kStream ? __builtin_nontemporal_load(q) : *q;
}

//! N codes of one lane: N / 8 dwords in ONE load at a 4-byte aligned address (rows are W / 2 + 4 bytes: nothing wider
//! is guaranteed, and the hardware needs dword alignment only).
template <int N>
struct NibblePack {
  uint32_t d[N / 8];
};
template <int N, bool kStream>
__device__ __forceinline__ NibblePack<N> LoadNibbles(const uint8_t* p) {
  typedef unsigned __attribute__((ext_vector_type(N / 8), aligned(4))) raw_t;
  raw_t raw;
  if constexpr (kStream) raw = __builtin_nontemporal_load(reinterpret_cast<const raw_t*>(p));
  else raw = *reinterpret_cast<const raw_t*>(p);
  return *reinterpret_cast<const NibblePack<N>*>(&raw);
}

// ---------------------------------------------------------------------------
// Quantizer.  block = (group, kQuantizeThreads / group); grid = ceil(rows / blockDim.y).
// A group of `group` lanes (a power of two <= 64) owns a row; lane l holds packs l, l + group, ... of 8 values, each
// of which becomes ONE dword of codes.  Rows of up to group x kQuantizeRegChunks packs (2,048 values) are read once
// and kept in registers between the min / max butterfly and the encoding; wider rows are read twice.  Arithmetic,
// every step one IEEE fp32 operation, as torch's CPU prepack:
//     mn = float(half(min));  range = max - mn;  scale = half(range == 0 ? 1 : range / 15);
//     inv = float(scale) == 0 ? 1 : 1 / float(scale);  scale == 0 or inv infinite: scale = inv = 1;
//     code = clamp(rint((x - mn) * inv), 0, 15)
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint32_t EncodePack4Bit(const float (&x)[kQuantized4BitPack], const float mn, const float inv) {
  using A = Arith<float>;
  uint32_t d = 0;
#pragma unroll
  for (int e = 0; e < kQuantized4BitPack; ++e) {
    const float r = __builtin_rintf(A::mul(A::add(x[e], -mn), inv));
    const uint32_t code = static_cast<uint32_t>(__builtin_fminf(__builtin_fmaxf(r, 0.f), 15.f));
    d |= code << (4 * e);
  }
  return d;
}

template <typename InT>
__global__ void __launch_bounds__(kQuantizeThreads)
QuantizeRows4BitKernel(const InT* __restrict__ in, const int width, const int64_t rows, uint8_t* __restrict__ out) {
  using A = Arith<float>;
  constexpr int N = kQuantized4BitPack;
  const int lane = threadIdx.x;
  const int group = blockDim.x;
  const int64_t row = static_cast<int64_t>(blockIdx.x) * blockDim.y + threadIdx.y;
  if (row >= rows) return;     // (the lanes of a group share the row: they leave together)
  const int packs = width / N;
  const InT* src = in + row * static_cast<int64_t>(width);
  uint32_t* dst = reinterpret_cast<uint32_t*>(out + row * static_cast<int64_t>(CodeBytes4Bit(width) + kQuantized4BitTrailerBytes));
  const bool in_registers = packs <= group * kQuantizeRegChunks;
  float x[kQuantizeRegChunks][N];
  float mn = __builtin_inff(), mx = -__builtin_inff();
  if (in_registers) {
#pragma unroll
    for (int c = 0; c < kQuantizeRegChunks; ++c) {
      const int p = c * group + lane;
      if (p < packs) {
        LoadWide<InT, N>(src + static_cast<int64_t>(p) * N, x[c]);
#pragma unroll
        for (int e = 0; e < N; ++e) {
          mn = __builtin_fminf(mn, x[c][e]);
          mx = __builtin_fmaxf(mx, x[c][e]);
        }
      }
    }
  } else {
    for (int p = lane; p < packs; p += group) {
      float y[N];
      LoadWide<InT, N>(src + static_cast<int64_t>(p) * N, y);
#pragma unroll
      for (int e = 0; e < N; ++e) {
        mn = __builtin_fminf(mn, y[e]);
        mx = __builtin_fmaxf(mx, y[e]);
      }
    }
  }
  for (int d = group >> 1; d > 0; d >>= 1) {
    mn = __builtin_fminf(mn, __shfl_xor(mn, d, group));
    mx = __builtin_fmaxf(mx, __shfl_xor(mx, d, group));
  }
  const _Float16 bias16 = static_cast<_Float16>(mn);
  mn = static_cast<float>(bias16);
  const float range = A::add(mx, -mn);
  _Float16 scale16 = static_cast<_Float16>(range == 0.f ? 1.0f : range / 15.0f);
  float inv = static_cast<float>(scale16) == 0.f ? 1.0f : 1.0f / static_cast<float>(scale16);
  if (static_cast<float>(scale16) == 0.f || __builtin_isinf(inv)) {
    scale16 = static_cast<_Float16>(1.0f);
    inv = 1.0f;
  }
  if (in_registers) {
#pragma unroll
    for (int c = 0; c < kQuantizeRegChunks; ++c) {
      const int p = c * group + lane;
      if (p < packs) __builtin_nontemporal_store(EncodePack4Bit(x[c], mn, inv), dst + p);
    }
  } else {
    for (int p = lane; p < packs; p += group) {
      float y[N];
      LoadWide<InT, N>(src + static_cast<int64_t>(p) * N, y);
      __builtin_nontemporal_store(EncodePack4Bit(y, mn, inv), dst + p);
    }
  }
  if (lane == 0) {
    typedef _Float16 half2_t __attribute__((ext_vector_type(2)));
    half2_t trailer;
    trailer.x = scale16;
    trailer.y = bias16;
    dst[packs] = __builtin_bit_cast(uint32_t, trailer);   // (behind the W / 8 code dwords of the row)
  }
}

// ---------------------------------------------------------------------------
// Dequantizer: out[i, :] = float(code) * scale + bias of row ids[i] (ids == nullptr: row i), two rounded fp32
// operations, then one rounding to OutT.  block = (W / 8, rows_per_block); grid = ceil(n / rows_per_block): a lane
// turns one dword of codes into 8 values.  mode = "concat" of the lookup is this kernel on the batch's ids.
// ---------------------------------------------------------------------------
template <typename OutT, typename IndexT>
__global__ void __launch_bounds__(kMaxBlockThreads)
DequantizeRows4BitKernel(const uint8_t* __restrict__ table, const int width, const IndexT* __restrict__ ids,
                         const int64_t n, OutT* __restrict__ out) {
  using A = Arith<float>;
  constexpr int N = kQuantized4BitPack;
  const int lane_x = threadIdx.x;
  const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.y + threadIdx.y;
  if (i >= n) return;
  const int64_t r = ids != nullptr ? WidenIndex(ids[i]) : i;
  const int code_bytes = CodeBytes4Bit(width);
  const uint8_t* row = RowPtr<uint8_t>(table, r, code_bytes + kQuantized4BitTrailerBytes);
  const uint32_t d = LoadDword<false>(row + lane_x * 4);
  const ScaleBias sb = DecodeTrailer4Bit(LoadDword<false>(row + code_bytes));
  float v[N];
#pragma unroll
  for (int e = 0; e < N; ++e)
    v[e] = A::add(A::mul(static_cast<float>((d >> (4 * e)) & 0xFu), sb.scale), sb.bias);
  StoreWideStreaming<OutT, N>(out + i * static_cast<int64_t>(width) + lane_x * N, v);
}

// ---------------------------------------------------------------------------
// Sum / mean on fused rows.
//   block = (lanes_per_row, samples_per_block); grid = ceil(batch / samples_per_block)
//   dynamic LDS (kLdsStaged only) = samples_per_block * num_hots * (sizeof(IndexT) [+ sizeof(OutT) if weighted])
// ---------------------------------------------------------------------------
template <typename OutT, int N, bool kWeighted>
struct Quantized4BitRowPool {
  //! sum_j w_j * scale_j * code_j, per dword q of the lane in even / odd order: acc[q][0][k] is element 8q + 2k (the
  //! low nibble of byte k), acc[q][1][k] element 8q + 2k + 1 (its high nibble).
  float acc[N / 8][2][4];
  float bias_sum;     //!< sum_j w_j * bias_j
  float weight_sum;

  __device__ __forceinline__ Quantized4BitRowPool() : bias_sum(0.f), weight_sum(0.f) {
#pragma unroll
    for (int q = 0; q < N / 8; ++q)
#pragma unroll
      for (int k = 0; k < 4; ++k) acc[q][0][k] = acc[q][1][k] = 0.f;
  }

  __device__ __forceinline__ void Add(const NibblePack<N>& codes, const uint32_t trailer, const OutT w) {
    using A = Arith<float>;
    const ScaleBias sb = DecodeTrailer4Bit(trailer);
    float m = sb.scale;     // what a code is multiplied by
    if constexpr (kWeighted) {
      const float wf = static_cast<float>(w);
      m = A::mul(wf, sb.scale);
      weight_sum += wf;
      bias_sum = __builtin_fmaf(wf, sb.bias, bias_sum);
    } else {
      bias_sum = A::add(bias_sum, sb.bias);
    }
#pragma unroll
    for (int q = 0; q < N / 8; ++q) {
      uint32_t lo = codes.d[q] & kNibbleMask;
      uint32_t hi = (codes.d[q] >> 4) & kNibbleMask;
      // (opaque to the optimizer, which would otherwise fold mask and byte select into one bit-field extract PER
      // ELEMENT in front of v_cvt_f32_ubyte0: three operations an element instead of one and a quarter)
      __asm__("" : "+v"(lo));
      __asm__("" : "+v"(hi));
      acc[q][0][0] = __builtin_fmaf(ByteToFloat<0>(lo), m, acc[q][0][0]);
      acc[q][0][1] = __builtin_fmaf(ByteToFloat<1>(lo), m, acc[q][0][1]);
      acc[q][0][2] = __builtin_fmaf(ByteToFloat<2>(lo), m, acc[q][0][2]);
      acc[q][0][3] = __builtin_fmaf(ByteToFloat<3>(lo), m, acc[q][0][3]);
      acc[q][1][0] = __builtin_fmaf(ByteToFloat<0>(hi), m, acc[q][1][0]);
      acc[q][1][1] = __builtin_fmaf(ByteToFloat<1>(hi), m, acc[q][1][1]);
      acc[q][1][2] = __builtin_fmaf(ByteToFloat<2>(hi), m, acc[q][1][2]);
      acc[q][1][3] = __builtin_fmaf(ByteToFloat<3>(hi), m, acc[q][1][3]);
    }
  }

  //! Pools `count` lookups in order; kUnroll code loads and as many trailer loads are issued back-to-back before the
  //! first is consumed (`sched_barrier` pins "all loads first"), the tail of a bag as one predicated batch.
  //! lane_base = table + this lane's first code byte; the row's trailer is trailer_delta bytes behind the lane's codes
  //! (one 64-bit add on the address the codes are loaded from, instead of a second id x row_bytes multiply).
  template <int kUnroll, bool kStream, typename IndexFn, typename WeightFn>
  __device__ __forceinline__ void Gather(const uint8_t* lane_base, const int64_t trailer_delta, const int row_bytes,
                                         const int count, IndexFn index_at, WeightFn weight_at) {
    int j = 0;
    for (; j + kUnroll <= count; j += kUnroll)
      Batch<kUnroll, kStream>(lane_base, trailer_delta, row_bytes, j, kUnroll, index_at, weight_at);
    if (j < count) Batch<kUnroll - 1, kStream>(lane_base, trailer_delta, row_bytes, j, count - j, index_at, weight_at);
  }

  //! Lookups j .. j + n - 1 (n <= kSlots): all their loads, then their sums in order.  (Its registers are its own: a
  //! full batch and the tail of the bag share none.)
  template <int kSlots, bool kStream, typename IndexFn, typename WeightFn>
  __device__ __forceinline__ void Batch(const uint8_t* lane_base, const int64_t trailer_delta, const int row_bytes,
                                        const int j, const int n, IndexFn index_at, WeightFn weight_at) {
    NibblePack<N> codes[kSlots];
    uint32_t trailer[kSlots];
    OutT w[kSlots];
#pragma unroll
    for (int u = 0; u < kSlots; ++u) {
      if (u < n) {
        if constexpr (kWeighted) w[u] = weight_at(j + u);
        const uint8_t* p = RowPtr<uint8_t>(lane_base, index_at(j + u), row_bytes);
        codes[u] = LoadNibbles<N, kStream>(p);
        trailer[u] = LoadDword<kStream>(p + trailer_delta);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < kSlots; ++u)
      if (u < n) Add(codes[u], trailer[u], w[u]);
  }
};

//! Workgroup size limit of the 32-codes-per-lane gather: 32 sums, 4 x 20 bytes in flight and the unpacking take up to
//! 166 registers, and the 128 a 1,024-thread workgroup leaves a lane would spill.  Rows of more than 256 such lanes
//! (W > 8,192) take 16 codes per lane.
constexpr int kQuantized4BitWideLaneThreads = 256;
//! Lookups in flight per sample, chosen so that no instantiation spills (profiles/quantized_4bit_kernel_resources.txt):
//! four 16-byte loads per lane with 32 codes, eight 8-byte loads with 16, four dwords with 8 (eight dwords in flight
//! spill 12 bytes in two of the 48 instantiations under the 1,024-thread bound).
template <int N>
constexpr int Quantized4BitUnroll() { return N == 16 ? kForwardUnroll : 4; }
template <int N>
constexpr int Quantized4BitThreads() { return N == 32 ? kQuantized4BitWideLaneThreads : kMaxBlockThreads; }

template <typename OutT,     // output and weight element: float or _Float16
          typename IndexT,   // int32_t / int64_t
          typename OffsetT,  // CSR offset type (unused for kLdsStaged)
          int N,             // codes per lane: 32 (W % 32 == 0), 16 (W % 16 == 0) or 8
          bool kWeighted,
          IndexSource kSource>
__global__ void __launch_bounds__(Quantized4BitThreads<N>())
GatherReduceQuantized4BitKernel(const uint8_t* __restrict__ table,
                                const int width,
                                const int batch,
                                const IndexT* __restrict__ indices,
                                const OffsetT* __restrict__ offsets,  // null => fixed hotness
                                const int num_hots,
                                const OutT* __restrict__ weights,
                                const bool is_mean,
                                OutT* __restrict__ out,
                                const bool stream_rows_host,
                                const int32_t* __restrict__ sample_order,         // ForwardOptions::sample_order (CSR only)
                                const uint32_t* __restrict__ row_loads_device) {  // ForwardOptions::row_loads_device
  using A = Arith<float>;
  constexpr int kUnroll = Quantized4BitUnroll<N>();
  const bool stream_rows = row_loads_device != nullptr ? (*row_loads_device != 0u) : stream_rows_host;
  const int lane_x = threadIdx.x;
  const int code_bytes = CodeBytes4Bit(width);
  const int row_bytes = code_bytes + kQuantized4BitTrailerBytes;
  const uint8_t* lane_base = table + lane_x * (N / 2);
  const int64_t trailer_delta = code_bytes - lane_x * (N / 2);
  Quantized4BitRowPool<OutT, N, kWeighted> pool;
  const auto gather = [&](const int count, const auto index_at, const auto weight_at) {
    if (stream_rows) pool.template Gather<kUnroll, true>(lane_base, trailer_delta, row_bytes, count, index_at, weight_at);
    else pool.template Gather<kUnroll, false>(lane_base, trailer_delta, row_bytes, count, index_at, weight_at);
  };
  int64_t sample;
  int hot;
  if (!WalkSample<kSource, kWeighted>(blockIdx.x, batch, indices, offsets, num_hots, weights, sample_order, sample, hot,
                                      gather))   // (the walk of GatherReduceKernel: gather_reduce_kernels.hpp)
    return;

  // ---- epilogue: even / odd accumulators back into element order, the bag's bias once, mean scaling (MeanFactor),
  // one rounding to OutT ----
  const float inv = is_mean ? MeanFactor<kWeighted>(pool.weight_sum, hot) : 1.f;
  float v[N];
#pragma unroll
  for (int e = 0; e < N; ++e) {
    v[e] = A::add(pool.acc[e / 8][e % 2][(e % 8) / 2], pool.bias_sum);
    if (is_mean) v[e] = A::mul(v[e], inv);
  }
  StoreWideStreaming<OutT, N>(out + sample * static_cast<int64_t>(width) + lane_x * N, v);
}

}  // namespace detail
}  // namespace cuembed

#endif  // CUEMBED_INCLUDE_QUANTIZED_4BIT_ROWS_KERNELS_HPP_
