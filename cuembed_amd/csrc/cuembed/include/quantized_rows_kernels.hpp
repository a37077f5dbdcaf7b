// MI355X (gfx950 / CDNA4) kernels for 8-bit row-wise quantized tables (an extension: the reference has fp32 / fp16
// tables only).
//
// The format is PyTorch's "fused 8-bit row-wise" layout (quantized::embedding_bag_byte_prepack): a row of W values is
// W + 8 bytes -- W uint8 codes, then the row's fp32 scale and fp32 bias -- and a value is code * scale + bias.  A
// looked-up row of 256 values is 264 bytes instead of 512 (fp16): the gather-reduce is bound by the bytes it loads,
// so this is the one way left to make it faster.
//
//   QuantizeRowsKernel            fp32 / fp16 / bf16 [rows, W] -> fused rows, bit-identical to torch's CPU prepack
//   DequantizeRowsKernel          fused rows (all, or the rows a list of ids names) -> fp32 / fp16 [n, W]
//   GatherReduceQuantizedKernel   sum / mean of looked-up rows, fixed hotness or CSR, optionally weighted
//
// The gather is GatherReduceKernel's sample walk (WalkSample, gather_reduce_kernels.hpp) and mapping on 16-byte loads
// of CODES: one lane owns 16 codes (one global_load_dwordx4 at an 8-byte aligned address), a 256-value row is 16 lanes,
// a wavefront pools FOUR samples, and four lookups per sample are in flight before the first is consumed (narrower
// lanes, 8 or 4 codes, where the row does not divide into 16s: eight in flight).  Per lookup a lane spends 16
// v_cvt_f32_ubyte and 8 v_pk_fma_f32.
//   * scale and bias reach the lanes by ONE extra 8-byte load per lookup at an address all lanes of the row share
//     (a broadcast inside the load unit: no cross-lane instruction, no LDS); its address is the code address plus a
//     per-lane constant, so a lookup costs one id x row_bytes multiply, as in the fp16 kernel;
//   * the bias is not added per element: acc[e] = fma(code[e], w * scale, acc[e]) pools the codes, bias_sum =
//     fma(w, bias, bias_sum) pools the biases of the bag, and the epilogue adds bias_sum once.  fp32 throughout,
//     strictly in lookup order: a bag's result depends on nothing but the bag;
//   * row-load policy and sample order are scheduling hints, as in the fp16 kernel: no bit changes.
// Measured (profiles/quantized_forward_timing.json, docs/EXPERIMENTS.md): 8 codes per lane -- the fp16 kernel's 32
// lanes per row -- was SLOWER than the fp16 kernel on skewed indices; 16 codes per lane with eight lookups in flight
// needs 158 registers and loses to four in flight (72 registers).
#ifndef CUEMBED_INCLUDE_QUANTIZED_ROWS_KERNELS_HPP_
#define CUEMBED_INCLUDE_QUANTIZED_ROWS_KERNELS_HPP_

#include <cstdint>

#include "cuembed/include/embedding_types.hpp"
#include "cuembed/include/gather_reduce_kernels.hpp"

namespace cuembed {
namespace detail {

constexpr int kQuantizedTrailerBytes = 8;   //!< fp32 scale + fp32 bias behind the codes of a row
constexpr int kQuantizeThreads = 256;
//! Workgroup size limit of the 16-codes-per-lane gather (it keeps 8 x 24 bytes in flight and 16 sums per lane: the
//! 128 registers a 1,024-thread workgroup leaves a lane would spill); wider rows take 8 codes per lane.
constexpr int kQuantizedWideLaneThreads = 256;
constexpr int kQuantizeRegChunks = 4;       //!< packs of a row one lane keeps in registers (rows up to 64 x 4 packs)

//! N consecutive values of a row as 16-byte (or smaller) loads / stores: N x sizeof(T) may exceed one access.
template <typename T, int N>
struct WidePieces {
  static constexpr int kPiece = (N * static_cast<int>(sizeof(T)) > 16) ? 16 / static_cast<int>(sizeof(T)) : N;
  static constexpr int kPieces = N / kPiece;
};

//! Ordinary (cached) load of a pack.
template <typename T, int N>
__device__ __forceinline__ Pack<T, N> LoadPackCached(const T* p) {
  return *reinterpret_cast<const Pack<T, N>*>(p);
}

template <typename T, int N>
__device__ __forceinline__ void LoadWide(const T* p, float (&x)[N]) {
  using W = WidePieces<T, N>;
#pragma unroll
  for (int k = 0; k < W::kPieces; ++k) {
    const Pack<T, W::kPiece> v = LoadPackStreaming<T, W::kPiece>(p + k * W::kPiece);
#pragma unroll
    for (int e = 0; e < W::kPiece; ++e) x[k * W::kPiece + e] = static_cast<float>(v.v[e]);
  }
}

template <typename T, int N>
__device__ __forceinline__ void StoreWideStreaming(T* p, const float (&x)[N]) {
  using W = WidePieces<T, N>;
#pragma unroll
  for (int k = 0; k < W::kPieces; ++k) {
    Pack<T, W::kPiece> v;
#pragma unroll
    for (int e = 0; e < W::kPiece; ++e) v.v[e] = static_cast<T>(x[k * W::kPiece + e]);
    StorePackStreaming<T, W::kPiece>(p + k * W::kPiece, v);
  }
}

//! N codes of one lane.  Rows are W + 8 bytes, so a lane's codes are 8-byte aligned at best: 16 codes are one
//! global_load_dwordx4 at an 8-byte aligned address (the hardware needs dword alignment only).
template <int N>
struct alignas(N < 8 ? N : 8) CodePack {
  uint8_t v[N];
};
template <int N, bool kStream>
__device__ __forceinline__ CodePack<N> LoadCodes(const uint8_t* p) {
  typedef unsigned __attribute__((ext_vector_type(N / 4), aligned(N < 8 ? N : 8))) raw_t;
  raw_t raw;
  if constexpr (kStream) raw = __builtin_nontemporal_load(reinterpret_cast<const raw_t*>(p));
  else raw = *reinterpret_cast<const raw_t*>(p);
  return *reinterpret_cast<const CodePack<N>*>(&raw);
}

//! scale and bias of the row whose trailer starts at `p` (8-byte aligned exactly when kAligned8: W % 8 == 0).
struct ScaleBias {
  float scale, bias;
};
template <bool kAligned8, bool kStream>
__device__ __forceinline__ ScaleBias LoadScaleBias(const uint8_t* p) {
  ScaleBias sb;
  if constexpr (kAligned8) {
    const float* f = reinterpret_cast<const float*>(p);
    const Pack<float, 2> v = kStream ? LoadPackStreaming<float, 2>(f) : LoadPackCached<float, 2>(f);
    sb.scale = v.v[0];
    sb.bias = v.v[1];
  } else {
    const float* f = reinterpret_cast<const float*>(p);
    const Pack<float, 1> s = kStream ? LoadPackStreaming<float, 1>(f) : LoadPackCached<float, 1>(f);
    const Pack<float, 1> b = kStream ? LoadPackStreaming<float, 1>(f + 1) : LoadPackCached<float, 1>(f + 1);
    sb.scale = s.v[0];
    sb.bias = b.v[0];
  }
  return sb;
}

// ---------------------------------------------------------------------------
// Quantizer.  block = (group, kQuantizeThreads / group); grid = ceil(rows / blockDim.y).
// A group of `group` lanes (a power of two <= 64: never straddles a wavefront) owns a row; lane l holds packs l,
// l + group, ... of N values.  Rows of up to group x kQuantizeRegChunks packs (2,048 values with N = 8) are read
// once and kept in registers between the min / max reduction (a cross-lane butterfly) and the encoding; wider rows
// are read twice.  Arithmetic, every step one IEEE fp32 operation (Arith: no contraction), as torch's CPU prepack:
//     range = max - min;  scale = range / 255;  inv = 255 / (range + 1e-8);  code = rint((x - min) * inv);  bias = min
// ---------------------------------------------------------------------------
template <int N>
__device__ __forceinline__ Pack<uint8_t, N> EncodePack(const float (&x)[N], const float mn, const float inv) {
  using A = Arith<float>;
  Pack<uint8_t, N> codes;
#pragma unroll
  for (int e = 0; e < N; ++e)
    codes.v[e] = static_cast<uint8_t>(static_cast<int>(__builtin_rintf(A::mul(A::add(x[e], -mn), inv))));
  return codes;
}

template <typename InT, int N>
__global__ void __launch_bounds__(kQuantizeThreads)
QuantizeRowsKernel(const InT* __restrict__ in, const int width, const int64_t rows, uint8_t* __restrict__ out) {
  using A = Arith<float>;
  const int lane = threadIdx.x;
  const int group = blockDim.x;
  const int64_t row = static_cast<int64_t>(blockIdx.x) * blockDim.y + threadIdx.y;
  if (row >= rows) return;     // (the lanes of a group share the row: they leave together)
  const int packs = width / N;
  const InT* src = in + row * static_cast<int64_t>(width);
  uint8_t* dst = out + row * static_cast<int64_t>(width + kQuantizedTrailerBytes);
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
  const float range = A::add(mx, -mn);
  const float scale = range / 255.0f;
  const float inv = 255.0f / A::add(range, 1e-8f);
  if (in_registers) {
#pragma unroll
    for (int c = 0; c < kQuantizeRegChunks; ++c) {
      const int p = c * group + lane;
      if (p < packs) StorePackStreaming<uint8_t, N>(dst + static_cast<int64_t>(p) * N, EncodePack<N>(x[c], mn, inv));
    }
  } else {
    for (int p = lane; p < packs; p += group) {
      float y[N];
      LoadWide<InT, N>(src + static_cast<int64_t>(p) * N, y);
      StorePackStreaming<uint8_t, N>(dst + static_cast<int64_t>(p) * N, EncodePack<N>(y, mn, inv));
    }
  }
  if (lane == 0) {
    float* trailer = reinterpret_cast<float*>(dst + width);   // 4-byte aligned: W % 4 == 0
    trailer[0] = scale;
    trailer[1] = mn;
  }
}

// ---------------------------------------------------------------------------
// Dequantizer: out[i, :] = float(code) * scale + bias of row ids[i] (ids == nullptr: row i), two rounded fp32
// operations, then one rounding to OutT.  block = (lanes_per_row, rows_per_block); grid = ceil(n / rows_per_block).
// mode = "concat" of the lookup is this kernel on the batch's ids.
// ---------------------------------------------------------------------------
template <typename OutT, typename IndexT, int N>
__global__ void __launch_bounds__(kMaxBlockThreads)
DequantizeRowsKernel(const uint8_t* __restrict__ table, const int width, const IndexT* __restrict__ ids,
                     const int64_t n, OutT* __restrict__ out) {
  using A = Arith<float>;
  const int lane_x = threadIdx.x;
  const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.y + threadIdx.y;
  if (i >= n) return;
  const int64_t r = ids != nullptr ? WidenIndex(ids[i]) : i;
  const int row_bytes = width + kQuantizedTrailerBytes;
  const uint8_t* row = RowPtr<uint8_t>(table, r, row_bytes);
  const Pack<uint8_t, N> codes = LoadPackCached<uint8_t, N>(row + lane_x * N);
  const ScaleBias sb = LoadScaleBias<N == 8, false>(row + width);
  float v[N];
#pragma unroll
  for (int e = 0; e < N; ++e) v[e] = A::add(A::mul(static_cast<float>(codes.v[e]), sb.scale), sb.bias);
  StoreWideStreaming<OutT, N>(out + i * static_cast<int64_t>(width) + lane_x * N, v);
}

// ---------------------------------------------------------------------------
// Sum / mean on fused rows.
//   block = (lanes_per_row, samples_per_block); grid = ceil(batch / samples_per_block)
//   dynamic LDS (kLdsStaged only) = samples_per_block * num_hots * (sizeof(IndexT) [+ sizeof(OutT) if weighted])
// ---------------------------------------------------------------------------
template <typename OutT, int N, bool kWeighted>
struct QuantizedRowPool {
  float acc[N];       //!< sum_j w_j * scale_j * code_j[e]
  float bias_sum;     //!< sum_j w_j * bias_j
  float weight_sum;

  __device__ __forceinline__ QuantizedRowPool() : bias_sum(0.f), weight_sum(0.f) {
#pragma unroll
    for (int e = 0; e < N; ++e) acc[e] = 0.f;
  }

  __device__ __forceinline__ void Add(const CodePack<N>& codes, const ScaleBias sb, const OutT w) {
    using A = Arith<float>;
    if constexpr (kWeighted) {
      const float wf = static_cast<float>(w);
      const float ws = A::mul(wf, sb.scale);
      weight_sum += wf;
      bias_sum = __builtin_fmaf(wf, sb.bias, bias_sum);
#pragma unroll
      for (int e = 0; e < N; ++e) acc[e] = __builtin_fmaf(static_cast<float>(codes.v[e]), ws, acc[e]);
    } else {
      bias_sum = A::add(bias_sum, sb.bias);
#pragma unroll
      for (int e = 0; e < N; ++e) acc[e] = __builtin_fmaf(static_cast<float>(codes.v[e]), sb.scale, acc[e]);
    }
  }

  //! Pools `count` lookups in order; kUnroll code loads and as many trailer loads are issued back-to-back before the
  //! first is consumed (`sched_barrier` pins "all loads first"), the tail of a bag as one predicated batch (as
  //! RowPool::Gather, gather_reduce_kernels.hpp: the same batch loop on rows, kept apart on purpose,
  //! docs/EXPERIMENTS.md).
  //! lane_base = table + this lane's first code; the row's trailer is trailer_delta bytes behind the lane's codes
  //! (one 64-bit add on the address the codes are loaded from, instead of a second id x row_bytes multiply).
  template <int kUnroll, bool kStream, typename IndexFn, typename WeightFn>
  __device__ __forceinline__ void Gather(const uint8_t* lane_base, const int64_t trailer_delta, const int row_bytes,
                                         const int count, IndexFn index_at, WeightFn weight_at) {
    auto load_codes = [](const uint8_t* p) { return LoadCodes<N, kStream>(p); };
    int j = 0;
    for (; j + kUnroll <= count; j += kUnroll) {
      CodePack<N> codes[kUnroll];
      ScaleBias sb[kUnroll];
      OutT w[kUnroll];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int64_t r = index_at(j + u);
        if constexpr (kWeighted) w[u] = weight_at(j + u);
        const uint8_t* p = RowPtr<uint8_t>(lane_base, r, row_bytes);
        codes[u] = load_codes(p);
        sb[u] = LoadScaleBias<N >= 8, kStream>(p + trailer_delta);
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) Add(codes[u], sb[u], w[u]);
    }
    const int rem = count - j;
    if (rem > 0) {
      CodePack<N> codes[kUnroll];
      ScaleBias sb[kUnroll];
      OutT w[kUnroll];
#pragma unroll
      for (int u = 0; u < kUnroll - 1; ++u) {
        if (u < rem) {
          const int64_t r = index_at(j + u);
          if constexpr (kWeighted) w[u] = weight_at(j + u);
          const uint8_t* p = RowPtr<uint8_t>(lane_base, r, row_bytes);
          codes[u] = load_codes(p);
          sb[u] = LoadScaleBias<N >= 8, kStream>(p + trailer_delta);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < kUnroll - 1; ++u) {
        if (u < rem) Add(codes[u], sb[u], w[u]);
      }
    }
  }
};

template <typename OutT,     // output and weight element: float or _Float16
          typename IndexT,   // int32_t / int64_t
          typename OffsetT,  // CSR offset type (unused for kLdsStaged)
          int N,             // codes per lane: 16 (W % 16 == 0), 8 (W % 8 == 0) or 4
          bool kWeighted,
          IndexSource kSource,
          int kUnroll = (N == 16 ? 4 : kForwardUnroll)>   // lookups in flight: the same 96..128 bytes per lane either way
__global__ void __launch_bounds__(N == 16 ? kQuantizedWideLaneThreads : kMaxBlockThreads)
GatherReduceQuantizedKernel(const uint8_t* __restrict__ table,
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
  const bool stream_rows = row_loads_device != nullptr ? (*row_loads_device != 0u) : stream_rows_host;
  const int lane_x = threadIdx.x;
  const int row_bytes = width + kQuantizedTrailerBytes;
  const uint8_t* lane_base = table + lane_x * N;
  const int64_t trailer_delta = width - lane_x * N;
  QuantizedRowPool<OutT, N, kWeighted> pool;
  const auto gather = [&](const int count, const auto index_at, const auto weight_at) {
    if (stream_rows) pool.template Gather<kUnroll, true>(lane_base, trailer_delta, row_bytes, count, index_at, weight_at);
    else pool.template Gather<kUnroll, false>(lane_base, trailer_delta, row_bytes, count, index_at, weight_at);
  };
  int64_t sample;
  int hot;
  if (!WalkSample<kSource, kWeighted>(blockIdx.x, batch, indices, offsets, num_hots, weights, sample_order, sample, hot,
                                      gather))   // (the walk of GatherReduceKernel: gather_reduce_kernels.hpp)
    return;

  // ---- epilogue: the bag's bias once, mean scaling (MeanFactor, as FinishPooledRow), one rounding to OutT ----
  const float inv = is_mean ? MeanFactor<kWeighted>(pool.weight_sum, hot) : 1.f;
  float v[N];
#pragma unroll
  for (int e = 0; e < N; ++e) {
    v[e] = A::add(pool.acc[e], pool.bias_sum);
    if (is_mean) v[e] = A::mul(v[e], inv);
  }
  StoreWideStreaming<OutT, N>(out + sample * static_cast<int64_t>(width) + lane_x * N, v);
}

}  // namespace detail
}  // namespace cuembed

#endif  // CUEMBED_INCLUDE_QUANTIZED_ROWS_KERNELS_HPP_
