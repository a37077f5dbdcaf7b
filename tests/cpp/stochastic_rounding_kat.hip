// Header-only API check of stochastic rounding in the sparse optimizer step (cuembed::SparseRowUpdate with
// options.stochastic_rounding, sparse_update.hpp + stochastic_rounding.hpp): Philox4x32-10 against Random123's known
// answers on the host, then SGD on arbitrary data with __half / __hip_bfloat16 tables, int32 / int64 ids, every lane
// width and body, the step as an argument and as a device word -- the table must equal a host recomputation that
// rounds with the SAME __host__ __device__ functions and the field of (seed, step, table row, column), bit for bit,
// and rows that no valid entry names must be untouched.  Built by __graft_entry__.build() (compile check, no GPU
// needed), run by tests/test_gpu_cpp_stochastic_rounding.py.
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "cuembed/include/sparse_update.hpp"

#define HIP_OK(x)                                                              \
  do {                                                                         \
    hipError_t e_ = (x);                                                       \
    if (e_ != hipSuccess) {                                                    \
      std::fprintf(stderr, "%s failed: %s\n", #x, hipGetErrorString(e_));      \
      std::exit(2);                                                            \
    }                                                                          \
  } while (0)

template <typename T>
struct DeviceArray {
  T* ptr = nullptr;
  size_t n = 0;
  explicit DeviceArray(const std::vector<T>& h) : n(h.size()) {
    HIP_OK(hipMalloc(&ptr, (n ? n : 1) * sizeof(T)));
    if (n) HIP_OK(hipMemcpy(ptr, h.data(), n * sizeof(T), hipMemcpyHostToDevice));
  }
  ~DeviceArray() { (void)hipFree(ptr); }
  std::vector<T> host() const {
    std::vector<T> h(n);
    if (n) HIP_OK(hipMemcpy(h.data(), ptr, n * sizeof(T), hipMemcpyDeviceToHost));
    return h;
  }
};

template <typename T> T From(float v);
template <> __half From<__half>(float v) { return __float2half(v); }
template <> __hip_bfloat16 From<__hip_bfloat16>(float v) { return __float2bfloat16(v); }
inline float ToF(__half v) { return __half2float(v); }
inline float ToF(__hip_bfloat16 v) { return __bfloat162float(v); }
inline uint16_t RoundBits(__half, float x, uint32_t r) { return cuembed::detail::StochasticRoundToHalfBits(x, r); }
inline uint16_t RoundBits(__hip_bfloat16, float x, uint32_t r) { return cuembed::detail::StochasticRoundToBf16Bits(x, r); }
template <typename T>
uint16_t Bits(T v) {
  uint16_t b;
  std::memcpy(&b, &v, 2);
  return b;
}

static int g_failures = 0;
static int g_checks = 0;

static void Check(bool ok, const char* what) {
  ++g_checks;
  if (!ok) {
    ++g_failures;
    std::fprintf(stderr, "MISMATCH %s\n", what);
  }
}

static uint32_t g_lcg = 12345u;
static float NextUniform() {   // (-1, 1), arbitrary mantissas
  g_lcg = g_lcg * 1664525u + 1013904223u;
  return (static_cast<float>(g_lcg >> 8) / 8388608.f) - 1.f;
}

constexpr int kRows = 40;
constexpr int kCapacity = 11;   // entries the gradient buffers hold (odd: one group's second in-flight entry is dead)
constexpr int kValid = 9;
constexpr float kLr = 0.0371f;
constexpr uint64_t kSeed = 0x9E3779B97F4A7C15ull;

template <typename ElemT, typename IndexT>
void Case(const int width, const bool step_on_device, hipStream_t stream, const char* what) {
  using A = cuembed::detail::Arith<float>;
  const int ids_h[kCapacity] = {3, 17, 0, 39, 5, 9, 21, 8, 30, 17, 3};   // the last two repeat valid rows: no effect
  const uint64_t step = 0x100000005ull;   // (the high word goes into the key)
  std::vector<ElemT> table(static_cast<size_t>(kRows) * width), grad(static_cast<size_t>(kCapacity) * width);
  for (auto& v : table) v = From<ElemT>(NextUniform());
  for (auto& v : grad) v = From<ElemT>(NextUniform());
  std::vector<ElemT> want = table;
  for (int k = 0; k < kValid; ++k) {
    const int r = ids_h[k];
    for (int j = 0; j < width; ++j) {
      const float x = A::add(ToF(table[static_cast<size_t>(r) * width + j]),
                             -A::mul(kLr, ToF(grad[static_cast<size_t>(k) * width + j])));
      const cuembed::detail::PhiloxWords p = cuembed::detail::RoundingWords(kSeed, step, r, j / 8);
      const uint16_t b = RoundBits(ElemT(), x, cuembed::detail::RoundingField(p, j % 8));
      std::memcpy(&want[static_cast<size_t>(r) * width + j], &b, 2);
    }
  }
  std::vector<IndexT> ids_e(ids_h, ids_h + kCapacity);
  DeviceArray<ElemT> d_table(table), d_grad(grad);
  DeviceArray<IndexT> d_ids(ids_e);
  DeviceArray<int64_t> d_step(std::vector<int64_t>{static_cast<int64_t>(step)});
  cuembed::SparseUpdateOptions o;
  o.rule = cuembed::UpdateRule::kSgd;
  o.lr = kLr;
  o.piece_rows = kCapacity;
  o.num_rows = kValid;
  o.stochastic_rounding = true;
  o.rounding_seed = kSeed;
  if (step_on_device) o.rounding_step_device = d_step.ptr, o.rounding_step = 77;   // (the argument is then ignored)
  else o.rounding_step = step;
  cuembed::SparseRowUpdate<ElemT, IndexT>(d_table.ptr, nullptr, width, d_ids.ptr, d_grad.ptr, o, stream);
  HIP_OK(hipGetLastError());
  HIP_OK(hipStreamSynchronize(stream));
  const std::vector<ElemT> got = d_table.host();
  bool ok = true;
  for (size_t i = 0; i < got.size(); ++i) ok = ok && Bits(got[i]) == Bits(want[i]);
  if (!ok) std::fprintf(stderr, "  (%s width %d step_on_device %d)\n", what, width, static_cast<int>(step_on_device));
  Check(ok, "stochastic SGD against the host recomputation");
}

template <typename ElemT, typename IndexT>
void Kat(hipStream_t stream, const char* what) {
  // 8: one 16-byte lane; 6: 4-byte lanes; 12: 8-byte lanes; 520: four slices per lane; 2056: the run-time loop
  const int widths[] = {8, 6, 12, 520, 2056};
  for (const int width : widths)
    for (const bool on_device : {false, true}) Case<ElemT, IndexT>(width, on_device, stream, what);
}

int main() {
  // Philox4x32-10 known answers (Random123's kat_vectors), on the host
  {
    using cuembed::detail::Philox4x32_10;
    const cuembed::detail::PhiloxWords a = Philox4x32_10(0, 0, 0, 0, 0, 0);
    Check(a.w[0] == 0x6627e8d5u && a.w[1] == 0xe169c58du && a.w[2] == 0xbc57ac4cu && a.w[3] == 0x9b00dbd8u, "philox zeros");
    const cuembed::detail::PhiloxWords b =
        Philox4x32_10(0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu);
    Check(b.w[0] == 0x408f276du && b.w[1] == 0x41c83b0eu && b.w[2] == 0xa20bc7c6u && b.w[3] == 0x6d5451fdu, "philox ones");
    const cuembed::detail::PhiloxWords c =
        Philox4x32_10(0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u, 0xa4093822u, 0x299f31d0u);
    Check(c.w[0] == 0xd16cfe09u && c.w[1] == 0x94fdccebu && c.w[2] == 0x5001e420u && c.w[3] == 0x24126ea1u, "philox pi");
  }
  hipStream_t stream;
  HIP_OK(hipStreamCreate(&stream));
  Kat<__half, int32_t>(stream, "half/int32");
  Kat<__half, int64_t>(stream, "half/int64");
  Kat<__hip_bfloat16, int32_t>(stream, "bf16/int32");
  Kat<__hip_bfloat16, int64_t>(stream, "bf16/int64");
  HIP_OK(hipStreamDestroy(stream));
  if (g_failures) {
    std::fprintf(stderr, "%d of %d stochastic-rounding checks failed\n", g_failures, g_checks);
    return 1;
  }
  std::printf("stochastic rounding: all %d known-answer checks passed\n", g_checks);
  return 0;
}
