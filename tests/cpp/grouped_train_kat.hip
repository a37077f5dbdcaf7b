// Header-only API check of what trains a group beyond sum pooling with table gradients (grouped_backward.hpp):
// cuembed::EmbeddingWeightGradGrouped and cuembed::GroupedMeanScale on a group of three tables (11, 5 and 7 rows of
// width 8), CSR and fixed hotness, fp32 and fp16, against a host recomputation.
//
// Tables and grad_y hold small integers, so a lookup's dot product is exact in fp32 and in fp16 whatever the order of
// its sum; weights are 0.5 or 0.25, so a bag's weight sum is exact too; the scaled rows are recomputed on the host with
// the same fp32 operations (one reciprocal, one multiply, one rounding).  Bits must be equal.  B = 5 with T = 3: the
// table boundaries fall inside a wavefront.  Built and run by tests/test_gpu_cpp_grouped_train.py.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "cuembed/include/grouped_backward.hpp"

#define HIP_OK(x)                                                              \
  do {                                                                         \
    hipError_t e_ = (x);                                                       \
    if (e_ != hipSuccess) {                                                    \
      std::fprintf(stderr, "%s failed: %s\n", #x, hipGetErrorString(e_));      \
      std::exit(2);                                                            \
    }                                                                          \
  } while (0)

template <typename T> T From(float v);
template <> float From<float>(float v) { return v; }
template <> __half From<__half>(float v) { return __float2half(v); }
inline float ToF(float v) { return v; }
inline float ToF(__half v) { return __half2float(v); }

static int g_failures = 0;
static int g_checks = 0;

static void Expect(const bool ok, const char* what, const char* detail, const long at = -1) {
  ++g_checks;
  if (ok) return;
  ++g_failures;
  std::fprintf(stderr, "FAILED %s: %s (at %ld)\n", what, detail, at);
}

constexpr int kTables = 3;
constexpr int kRows[kTables] = {11, 5, 7};
constexpr int kWidth = 8;
constexpr int kBatch = 5;
constexpr int kBags = kTables * kBatch;
constexpr int kHot = 3;
// CSR bag lengths, bag g = t * kBatch + b: empty bags at a table boundary, one bag past the 8-lookup batch
constexpr int kLengths[kBags] = {2, 0, 9, 1, 0, 0, 4, 8, 3, 1, 16, 0, 1, 2, 0};

template <typename T>
T* Device(const std::vector<T>& h) {
  T* p = nullptr;
  HIP_OK(hipMalloc(reinterpret_cast<void**>(&p), (h.empty() ? 1 : h.size()) * sizeof(T)));
  if (!h.empty()) HIP_OK(hipMemcpy(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
  return p;
}

template <typename T>
std::vector<T> Host(const T* d, const size_t n) {
  std::vector<T> h(n);
  if (n) HIP_OK(hipMemcpy(h.data(), d, n * sizeof(T), hipMemcpyDeviceToHost));
  return h;
}

template <typename T>
bool SameBits(const T a, const T b) { return std::memcmp(&a, &b, sizeof(T)) == 0; }

static uint32_t Next(uint32_t& s) { return s = s * 1664525u + 1013904223u; }

template <typename T>
void Run(const char* name) {
  uint32_t seed = 12345u;
  // ---- the group: three allocations; integers in [-3, 3]
  std::vector<std::vector<T>> tables(kTables);
  std::vector<T*> d_tables(kTables);
  for (int t = 0; t < kTables; ++t) {
    tables[t].resize(static_cast<size_t>(kRows[t]) * kWidth);
    for (auto& v : tables[t]) v = From<T>(static_cast<float>(static_cast<int>(Next(seed) >> 8) % 7 - 3));
    d_tables[t] = Device(tables[t]);
  }
  std::vector<const T*> host_ptrs(d_tables.begin(), d_tables.end());
  const T** d_ptrs = nullptr;
  HIP_OK(hipMalloc(reinterpret_cast<void**>(&d_ptrs), kTables * sizeof(T*)));
  HIP_OK(hipMemcpy(d_ptrs, host_ptrs.data(), kTables * sizeof(T*), hipMemcpyHostToDevice));
  // ---- grad_y [B, T, W]: integers in [-2, 2]
  std::vector<T> grad_y(static_cast<size_t>(kBatch) * kTables * kWidth);
  for (auto& v : grad_y) v = From<T>(static_cast<float>(static_cast<int>(Next(seed) >> 8) % 5 - 2));
  T* d_grad_y = Device(grad_y);

  for (int fixed = 0; fixed < 2; ++fixed) {
    // ---- the lookups, bag after bag; ids of table t are rows of table t
    std::vector<int64_t> offsets(kBags + 1, 0);
    for (int g = 0; g < kBags; ++g) offsets[g + 1] = offsets[g] + (fixed ? kHot : kLengths[g]);
    const int nnz = static_cast<int>(offsets[kBags]);
    std::vector<int32_t> ids(nnz);
    std::vector<T> weights(nnz);
    for (int g = 0; g < kBags; ++g)
      for (int64_t p = offsets[g]; p < offsets[g + 1]; ++p) {
        ids[p] = static_cast<int32_t>((Next(seed) >> 8) % static_cast<uint32_t>(kRows[g / kBatch]));
        weights[p] = From<T>((Next(seed) >> 8) % 2 ? 0.5f : 0.25f);
      }
    int32_t* d_ids = Device(ids);
    int64_t* d_offsets = Device(offsets);
    T* d_weights = Device(weights);
    const int64_t* call_offsets = fixed ? nullptr : d_offsets;
    const int call_hots = fixed ? kHot : 0;

    // ---- the weight gradient
    std::vector<T> poison(nnz, From<T>(-77.f));
    T* d_grad_w = Device(poison);
    cuembed::EmbeddingWeightGradGrouped<T, int32_t, int64_t>(host_ptrs.data(), d_ptrs, kTables, kWidth, d_ids, call_offsets,
                                                             d_grad_y, kBatch, call_hots, d_grad_w);
    HIP_OK(hipDeviceSynchronize());
    const std::vector<T> grad_w = Host(d_grad_w, nnz);
    for (int g = 0; g < kBags; ++g) {
      const int t = g / kBatch, b = g % kBatch;
      const T* gy = grad_y.data() + (static_cast<size_t>(b) * kTables + t) * kWidth;
      for (int64_t p = offsets[g]; p < offsets[g + 1]; ++p) {
        float dot = 0.f;
        for (int e = 0; e < kWidth; ++e) dot += ToF(tables[t][static_cast<size_t>(ids[p]) * kWidth + e]) * ToF(gy[e]);
        Expect(SameBits(grad_w[p], From<T>(dot)), name, fixed ? "weight gradient, fixed hotness" : "weight gradient, CSR", p);
      }
    }

    // ---- the mean's scale: unweighted out of place, weighted in place
    for (int weighted = 0; weighted < 2; ++weighted) {
      T* d_out = weighted ? Device(grad_y) : Device(std::vector<T>(grad_y.size(), From<T>(-77.f)));
      cuembed::GroupedMeanScale<T, int64_t>(weighted ? d_out : d_grad_y, call_offsets, weighted ? d_weights : nullptr, kTables,
                                            kBatch, kWidth, call_hots, d_out);
      HIP_OK(hipDeviceSynchronize());
      const std::vector<T> out = Host(d_out, grad_y.size());
      for (int g = 0; g < kBags; ++g) {
        const int t = g / kBatch, b = g % kBatch;
        float denom = static_cast<float>(offsets[g + 1] - offsets[g]);
        if (weighted) {
          denom = 0.f;
          for (int64_t p = offsets[g]; p < offsets[g + 1]; ++p) denom += ToF(weights[p]);
        }
        const float f = denom == 0.f ? 0.f : 1.0f / denom;
        const size_t at = (static_cast<size_t>(b) * kTables + t) * kWidth;
        for (int e = 0; e < kWidth; ++e)
          Expect(SameBits(out[at + e], From<T>(ToF(grad_y[at + e]) * f)), name,
                 weighted ? "weighted mean scale, in place" : "mean scale", static_cast<long>(at + e));
      }
      HIP_OK(hipFree(d_out));
    }
    HIP_OK(hipFree(d_grad_w));
    HIP_OK(hipFree(d_weights));
    HIP_OK(hipFree(d_offsets));
    HIP_OK(hipFree(d_ids));
  }
  // the source of the out-of-place calls was left alone
  const std::vector<T> after = Host(d_grad_y, grad_y.size());
  for (size_t i = 0; i < grad_y.size(); ++i) Expect(SameBits(after[i], grad_y[i]), name, "grad_y was written", static_cast<long>(i));
  HIP_OK(hipFree(d_grad_y));
  HIP_OK(hipFree(d_ptrs));
  for (T* p : d_tables) HIP_OK(hipFree(p));
}

int main() {
  int devices = 0;
  if (hipGetDeviceCount(&devices) != hipSuccess || devices == 0) {
    std::fprintf(stderr, "grouped_train_kat: no GPU\n");
    return 2;
  }
  Run<float>("fp32");
  Run<__half>("fp16");
  if (g_failures) {
    std::fprintf(stderr, "%d of %d checks FAILED\n", g_failures, g_checks);
    return 1;
  }
  std::printf("grouped_train_kat: %d known-answer checks passed\n", g_checks);
  return 0;
}
