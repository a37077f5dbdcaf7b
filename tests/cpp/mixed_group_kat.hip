// Header-only API check of cuembed::EmbeddingForwardMixedGroup (mixed_group_lookup.hpp) on a small hand-written group
// whose answers are written out below: three fp32 tables of widths 4, 8 and 2 (5, 3 and 4 rows), two samples per table,
// table t's element [r, c] = 100 * (t + 1) + 10 * r + c (sums of a few of them are exact in fp32).  First CSR with an
// empty bag, sum and weighted mean; then fixed hotness 2, sum.  The result [2, 14] sits between guard words.
// Built and run by tests/test_gpu_cpp_mixed_group.py.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "cuembed/include/mixed_group_lookup.hpp"

#define HIP_OK(x)                                                              \
  do {                                                                         \
    hipError_t e_ = (x);                                                       \
    if (e_ != hipSuccess) {                                                    \
      std::fprintf(stderr, "%s failed: %s\n", #x, hipGetErrorString(e_));      \
      std::exit(2);                                                            \
    }                                                                          \
  } while (0)

static int g_failures = 0;
static int g_checks = 0;

template <typename T>
T* Device(const std::vector<T>& h) {
  T* p = nullptr;
  HIP_OK(hipMalloc(reinterpret_cast<void**>(&p), (h.empty() ? 1 : h.size()) * sizeof(T)));
  if (!h.empty()) HIP_OK(hipMemcpy(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
  return p;
}

static void ExpectArray(const float* device, const std::vector<float>& want, const char* what) {
  std::vector<float> got(want.size());
  HIP_OK(hipMemcpy(got.data(), device, want.size() * sizeof(float), hipMemcpyDeviceToHost));
  for (size_t i = 0; i < want.size(); ++i) {
    ++g_checks;
    if (got[i] == want[i]) continue;
    ++g_failures;
    std::fprintf(stderr, "FAILED %s[%zu]: got %g, want %g\n", what, i, got[i], want[i]);
  }
}

static void ExpectInt(const long long got, const long long want, const char* what) {
  ++g_checks;
  if (got == want) return;
  ++g_failures;
  std::fprintf(stderr, "FAILED %s: got %lld, want %lld\n", what, got, want);
}

int main() {
  constexpr int kTables = 3, kBatch = 2, kDim = 14, kGuard = 4;
  const int widths[kTables] = {4, 8, 2};
  const int rows[kTables] = {5, 3, 4};
  float* d_table[kTables];
  for (int t = 0; t < kTables; ++t) {
    std::vector<float> h(static_cast<size_t>(rows[t]) * widths[t]);
    for (int r = 0; r < rows[t]; ++r)
      for (int c = 0; c < widths[t]; ++c) h[static_cast<size_t>(r) * widths[t] + c] = 100.f * (t + 1) + 10.f * r + c;
    d_table[t] = Device(h);
  }
  const float* tables_host[kTables] = {d_table[0], d_table[1], d_table[2]};
  const float** tables_device = nullptr;
  HIP_OK(hipMalloc(reinterpret_cast<void**>(&tables_device), sizeof(tables_host)));
  HIP_OK(hipMemcpy(tables_device, tables_host, sizeof(tables_host), hipMemcpyHostToDevice));

  // the result, between guard words
  const std::vector<float> guard_fill(kGuard + kBatch * kDim + kGuard, -7.f);
  float* d_buffer = Device(guard_fill);
  float* d_out = d_buffer + kGuard;

  // ---- the descriptor: widths 4, 8, 2 in fp32 -> D * 4 = 56 and W_2 * 4 = 8 bytes: 8-byte lanes, N = 2 ----------------
  const int lane_bytes = cuembed::MixedGroupLaneBytes(reinterpret_cast<const void* const*>(tables_host), widths, kTables, 4,
                                                      d_out);
  ExpectInt(lane_bytes, 8, "lane bytes");
  ExpectInt(static_cast<long long>(cuembed::MixedGroupDescriptorBytes(kTables)), 64, "descriptor bytes");
  std::vector<int32_t> blob(16, -1);
  const int grid = cuembed::FillMixedGroupDescriptor(widths, kTables, 4, lane_bytes, kBatch, cuembed::kMixedGroupBlockThreads,
                                                     blob.data());
  // lanes per bag 2, 4, 1 -> 128, 64, 256 bags per workgroup -> one workgroup per table
  const int32_t want_blob[16] = {4, 0, 2, 0, 8, 4, 4, 1, 2, 12, 1, 2, 0, 14, 0, 3};
  ExpectInt(grid, 3, "grid");
  for (int i = 0; i < 16; ++i) ExpectInt(blob[i], want_blob[i], "descriptor word");
  int32_t* d_descriptor = Device(blob);

  // ---- CSR: bags (t, b) = (0,0): rows 1, 3; (0,1): empty; (1,0): row 2; (1,1): rows 0, 0, 1; (2,0): row 3; (2,1): 0, 2
  const std::vector<int32_t> indices = {1, 3, 2, 0, 0, 1, 3, 0, 2};
  const std::vector<int64_t> offsets = {0, 2, 2, 3, 6, 7, 9};
  int32_t* d_indices = Device(indices);
  int64_t* d_offsets = Device(offsets);
  cuembed::EmbeddingForwardMixedGroup<float, float, int32_t, int64_t>(
      tables_host, tables_device, widths, d_descriptor, kTables, d_indices, d_offsets, nullptr, kBatch, 0,
      cuembed::CombineMode::kSum, d_out);
  HIP_OK(hipDeviceSynchronize());
  std::vector<float> want = guard_fill;
  {
    const float sum[kBatch * kDim] = {
        // sample 0: table 0 rows 1 + 3 (110 + c) + (130 + c); table 1 row 2 (220 + c); table 2 row 3 (330 + c)
        240, 242, 244, 246, 220, 221, 222, 223, 224, 225, 226, 227, 330, 331,
        // sample 1: empty; table 1 rows 0 + 0 + 1: 2 (200 + c) + (210 + c); table 2 rows 0 + 2: (300 + c) + (320 + c)
        0, 0, 0, 0, 610, 613, 616, 619, 622, 625, 628, 631, 620, 622};
    for (int i = 0; i < kBatch * kDim; ++i) want[kGuard + i] = sum[i];
  }
  ExpectArray(d_buffer, want, "CSR sum");

  // ---- the same bags, weighted mean: weights that are powers of two, so that every step is exact -----------------------
  const std::vector<float> weights = {0.5f, 0.5f, 2.f, 1.f, 1.f, 2.f, 4.f, 0.25f, 0.75f};
  float* d_weights = Device(weights);
  HIP_OK(hipMemcpy(d_buffer, guard_fill.data(), guard_fill.size() * sizeof(float), hipMemcpyHostToDevice));
  cuembed::EmbeddingForwardMixedGroup<float, float, int32_t, int64_t>(
      tables_host, tables_device, widths, d_descriptor, kTables, d_indices, d_offsets, d_weights, kBatch, 0,
      cuembed::CombineMode::kMean, d_out);
  HIP_OK(hipDeviceSynchronize());
  {
    const float mean[kBatch * kDim] = {
        // (0,0): (0.5 (110 + c) + 0.5 (130 + c)) / 1; (1,0): 2 (220 + c) / 2; (2,0): 4 (330 + c) / 4
        120, 121, 122, 123, 220, 221, 222, 223, 224, 225, 226, 227, 330, 331,
        // (0,1): empty -> zeros; (1,1): ((200 + c) + (200 + c) + 2 (210 + c)) / 4 = 205 + c;
        // (2,1): (0.25 (300 + c) + 0.75 (320 + c)) / 1 = 315 + c
        0, 0, 0, 0, 205, 206, 207, 208, 209, 210, 211, 212, 315, 316};
    for (int i = 0; i < kBatch * kDim; ++i) want[kGuard + i] = mean[i];
  }
  ExpectArray(d_buffer, want, "CSR weighted mean");

  // ---- fixed hotness 2, int64 ids: indices [T, B, H] ---------------------------------------------------------------------
  const std::vector<int64_t> fixed = {0, 4, 2, 2, /* table 1 */ 1, 2, 0, 1, /* table 2 */ 3, 3, 1, 0};
  int64_t* d_fixed = Device(fixed);
  HIP_OK(hipMemcpy(d_buffer, guard_fill.data(), guard_fill.size() * sizeof(float), hipMemcpyHostToDevice));
  cuembed::EmbeddingForwardMixedGroup<float, float, int64_t, int32_t>(
      tables_host, tables_device, widths, d_descriptor, kTables, d_fixed, nullptr, nullptr, kBatch, 2,
      cuembed::CombineMode::kSum, d_out);
  HIP_OK(hipDeviceSynchronize());
  {
    const float sum[kBatch * kDim] = {
        // sample 0: rows 0 + 4 of table 0: (100 + c) + (140 + c); rows 1 + 2 of table 1: (210 + c) + (220 + c);
        // rows 3 + 3 of table 2: 2 (330 + c)
        240, 242, 244, 246, 430, 432, 434, 436, 438, 440, 442, 444, 660, 662,
        // sample 1: rows 2 + 2: 2 (120 + c); rows 0 + 1: (200 + c) + (210 + c); rows 1 + 0: (310 + c) + (300 + c)
        240, 242, 244, 246, 410, 412, 414, 416, 418, 420, 422, 424, 610, 612};
    for (int i = 0; i < kBatch * kDim; ++i) want[kGuard + i] = sum[i];
  }
  ExpectArray(d_buffer, want, "fixed-hotness sum");
  HIP_OK(hipGetLastError());

  if (g_failures != 0) {
    std::fprintf(stderr, "%d of %d checks FAILED\n", g_failures, g_checks);
    return 1;
  }
  std::printf("mixed group forward: %d known-answer checks passed\n", g_checks);
  return 0;
}
