// Header-only API check of cuembed::EmbeddingBackwardMixedGroup and cuembed::MixedGroupMeanScale
// (mixed_group_backward.hpp) on the hand-written group of mixed_group_kat.hip, with the answers written out below: three
// fp32 tables of widths 4, 8 and 2 (5, 3 and 4 rows; row_base 0, 5, 8, 12), two samples per table, grad_y [2, 14] with
// grad_y[b, c] = 100 (b + 1) + c.  The chain is the library's own: GroupedBackwardKeys, Transpose with the remapped ids,
// the mixed scatter-add.  The outputs are filled with a sentinel first: entries at and past the count stay untouched,
// padding columns hold the sentinel or zero, and with capacity_rows = count - 1 NOTHING is written and the overflow
// word is raised.  Built and run by tests/test_gpu_cpp_mixed_group_backward.py.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "cuembed/include/grouped_backward.hpp"
#include "cuembed/include/index_transforms.hpp"
#include "cuembed/include/mixed_group_backward.hpp"

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

template <typename T>
std::vector<T> Host(const T* device, const size_t n) {
  std::vector<T> h(n);
  HIP_OK(hipMemcpy(h.data(), device, n * sizeof(T), hipMemcpyDeviceToHost));
  return h;
}

static void Expect(const bool ok, const char* what, const long long at, const double got, const double want) {
  ++g_checks;
  if (ok) return;
  ++g_failures;
  std::fprintf(stderr, "FAILED %s[%lld]: got %g, want %g\n", what, at, got, want);
}

int main() {
  constexpr int kTables = 3, kBatch = 2, kDim = 14, kMaxWidth = 8, kCapacity = 10, kCount = 8;
  constexpr float kSentinel = -7.f;
  const int widths[kTables] = {4, 8, 2};
  const std::vector<int64_t> row_base = {0, 5, 8, 12};
  const std::vector<int32_t> table_columns = {0, 4, 4, 8, 12, 2};   // (c_t, W_t)
  std::vector<float> grad_y(kBatch * kDim);
  for (int b = 0; b < kBatch; ++b)
    for (int c = 0; c < kDim; ++c) grad_y[b * kDim + c] = 100.f * (b + 1) + c;
  // bags (t, b) = (0,0): rows 1, 3; (0,1): empty; (1,0): row 2; (1,1): rows 0, 0, 1; (2,0): row 3; (2,1): rows 0, 2
  const std::vector<int32_t> indices = {1, 3, 2, 0, 0, 1, 3, 0, 2};
  const std::vector<int64_t> offsets = {0, 2, 2, 3, 6, 7, 9};
  const int nnz = static_cast<int>(indices.size());

  const int64_t* d_row_base = Device(row_base);
  const int32_t* d_columns = Device(table_columns);
  const float* d_grad_y = Device(grad_y);
  const int32_t* d_indices = Device(indices);
  const int64_t* d_offsets = Device(offsets);
  int32_t* d_keys = Device(std::vector<int32_t>(nnz));
  int32_t* d_sids = Device(std::vector<int32_t>(nnz));
  int32_t* d_tkeys = Device(std::vector<int32_t>(nnz));
  int32_t* d_tsids = Device(std::vector<int32_t>(nnz));
  int32_t* d_remap = Device(std::vector<int32_t>(nnz));

  cuembed::GroupedBackwardKeys<int32_t, int64_t, int32_t>(d_indices, d_offsets, d_row_base, kTables, kBatch, 0, nnz, d_keys,
                                                          d_sids);
  size_t lwork = 0;
  cuembed::Transpose<int32_t, float>(d_sids, d_keys, nullptr, nnz, d_tkeys, d_tsids, nullptr, nullptr, &lwork, 0, 4, 0, 1,
                                     d_remap);
  char* d_work = nullptr;
  HIP_OK(hipMalloc(reinterpret_cast<void**>(&d_work), lwork > 0 ? lwork : 1));
  cuembed::Transpose<int32_t, float>(d_sids, d_keys, nullptr, nnz, d_tkeys, d_tsids, nullptr, d_work, &lwork, 0, 4, 0, 1,
                                     d_remap);
  HIP_OK(hipDeviceSynchronize());
  {
    const int32_t want_keys[9] = {1, 3, 5, 5, 6, 7, 8, 10, 11};
    const int32_t want_remap[9] = {0, 1, 2, 2, 3, 4, 5, 6, 7};
    const std::vector<int32_t> keys = Host(d_tkeys, nnz), remap = Host(d_remap, nnz);
    for (int i = 0; i < nnz; ++i) {
      Expect(keys[i] == want_keys[i], "sorted key", i, keys[i], want_keys[i]);
      Expect(remap[i] == want_remap[i], "remapped id", i, remap[i], want_remap[i]);
    }
  }

  // ---- the scatter-add into sentinel-filled buffers of 10 entries ------------------------------------------------------
  const std::vector<float> rows_fill(kCapacity * kMaxWidth, kSentinel);
  const std::vector<int32_t> ids_fill(kCapacity, -7);
  float* d_rows = Device(rows_fill);
  int32_t* d_ids = Device(ids_fill);
  uint32_t* d_overflow = Device(std::vector<uint32_t>(1, 0u));
  cuembed::EmbeddingBackwardMixedGroup<float, int32_t>(d_grad_y, widths, d_columns, kTables, kBatch, nnz, d_tkeys, d_tsids,
                                                       d_remap, nullptr, d_rows, d_ids, 0, kCapacity, d_overflow);
  HIP_OK(hipDeviceSynchronize());
  // entry -> (global id, table, the gradient's first value, its step per lookup of the row)
  const int32_t want_ids[kCount] = {1, 3, 5, 6, 7, 8, 10, 11};
  const int want_table[kCount] = {0, 0, 1, 1, 1, 2, 2, 2};
  // id 1, 3: grad_y[0, 0:4]; id 5: 2 x grad_y[1, 4:12]; id 6: grad_y[1, 4:12]; id 7: grad_y[0, 4:12];
  // id 8, 10: grad_y[1, 12:14]; id 11: grad_y[0, 12:14]
  const float want_first[kCount] = {100, 100, 408, 204, 104, 212, 212, 112};
  const float want_step[kCount] = {1, 1, 2, 1, 1, 1, 1, 1};
  {
    const std::vector<float> rows = Host(d_rows, rows_fill.size());
    const std::vector<int32_t> ids = Host(d_ids, ids_fill.size());
    for (int k = 0; k < kCapacity; ++k) {
      Expect(ids[k] == (k < kCount ? want_ids[k] : -7), "inverse_mapping", k, ids[k], k < kCount ? want_ids[k] : -7);
      for (int c = 0; c < kMaxWidth; ++c) {
        const float got = rows[k * kMaxWidth + c];
        if (k < kCount && c < widths[want_table[k]]) {
          const float want = want_first[k] + want_step[k] * c;
          Expect(got == want, "gradient", k * kMaxWidth + c, got, want);
        } else if (k < kCount) {
          Expect(got == kSentinel || got == 0.f, "padding column (untouched or zero)", k * kMaxWidth + c, got, kSentinel);
        } else {
          Expect(got == kSentinel, "row past the count (untouched)", k * kMaxWidth + c, got, kSentinel);
        }
      }
    }
    Expect(Host(d_overflow, 1)[0] == 0u, "overflow word", 0, Host(d_overflow, 1)[0], 0);
  }

  // ---- capacity_rows = count - 1: nothing is written, the word is raised ----------------------------------------------
  HIP_OK(hipMemcpy(d_rows, rows_fill.data(), rows_fill.size() * sizeof(float), hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(d_ids, ids_fill.data(), ids_fill.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  cuembed::EmbeddingBackwardMixedGroup<float, int32_t>(d_grad_y, widths, d_columns, kTables, kBatch, nnz, d_tkeys, d_tsids,
                                                       d_remap, nullptr, d_rows, d_ids, 0, kCount - 1, d_overflow);
  HIP_OK(hipDeviceSynchronize());
  {
    const std::vector<float> rows = Host(d_rows, rows_fill.size());
    const std::vector<int32_t> ids = Host(d_ids, ids_fill.size());
    for (size_t i = 0; i < rows.size(); ++i) Expect(rows[i] == kSentinel, "overflow: gradient untouched", i, rows[i], kSentinel);
    for (size_t i = 0; i < ids.size(); ++i) Expect(ids[i] == -7, "overflow: inverse_mapping untouched", i, ids[i], -7);
    Expect(Host(d_overflow, 1)[0] == 1u, "overflow word", 0, Host(d_overflow, 1)[0], 1);
  }

  // ---- the mean's scale, weighted: powers of two, so that every step is exact ------------------------------------------
  const std::vector<float> weights = {0.5f, 0.5f, 2.f, 1.f, 1.f, 2.f, 4.f, 0.25f, 0.75f};
  const float* d_weights = Device(weights);
  float* d_scaled = Device(std::vector<float>(kBatch * kDim, kSentinel));
  cuembed::MixedGroupMeanScale<float, int64_t>(d_grad_y, widths, d_columns, d_offsets, d_weights, kTables, kBatch, 0, d_scaled);
  HIP_OK(hipDeviceSynchronize());
  {
    // bag weights sum to (0,0): 1; (0,1): empty -> factor 0; (1,0): 2; (1,1): 4; (2,0): 4; (2,1): 1
    const float factor[kBatch][kTables] = {{1.f, 0.5f, 0.25f}, {0.f, 0.25f, 1.f}};
    const std::vector<float> scaled = Host(d_scaled, kBatch * kDim);
    for (int b = 0; b < kBatch; ++b)
      for (int c = 0; c < kDim; ++c) {
        const int t = c < 4 ? 0 : (c < 12 ? 1 : 2);
        const float want = grad_y[b * kDim + c] * factor[b][t];
        Expect(scaled[b * kDim + c] == want, "mean scale", b * kDim + c, scaled[b * kDim + c], want);
      }
  }
  HIP_OK(hipGetLastError());

  if (g_failures != 0) {
    std::fprintf(stderr, "%d of %d checks FAILED\n", g_failures, g_checks);
    return 1;
  }
  std::printf("mixed group backward: %d known-answer checks passed\n", g_checks);
  return 0;
}
