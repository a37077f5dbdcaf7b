// Header-only API check of cuembed::CheckIndices (index_check.hpp) on a small hand-written batch whose answers are
// written out below: a three-table CSR group (11, 5 and 7 rows, two bags per table) with one decreasing offset, one
// offset past nnz and five bad ids -- at a table's row count, negative, INT32_MIN, and valid for the neighbouring table
// only --, out of place; the repaired batch checked again in place (a zero report over garbage, nothing changed); and a
// fixed-hotness table with int64 ids, report only.  The workspace is exactly the queried size, filled with 0xFF.
// Built and run by tests/test_gpu_cpp_index_check.py.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "cuembed/include/index_check.hpp"

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
T* Device(const std::vector<T>& h, const size_t at_least = 1) {
  T* p = nullptr;
  const size_t n = h.size() > at_least ? h.size() : at_least;
  HIP_OK(hipMalloc(reinterpret_cast<void**>(&p), n * sizeof(T)));
  if (!h.empty()) HIP_OK(hipMemcpy(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
  return p;
}

template <typename T>
void ExpectArray(const T* device, const std::vector<T>& want, const char* what) {
  std::vector<T> got(want.size());
  HIP_OK(hipMemcpy(got.data(), device, want.size() * sizeof(T), hipMemcpyDeviceToHost));
  for (size_t i = 0; i < want.size(); ++i) {
    ++g_checks;
    if (got[i] == want[i]) continue;
    ++g_failures;
    std::fprintf(stderr, "FAILED %s[%zu]: got %lld, want %lld\n", what, i, static_cast<long long>(got[i]),
                 static_cast<long long>(want[i]));
  }
}

static char* Workspace(const size_t bytes) {
  char* work = nullptr;
  HIP_OK(hipMalloc(reinterpret_cast<void**>(&work), bytes > 0 ? bytes : 8));
  HIP_OK(hipMemset(work, 0xFF, bytes > 0 ? bytes : 8));
  return work;
}

int main() {
  // ---- a three-table group, CSR -------------------------------------------------------------------------------------
  constexpr int kTables = 3, kBatch = 2;
  const std::vector<int64_t> row_base = {0, 11, 16, 23};          // 11, 5 and 7 rows
  const std::vector<int32_t> offsets = {0, 2, 2, 5, 4, 9, 12};    // [4] decreases, [6] lies past nnz = 10
  const std::vector<int32_t> repaired_offsets = {0, 2, 2, 5, 5, 9, 10};
  // cuts r[0], r[2], r[4], r[6] = 0, 2, 5, 10: table 0 owns positions 0-1, table 1 2-4, table 2 5-9
  const std::vector<int32_t> indices = {10, 11, 4, 5, -1, 6, 7, 0, INT32_MIN, 3};
  const std::vector<int32_t> repaired_indices = {10, 0, 4, 0, 0, 6, 0, 0, 0, 3};
  const int64_t nnz = 10;
  int64_t* d_base = Device(row_base);
  int32_t* d_offsets = Device(offsets);
  int32_t* d_indices = Device(indices);
  int32_t* d_offsets_out = Device(std::vector<int32_t>(offsets.size(), -7));
  int32_t* d_indices_out = Device(std::vector<int32_t>(indices.size(), -7));
  int64_t* d_report = Device(std::vector<int64_t>{1234567, -99, INT64_MIN, INT64_MAX});
  size_t lwork = 0;
  cuembed::CheckIndices<int32_t, int32_t>(nullptr, nullptr, nnz, d_base, 0, kTables, kBatch, 0, nullptr, nullptr, nullptr,
                                          nullptr, &lwork);
  char* work = Workspace(lwork);
  cuembed::CheckIndices<int32_t, int32_t>(d_indices, d_offsets, nnz, d_base, 0, kTables, kBatch, 0, d_report,
                                          d_indices_out, d_offsets_out, work, &lwork);
  HIP_OK(hipDeviceSynchronize());
  ExpectArray(d_report, std::vector<int64_t>{5, 1, 2, 4}, "group report");
  ExpectArray(d_indices_out, repaired_indices, "group repaired indices");
  ExpectArray(d_offsets_out, repaired_offsets, "group repaired offsets");
  ExpectArray(d_indices, indices, "group indices (input untouched)");
  ExpectArray(d_offsets, offsets, "group offsets (input untouched)");

  // ---- the repaired batch again, in place: clean, whatever the report and the workspace held --------------------------
  HIP_OK(hipMemset(work, 0x5A, lwork > 0 ? lwork : 8));
  cuembed::CheckIndices<int32_t, int32_t>(d_indices_out, d_offsets_out, nnz, d_base, 0, kTables, kBatch, 0, d_report,
                                          d_indices_out, d_offsets_out, work, &lwork);
  HIP_OK(hipDeviceSynchronize());
  ExpectArray(d_report, std::vector<int64_t>{0, -1, 0, -1}, "clean report");
  ExpectArray(d_indices_out, repaired_indices, "clean indices in place");
  ExpectArray(d_offsets_out, repaired_offsets, "clean offsets in place");

  // ---- one table of 7 rows, fixed hotness 2, int64 ids, report only ----------------------------------------------------
  const std::vector<int64_t> wide = {0, 7, 6, -5, INT64_MAX, 1};
  int64_t* d_wide = Device(wide);
  size_t lwork_fixed = 99;
  cuembed::CheckIndices<int64_t, int64_t>(nullptr, nullptr, 6, nullptr, 7, 1, 3, 2, nullptr, nullptr, nullptr, nullptr,
                                          &lwork_fixed);
  ++g_checks;
  if (lwork_fixed != 0) {
    ++g_failures;
    std::fprintf(stderr, "FAILED: fixed hotness asks for %zu workspace bytes, want 0\n", lwork_fixed);
  }
  cuembed::CheckIndices<int64_t, int64_t>(d_wide, nullptr, 6, nullptr, 7, 1, 3, 2, d_report, nullptr, nullptr, work,
                                          &lwork_fixed);
  HIP_OK(hipDeviceSynchronize());
  ExpectArray(d_report, std::vector<int64_t>{3, 1, 0, -1}, "fixed-hotness report");
  ExpectArray(d_wide, wide, "fixed-hotness indices (report only)");
  HIP_OK(hipGetLastError());

  if (g_failures != 0) {
    std::fprintf(stderr, "%d of %d checks FAILED\n", g_failures, g_checks);
    return 1;
  }
  std::printf("index check: %d known-answer checks passed\n", g_checks);
  return 0;
}
