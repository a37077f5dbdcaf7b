// What the row cache's known-answer programs (row_cache_state_kat.hip, row_cache_adam_kat.hip, row_cache_stochastic_kat.hip)
// share: the error and check macros, conversions to the table's type, pinned and device buffers, and the cache of ONE set
// (64 slots) with zero to two state planes that every case builds behind its pinned table.  Each program keeps its own
// cases and its own expected values.
#ifndef CUEMBED_TESTS_CPP_ROW_CACHE_KAT_COMMON_HPP_
#define CUEMBED_TESTS_CPP_ROW_CACHE_KAT_COMMON_HPP_

#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "cuembed/include/row_cache.hpp"

#define HIP_OK(x)                                                              \
  do {                                                                         \
    hipError_t e_ = (x);                                                       \
    if (e_ != hipSuccess) {                                                    \
      std::fprintf(stderr, "%s failed: %s\n", #x, hipGetErrorString(e_));      \
      std::exit(2);                                                            \
    }                                                                          \
  } while (0)

template <typename T> T From(float v);
template <> inline float From<float>(float v) { return v; }
template <> inline __half From<__half>(float v) { return __float2half(v); }
template <> inline __hip_bfloat16 From<__hip_bfloat16>(float v) { return __float2bfloat16(v); }
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

//! The last line of a program: the count of failures to stderr and 1, or `title` with the count of checks and 0.
inline int Report(const char* title) {
  if (g_failures) {
    std::fprintf(stderr, "%d of %d checks FAILED\n", g_failures, g_checks);
    return 1;
  }
  std::printf("%s: %d known-answer checks passed\n", title, g_checks);
  return 0;
}

constexpr int kSlots = cuembed::kRowCacheWays;   // one set

static std::vector<void*> g_device;   // what a case allocated on the device, until FreeDevice()

inline char* DeviceBytes(const size_t bytes) {
  char* p = nullptr;
  HIP_OK(hipMalloc(reinterpret_cast<void**>(&p), bytes ? bytes : 1));
  g_device.push_back(p);
  return p;
}

inline void FreeDevice() {
  for (void* p : g_device) HIP_OK(hipFree(p));
  g_device.clear();
}

template <typename T>
T* Pinned(const size_t n) {
  T* p = nullptr;
  HIP_OK(hipHostMalloc(reinterpret_cast<void**>(&p), n * sizeof(T), hipHostMallocDefault));
  return p;
}

template <typename T>
T* Device(const std::vector<T>& h) {
  T* p = reinterpret_cast<T*>(DeviceBytes(h.size() * sizeof(T)));
  HIP_OK(hipMemcpy(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
  return p;
}

template <typename T>
std::vector<T> Host(const T* device, const size_t n) {
  std::vector<T> h(n);
  HIP_OK(hipMemcpy(h.data(), device, n * sizeof(T), hipMemcpyDeviceToHost));
  return h;
}

//! kSlots rows of row_bytes in HBM, a whole number of rows away from `home` (one row over-allocated).
inline char* PlaneBehind(const void* home, const int64_t row_bytes) {
  char* raw = DeviceBytes(static_cast<size_t>((kSlots + 1) * row_bytes));
  const intptr_t gap = reinterpret_cast<intptr_t>(home) - reinterpret_cast<intptr_t>(raw);
  return raw + ((gap % row_bytes) + row_bytes) % row_bytes;
}

//! How many of its rows a plane's slots lie behind its home tensor: what a translate adds to a slot.
inline int64_t PlaneOffset(const void* home, const void* cached, const int64_t row_bytes) {
  return (static_cast<const char*>(cached) - static_cast<const char*>(home)) / row_bytes;
}

//! An empty cache of one set behind `table`, with the state planes whose row size is not 0 (device memory: FreeDevice()).
inline cuembed::RowCache OneSetCache(void* table, const int64_t row_bytes, const int64_t num_rows, float* state = nullptr,
                                     const int64_t state_row_bytes = 0, float* state2 = nullptr,
                                     const int64_t state2_row_bytes = 0) {
  cuembed::RowCache c;
  c.table = table;
  c.row_bytes = row_bytes;
  c.num_rows = num_rows;
  c.num_sets = 1;
  c.cache_rows = PlaneBehind(table, row_bytes);
  if (state_row_bytes != 0) {
    c.state = state;
    c.state_row_bytes = state_row_bytes;
    c.state_cache = reinterpret_cast<float*>(PlaneBehind(state, state_row_bytes));
  }
  if (state2_row_bytes != 0) {
    c.state2 = state2;
    c.state2_row_bytes = state2_row_bytes;
    c.state2_cache = reinterpret_cast<float*>(PlaneBehind(state2, state2_row_bytes));
  }
  c.tags = Device(std::vector<int64_t>(kSlots, -1));
  c.stamps = Device(std::vector<uint32_t>(kSlots, 0));
  c.dirty = Device(std::vector<uint8_t>(kSlots, 0));
  c.slot_of_row = Device(std::vector<int32_t>(static_cast<size_t>(num_rows), -1));
  std::vector<unsigned long long> words(cuembed::kCacheWords, 0);
  words[cuembed::kCacheClock] = 1;
  c.words = Device(words);
  return c;
}

//! One prefetch for update of all `n` ids: the workspace query, the workspace, the run.
template <typename IndexT>
void PrefetchForUpdate(const cuembed::RowCache& c, const IndexT* ids, const int n, hipStream_t stream) {
  cuembed::RowCacheCounts counts;
  counts.num_valid = n;
  size_t lwork = 0;
  cuembed::RowCachePrefetch<IndexT>(c, ids, n, counts, true, nullptr, &lwork, stream);
  cuembed::RowCachePrefetch<IndexT>(c, ids, n, counts, true, DeviceBytes(lwork), &lwork, stream);
}

#endif  // CUEMBED_TESTS_CPP_ROW_CACHE_KAT_COMMON_HPP_
