// Header-only API check of the row cache's state plane (row_cache.hpp) and of cuembed::SparseRowUpdate with state_ids
// (sparse_update.hpp): one prefetch with a state plane, one placed update, one flush, against a host recomputation.
//
// A table of 200 rows and its optimizer state live in pinned host memory behind a cache of ONE set (64 slots).  The batch
// names rows 0..69 for update: rows 0..63 are placed (misses in ascending row id), rows 64..69 find no way.  The ids are
// translated once per plane and one placed step updates the 64 resident rows and their state in the cache and the six
// others in host memory.  Before the flush the host holds the new values of the six only; after it, of all 70.  The
// host state starts at values that differ row by row, so a fill that did not carry the state would show.  All data is
// exact in fp32 (small integers, sqrt of perfect squares, power-of-two denominators): bits must be equal.
// Built and run by tests/test_gpu_cpp_row_cache_state.py.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

constexpr int kRows = 200;
constexpr int kSlots = cuembed::kRowCacheWays;   // one set
constexpr int kBatch = 70;
constexpr float kLr = 0.75f;
constexpr float kEps = 1.0f;
// (state before, gradient magnitude): sqrt(before + m^2) + eps = 4, 8, 16
constexpr float kBefore[3] = {8.f, 40.f, 216.f};
constexpr float kMagnitude[3] = {1.f, 3.f, 3.f};

template <typename T>
T* Pinned(const size_t n) {
  T* p = nullptr;
  HIP_OK(hipHostMalloc(reinterpret_cast<void**>(&p), n * sizeof(T), hipHostMallocDefault));
  return p;
}

template <typename T>
T* Device(const std::vector<T>& h) {
  T* p = nullptr;
  HIP_OK(hipMalloc(reinterpret_cast<void**>(&p), h.size() * sizeof(T)));
  HIP_OK(hipMemcpy(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
  return p;
}

//! `slots` rows of row_bytes in HBM, a whole number of rows away from `home` (one row over-allocated).
static char* PlaneBehind(const void* home, const int64_t row_bytes, char** raw) {
  HIP_OK(hipMalloc(reinterpret_cast<void**>(raw), static_cast<size_t>((kSlots + 1) * row_bytes)));
  const intptr_t gap = reinterpret_cast<intptr_t>(home) - reinterpret_cast<intptr_t>(*raw);
  const int64_t shift = ((gap % row_bytes) + row_bytes) % row_bytes;
  return *raw + shift;
}

template <typename ElemT, typename IndexT>
void Case(const cuembed::UpdateRule rule, const int width, hipStream_t stream, const char* what) {
  const bool per_element = rule == cuembed::UpdateRule::kAdagrad;
  const int state_width = per_element ? width : 1;
  ElemT* table = Pinned<ElemT>(static_cast<size_t>(kRows) * width);
  float* state = Pinned<float>(static_cast<size_t>(kRows) * state_width);
  std::vector<float> table_f(static_cast<size_t>(kRows) * width), state_f(static_cast<size_t>(kRows) * state_width);
  for (int r = 0; r < kRows; ++r) {
    for (int j = 0; j < width; ++j) table_f[r * width + j] = static_cast<float>((r * 5 + j * 3) % 17 - 8);
    for (int j = 0; j < state_width; ++j) state_f[r * state_width + j] = kBefore[r % 3];
  }
  for (size_t i = 0; i < table_f.size(); ++i) table[i] = From<ElemT>(table_f[i]);
  std::memcpy(state, state_f.data(), state_f.size() * sizeof(float));

  // the batch: entry k names row k; every element of its gradient row is +-magnitude (so the row's mean square is m^2)
  std::vector<IndexT> ids_h(kBatch);
  std::vector<ElemT> grad_h(static_cast<size_t>(kBatch) * width);
  std::vector<float> want_table = table_f, want_state = state_f;
  for (int k = 0; k < kBatch; ++k) {
    ids_h[k] = static_cast<IndexT>(k);
    const float m = kMagnitude[k % 3];
    const float after = kBefore[k % 3] + m * m;
    for (int j = 0; j < width; ++j) {
      const float g = ((k + j) % 2 ? -1.f : 1.f) * m;
      grad_h[static_cast<size_t>(k) * width + j] = From<ElemT>(g);
      const float d = kLr * g / (std::sqrt(after) + kEps);
      want_table[k * width + j] = ToF(From<ElemT>(table_f[k * width + j] - d));   // the one rounding to ElemT
    }
    for (int j = 0; j < state_width; ++j) want_state[k * state_width + j] = after;
  }

  cuembed::RowCache c;
  c.table = table;
  c.row_bytes = static_cast<int64_t>(width) * sizeof(ElemT);
  c.num_rows = kRows;
  c.num_sets = 1;
  c.state = state;
  c.state_row_bytes = 4 * state_width;
  char *raw_rows = nullptr, *raw_state = nullptr;
  c.cache_rows = PlaneBehind(table, c.row_bytes, &raw_rows);
  c.state_cache = reinterpret_cast<float*>(PlaneBehind(state, c.state_row_bytes, &raw_state));
  c.tags = Device(std::vector<int64_t>(kSlots, -1));
  c.stamps = Device(std::vector<uint32_t>(kSlots, 0));
  c.dirty = Device(std::vector<uint8_t>(kSlots, 0));
  c.slot_of_row = Device(std::vector<int32_t>(kRows, -1));
  std::vector<unsigned long long> words_h(cuembed::kCacheWords, 0);
  words_h[cuembed::kCacheClock] = 1;
  c.words = Device(words_h);
  IndexT* ids = Device(ids_h);
  ElemT* grad = Device(grad_h);
  int64_t* placed_rows = Device(std::vector<int64_t>(kBatch, 0));
  int64_t* placed_state = Device(std::vector<int64_t>(kBatch, 0));

  // 1. the prefetch with a state plane
  cuembed::RowCacheCounts counts;
  counts.num_valid = kBatch;
  size_t lwork = 0;
  cuembed::RowCachePrefetch<IndexT>(c, ids, kBatch, counts, true, nullptr, &lwork, stream);
  char* work = nullptr;
  HIP_OK(hipMalloc(reinterpret_cast<void**>(&work), lwork ? lwork : 1));
  cuembed::RowCachePrefetch<IndexT>(c, ids, kBatch, counts, true, work, &lwork, stream);
  // 2. one translate per plane, one placed update (the count as the prefetch resolved it: one int64 word)
  const int64_t row_offset = (static_cast<char*>(c.cache_rows) - reinterpret_cast<char*>(table)) / c.row_bytes;
  const int64_t state_offset =
      (reinterpret_cast<char*>(c.state_cache) - reinterpret_cast<char*>(state)) / c.state_row_bytes;
  cuembed::TranslateIndicesForRowCache<IndexT>(ids, kBatch, c.slot_of_row, kRows, row_offset, placed_rows, stream);
  cuembed::TranslateIndicesForRowCache<IndexT>(ids, kBatch, c.slot_of_row, kRows, state_offset, placed_state, stream);
  cuembed::SparseUpdateOptions o;
  o.rule = rule;
  o.lr = kLr;
  o.eps = kEps;
  o.piece_rows = kBatch;
  o.counts = c.words + cuembed::kCacheBatchCount;
  o.counts_are_int64 = true;
  cuembed::SparseRowUpdate<ElemT, int64_t>(table, state, width, placed_rows, grad, o, stream, placed_state);
  HIP_OK(hipStreamSynchronize(stream));
  HIP_OK(hipGetLastError());

  // before the flush: the six rows without a way are updated in host memory, the 64 resident ones are not
  for (int r = 0; r < kRows; ++r) {
    const bool direct = r >= kSlots && r < kBatch;
    for (int j = 0; j < width; ++j) {
      const float want = direct ? want_table[r * width + j] : table_f[r * width + j];
      Expect(ToF(table[r * width + j]) == want, what, "host table before the flush", r);
    }
    for (int j = 0; j < state_width; ++j) {
      const float want = direct ? want_state[r * state_width + j] : state_f[r * state_width + j];
      Expect(state[r * state_width + j] == want, what, "host state before the flush", r);
    }
  }
  std::vector<float> cached_state(static_cast<size_t>(kSlots) * state_width);
  HIP_OK(hipMemcpy(cached_state.data(), c.state_cache, cached_state.size() * sizeof(float), hipMemcpyDeviceToHost));
  std::vector<int64_t> tags(kSlots);
  HIP_OK(hipMemcpy(tags.data(), c.tags, kSlots * sizeof(int64_t), hipMemcpyDeviceToHost));
  for (int s = 0; s < kSlots; ++s) {
    Expect(tags[s] == s, what, "rows 0..63 take ways 0..63 in order", s);
    for (int j = 0; j < state_width; ++j)
      Expect(cached_state[s * state_width + j] == want_state[s * state_width + j], what, "cached state after the step", s);
  }

  // 3. the flush
  cuembed::RowCacheFlush(c, stream);
  HIP_OK(hipStreamSynchronize(stream));
  HIP_OK(hipGetLastError());
  for (size_t i = 0; i < want_table.size(); ++i)
    Expect(ToF(table[i]) == want_table[i], what, "host table after the flush", static_cast<long>(i / width));
  for (size_t i = 0; i < want_state.size(); ++i)
    Expect(state[i] == want_state[i], what, "host state after the flush", static_cast<long>(i / state_width));
  HIP_OK(hipMemcpy(words_h.data(), c.words, words_h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  Expect(words_h[cuembed::kCacheHits] == 0 && words_h[cuembed::kCacheMisses] == kBatch, what, "hits / misses");
  Expect(words_h[cuembed::kCacheUnplaced] == kBatch - kSlots, what, "unplaced");
  Expect(words_h[cuembed::kCacheWriteBacks] == kSlots, what, "write-backs count rows, not planes");
  Expect(words_h[cuembed::kCacheOverflow] == 0 && words_h[cuembed::kCacheClock] == 2, what, "overflow / clock");
  std::vector<uint8_t> dirty(kSlots);
  HIP_OK(hipMemcpy(dirty.data(), c.dirty, kSlots, hipMemcpyDeviceToHost));
  for (int s = 0; s < kSlots; ++s) Expect(dirty[s] == 0, what, "dirty bytes after the flush", s);

  for (void* p : {static_cast<void*>(raw_rows), static_cast<void*>(raw_state), static_cast<void*>(c.tags),
                  static_cast<void*>(c.stamps), static_cast<void*>(c.dirty), static_cast<void*>(c.slot_of_row),
                  static_cast<void*>(c.words), static_cast<void*>(ids), static_cast<void*>(grad),
                  static_cast<void*>(placed_rows), static_cast<void*>(placed_state), static_cast<void*>(work)})
    HIP_OK(hipFree(p));
  HIP_OK(hipHostFree(table));
  HIP_OK(hipHostFree(state));
}

int main() {
  hipStream_t stream;
  HIP_OK(hipStreamCreate(&stream));
  using cuembed::UpdateRule;
  Case<__half, int32_t>(UpdateRule::kRowwiseAdagrad, 8, stream, "row-wise Adagrad, fp16 x 8, int32");
  Case<__half, int32_t>(UpdateRule::kAdagrad, 8, stream, "Adagrad, fp16 x 8, int32");
  Case<float, int64_t>(UpdateRule::kRowwiseAdagrad, 6, stream, "row-wise Adagrad, fp32 x 6, int64");
  Case<float, int64_t>(UpdateRule::kAdagrad, 6, stream, "Adagrad, fp32 x 6, int64");
  HIP_OK(hipStreamDestroy(stream));
  if (g_failures) {
    std::fprintf(stderr, "%d of %d checks FAILED\n", g_failures, g_checks);
    return 1;
  }
  std::printf("row cache state plane: %d known-answer checks passed\n", g_checks);
  return 0;
}
