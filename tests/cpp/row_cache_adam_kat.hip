// Header-only API check of the row cache's TWO state planes (row_cache.hpp), of cuembed::TranslateIndicesForRowCachePlanes
// (index_transforms.hpp) and of cuembed::SparseRowAdam with placed moments (sparse_adam.hpp): one prefetch with two
// planes, one translate for the three planes, one placed Adam step, one flush, against a host recomputation.
//
// A table of 200 rows and its two moments live in pinned host memory behind a cache of ONE set (64 slots).  The batch
// names rows 0..69 for update: rows 0..63 are placed (misses in ascending row id), rows 64..69 find no way.  One launch
// translates the ids three ways and one placed step updates the 64 resident rows and their moments in the cache and the
// six others in host memory.  Before the flush the host holds the new values of the six only; after it, of all 70.  The
// host moments differ row by row and from each other, so a fill that did not carry a plane, or carried the wrong one,
// would show.  All data is exact in fp32 (beta1 = beta2 = 1/2, small integers, sqrt of perfect squares, power-of-two
// denominators): bits must be equal.  Built and run by tests/test_gpu_cpp_row_cache_adam.py.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "cuembed/include/row_cache.hpp"
#include "cuembed/include/sparse_adam.hpp"

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
// (second moment before, gradient magnitude): sqrt(v / 2 + g^2 / 2) + eps = 4, 8, 16
constexpr float kSecond[3] = {2.f, 62.f, 446.f};
constexpr float kMagnitude[3] = {4.f, 6.f, 2.f};
//! The first moment of row r before the step: an even integer in [-4, 4] (m / 2 + g / 2 is exact).
inline float FirstOf(const int r) { return static_cast<float>((r % 5) * 2 - 4); }

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
void Case(const cuembed::AdamRule rule, const int width, hipStream_t stream, const char* what) {
  const int second_width = rule == cuembed::AdamRule::kAdam ? width : 1;
  ElemT* table = Pinned<ElemT>(static_cast<size_t>(kRows) * width);
  float* first = Pinned<float>(static_cast<size_t>(kRows) * width);
  float* second = Pinned<float>(static_cast<size_t>(kRows) * second_width);
  std::vector<float> table_f(static_cast<size_t>(kRows) * width), first_f(static_cast<size_t>(kRows) * width),
      second_f(static_cast<size_t>(kRows) * second_width);
  for (int r = 0; r < kRows; ++r) {
    for (int j = 0; j < width; ++j) {
      table_f[r * width + j] = static_cast<float>((r * 5 + j * 3) % 17 - 8);
      first_f[r * width + j] = FirstOf(r + j);
    }
    for (int j = 0; j < second_width; ++j) second_f[r * second_width + j] = kSecond[r % 3];
  }
  for (size_t i = 0; i < table_f.size(); ++i) table[i] = From<ElemT>(table_f[i]);
  std::memcpy(first, first_f.data(), first_f.size() * sizeof(float));
  std::memcpy(second, second_f.data(), second_f.size() * sizeof(float));

  // the batch: entry k names row k; every element of its gradient row is +-magnitude (so the row's mean square is m^2)
  std::vector<IndexT> ids_h(kBatch);
  std::vector<ElemT> grad_h(static_cast<size_t>(kBatch) * width);
  std::vector<float> want_table = table_f, want_first = first_f, want_second = second_f;
  for (int k = 0; k < kBatch; ++k) {
    ids_h[k] = static_cast<IndexT>(k);
    const float mag = kMagnitude[k % 3];
    const float v_new = 0.5f * kSecond[k % 3] + 0.5f * (mag * mag);
    const float denominator = std::sqrt(v_new) + kEps;       // 4, 8 or 16
    for (int j = 0; j < width; ++j) {
      const float g = ((k + j) % 2 ? -1.f : 1.f) * mag;
      grad_h[static_cast<size_t>(k) * width + j] = From<ElemT>(g);
      const float m_new = 0.5f * first_f[k * width + j] + 0.5f * g;
      want_first[k * width + j] = m_new;
      // adam: (lr * c) * m / (sqrt(v) + eps); row-wise: ((lr * c) / (sqrt(v_r) + eps)) * m -- both exact here
      want_table[k * width + j] = ToF(From<ElemT>(table_f[k * width + j] - kLr * m_new / denominator));
    }
    for (int j = 0; j < second_width; ++j) want_second[k * second_width + j] = v_new;
  }

  cuembed::RowCache c;
  c.table = table;
  c.row_bytes = static_cast<int64_t>(width) * sizeof(ElemT);
  c.num_rows = kRows;
  c.num_sets = 1;
  c.state = first;
  c.state_row_bytes = 4 * width;
  c.state2 = second;
  c.state2_row_bytes = 4 * second_width;
  char *raw_rows = nullptr, *raw_first = nullptr, *raw_second = nullptr;
  c.cache_rows = PlaneBehind(table, c.row_bytes, &raw_rows);
  c.state_cache = reinterpret_cast<float*>(PlaneBehind(first, c.state_row_bytes, &raw_first));
  c.state2_cache = reinterpret_cast<float*>(PlaneBehind(second, c.state2_row_bytes, &raw_second));
  c.tags = Device(std::vector<int64_t>(kSlots, -1));
  c.stamps = Device(std::vector<uint32_t>(kSlots, 0));
  c.dirty = Device(std::vector<uint8_t>(kSlots, 0));
  c.slot_of_row = Device(std::vector<int32_t>(kRows, -1));
  std::vector<unsigned long long> words_h(cuembed::kCacheWords, 0);
  words_h[cuembed::kCacheClock] = 1;
  c.words = Device(words_h);
  IndexT* ids = Device(ids_h);
  ElemT* grad = Device(grad_h);
  int64_t* placed_rows = Device(std::vector<int64_t>(kBatch, -7));
  int64_t* placed_first = Device(std::vector<int64_t>(kBatch, -7));
  int64_t* placed_second = Device(std::vector<int64_t>(kBatch, -7));

  // 1. the prefetch with two state planes
  cuembed::RowCacheCounts counts;
  counts.num_valid = kBatch;
  size_t lwork = 0;
  cuembed::RowCachePrefetch<IndexT>(c, ids, kBatch, counts, true, nullptr, &lwork, stream);
  char* work = nullptr;
  HIP_OK(hipMalloc(reinterpret_cast<void**>(&work), lwork ? lwork : 1));
  cuembed::RowCachePrefetch<IndexT>(c, ids, kBatch, counts, true, work, &lwork, stream);
  // 2. one translate for the three planes, one placed step (the count as the prefetch resolved it: one int64 word)
  const int64_t row_offset = (static_cast<char*>(c.cache_rows) - reinterpret_cast<char*>(table)) / c.row_bytes;
  const int64_t first_offset =
      (reinterpret_cast<char*>(c.state_cache) - reinterpret_cast<char*>(first)) / c.state_row_bytes;
  const int64_t second_offset =
      (reinterpret_cast<char*>(c.state2_cache) - reinterpret_cast<char*>(second)) / c.state2_row_bytes;
  cuembed::TranslateIndicesForRowCachePlanes<IndexT>(ids, kBatch, c.slot_of_row, kRows, row_offset, placed_rows,
                                                     first_offset, placed_first, second_offset, placed_second, stream);
  cuembed::SparseAdamOptions o;
  o.rule = rule;
  o.lr = kLr;
  o.bias_factor = 1.f;
  o.beta1 = o.one_minus_beta1 = 0.5f;
  o.beta2 = o.one_minus_beta2 = 0.5f;
  o.eps = kEps;
  o.piece_rows = kBatch;
  o.counts = c.words + cuembed::kCacheBatchCount;
  o.counts_are_int64 = true;
  cuembed::SparseRowAdam<ElemT, int64_t>(table, first, second, width, placed_rows, grad, o, stream, placed_first,
                                         placed_second);
  HIP_OK(hipStreamSynchronize(stream));
  HIP_OK(hipGetLastError());

  // the translate: a resident row's id is its slot behind each plane's offset, a row without a way keeps its id
  std::vector<int64_t> got_rows(kBatch), got_first(kBatch), got_second(kBatch);
  HIP_OK(hipMemcpy(got_rows.data(), placed_rows, kBatch * sizeof(int64_t), hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(got_first.data(), placed_first, kBatch * sizeof(int64_t), hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(got_second.data(), placed_second, kBatch * sizeof(int64_t), hipMemcpyDeviceToHost));
  for (int k = 0; k < kBatch; ++k) {
    const bool resident = k < kSlots;
    Expect(got_rows[k] == (resident ? row_offset + k : k), what, "translated id, table plane", k);
    Expect(got_first[k] == (resident ? first_offset + k : k), what, "translated id, first moment", k);
    Expect(got_second[k] == (resident ? second_offset + k : k), what, "translated id, second moment", k);
  }

  // before the flush: the six rows without a way are updated in host memory, the 64 resident ones are not
  for (int r = 0; r < kRows; ++r) {
    const bool direct = r >= kSlots && r < kBatch;
    for (int j = 0; j < width; ++j) {
      Expect(ToF(table[r * width + j]) == (direct ? want_table : table_f)[r * width + j], what,
             "host table before the flush", r);
      Expect(first[r * width + j] == (direct ? want_first : first_f)[r * width + j], what,
             "host first moment before the flush", r);
    }
    for (int j = 0; j < second_width; ++j)
      Expect(second[r * second_width + j] == (direct ? want_second : second_f)[r * second_width + j], what,
             "host second moment before the flush", r);
  }
  std::vector<float> cached_first(static_cast<size_t>(kSlots) * width), cached_second(static_cast<size_t>(kSlots) * second_width);
  HIP_OK(hipMemcpy(cached_first.data(), c.state_cache, cached_first.size() * sizeof(float), hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(cached_second.data(), c.state2_cache, cached_second.size() * sizeof(float), hipMemcpyDeviceToHost));
  std::vector<int64_t> tags(kSlots);
  HIP_OK(hipMemcpy(tags.data(), c.tags, kSlots * sizeof(int64_t), hipMemcpyDeviceToHost));
  for (int s = 0; s < kSlots; ++s) {
    Expect(tags[s] == s, what, "rows 0..63 take ways 0..63 in order", s);
    for (int j = 0; j < width; ++j)
      Expect(cached_first[s * width + j] == want_first[s * width + j], what, "cached first moment after the step", s);
    for (int j = 0; j < second_width; ++j)
      Expect(cached_second[s * second_width + j] == want_second[s * second_width + j], what,
             "cached second moment after the step", s);
  }

  // 3. the flush
  cuembed::RowCacheFlush(c, stream);
  HIP_OK(hipStreamSynchronize(stream));
  HIP_OK(hipGetLastError());
  for (size_t i = 0; i < want_table.size(); ++i) {
    Expect(ToF(table[i]) == want_table[i], what, "host table after the flush", static_cast<long>(i / width));
    Expect(first[i] == want_first[i], what, "host first moment after the flush", static_cast<long>(i / width));
  }
  for (size_t i = 0; i < want_second.size(); ++i)
    Expect(second[i] == want_second[i], what, "host second moment after the flush", static_cast<long>(i / second_width));
  HIP_OK(hipMemcpy(words_h.data(), c.words, words_h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  Expect(words_h[cuembed::kCacheHits] == 0 && words_h[cuembed::kCacheMisses] == kBatch, what, "hits / misses");
  Expect(words_h[cuembed::kCacheUnplaced] == kBatch - kSlots, what, "unplaced");
  Expect(words_h[cuembed::kCacheWriteBacks] == kSlots, what, "write-backs count rows, not planes");
  Expect(words_h[cuembed::kCacheOverflow] == 0 && words_h[cuembed::kCacheClock] == 2, what, "overflow / clock");
  std::vector<uint8_t> dirty(kSlots);
  HIP_OK(hipMemcpy(dirty.data(), c.dirty, kSlots, hipMemcpyDeviceToHost));
  for (int s = 0; s < kSlots; ++s) Expect(dirty[s] == 0, what, "dirty bytes after the flush", s);

  for (void* p : {static_cast<void*>(raw_rows), static_cast<void*>(raw_first), static_cast<void*>(raw_second),
                  static_cast<void*>(c.tags), static_cast<void*>(c.stamps), static_cast<void*>(c.dirty),
                  static_cast<void*>(c.slot_of_row), static_cast<void*>(c.words), static_cast<void*>(ids),
                  static_cast<void*>(grad), static_cast<void*>(placed_rows), static_cast<void*>(placed_first),
                  static_cast<void*>(placed_second), static_cast<void*>(work)})
    HIP_OK(hipFree(p));
  HIP_OK(hipHostFree(table));
  HIP_OK(hipHostFree(first));
  HIP_OK(hipHostFree(second));
}

int main() {
  hipStream_t stream;
  HIP_OK(hipStreamCreate(&stream));
  using cuembed::AdamRule;
  Case<__half, int32_t>(AdamRule::kRowwiseAdam, 8, stream, "row-wise Adam, fp16 x 8, int32");
  Case<__half, int32_t>(AdamRule::kAdam, 8, stream, "Adam, fp16 x 8, int32");
  Case<float, int64_t>(AdamRule::kRowwiseAdam, 6, stream, "row-wise Adam, fp32 x 6, int64");
  Case<float, int64_t>(AdamRule::kAdam, 6, stream, "Adam, fp32 x 6, int64");
  HIP_OK(hipStreamDestroy(stream));
  if (g_failures) {
    std::fprintf(stderr, "%d of %d checks FAILED\n", g_failures, g_checks);
    return 1;
  }
  std::printf("row cache Adam planes: %d known-answer checks passed\n", g_checks);
  return 0;
}
