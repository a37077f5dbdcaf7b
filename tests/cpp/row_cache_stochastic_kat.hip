// Header-only API check of STOCHASTIC ROUNDING THROUGH THE ROW CACHE: cuembed::SparseRowUpdate / cuembed::SparseRowAdam
// with row_names (sparse_update.hpp, sparse_adam.hpp) behind the planes of row_cache.hpp -- one prefetch, one translate,
// one named step, one flush, against a host recomputation that uses stochastic_rounding.hpp's own host functions with
// the TABLE ROW as the name.
//
// A table of 200 rows and its state live in pinned host memory behind a cache of ONE set (64 slots).  The batch names
// rows 100..169 for update: rows 100..163 take ways 0..63 (misses in ascending row id), rows 164..169 find no way and
// are updated in host memory.  No row sits in the slot of its own number, so bits drawn for the slot, or for a
// translated id, are another row's and give another table.  Row-wise Adagrad has one state plane, lazy Adam two.
// The fp32 values are exact (small integers, sqrt of perfect squares, power-of-two denominators) but carry more bits
// than the 16-bit types hold (the update is a multiple of 3 * 2^-12 on weights of magnitude up to 8), so every store
// really rounds.  Built and run by tests/test_gpu_cpp_row_cache_stochastic.py.
#include <hip/hip_bf16.h>
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
template <> __half From<__half>(float v) { return __float2half(v); }
template <> __hip_bfloat16 From<__hip_bfloat16>(float v) { return __float2bfloat16(v); }
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

static void Expect(const bool ok, const char* what, const char* detail, const long at = -1) {
  ++g_checks;
  if (ok) return;
  ++g_failures;
  std::fprintf(stderr, "FAILED %s: %s (at %ld)\n", what, detail, at);
}

constexpr int kRows = 200;
constexpr int kSlots = cuembed::kRowCacheWays;   // one set
constexpr int kBatch = 70;
constexpr int kFirstRow = 100;                   // entry k names row 100 + k
constexpr float kLr = 0.75f / 64.f;
constexpr float kEps = 1.0f;
constexpr uint64_t kSeed = 0x9E3779B97F4A7C15ull;
constexpr uint64_t kStep = 0x100000005ull;       // (the high word goes into the key)
// (second moment before, gradient magnitude): sqrt(v / 2 + g^2 / 2) + eps = 4, 8, 16
constexpr float kSecond[3] = {2.f, 62.f, 446.f};
constexpr float kMagnitude[3] = {4.f, 6.f, 2.f};
// (row-wise Adagrad's accumulator before): sqrt(s + g^2) + eps = 8, 8, 16 for the same magnitudes
constexpr float kAccumulator[3] = {33.f, 13.f, 221.f};
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

//! The stochastic rounding of x for (table row, column), as the specification's host functions give it.
template <typename ElemT>
uint16_t Rounded(const float x, const int row, const int column) {
  const cuembed::detail::PhiloxWords p = cuembed::detail::RoundingWords(kSeed, kStep, static_cast<uint64_t>(row), column / 8);
  return RoundBits(ElemT(), x, cuembed::detail::RoundingField(p, column % 8));
}

//! adam: lazy Adam with two state planes; otherwise row-wise Adagrad with one.
template <typename ElemT, typename IndexT>
void Case(const bool adam, const int width, hipStream_t stream, const char* what) {
  ElemT* table = Pinned<ElemT>(static_cast<size_t>(kRows) * width);
  const int first_width = adam ? width : 1;     // (row-wise Adagrad: `first` holds the row words)
  float* first = Pinned<float>(static_cast<size_t>(kRows) * first_width);
  float* second = adam ? Pinned<float>(static_cast<size_t>(kRows) * width) : nullptr;
  std::vector<float> table_f(static_cast<size_t>(kRows) * width), first_f(static_cast<size_t>(kRows) * first_width),
      second_f(adam ? static_cast<size_t>(kRows) * width : 0);
  for (int r = 0; r < kRows; ++r) {
    for (int j = 0; j < width; ++j) {
      table_f[r * width + j] = static_cast<float>((r * 5 + j * 3) % 17 - 8);
      if (adam) first_f[r * width + j] = FirstOf(r + j), second_f[r * width + j] = kSecond[r % 3];
    }
    if (!adam) first_f[r] = kAccumulator[r % 3];
  }
  for (size_t i = 0; i < table_f.size(); ++i) table[i] = From<ElemT>(table_f[i]);
  std::memcpy(first, first_f.data(), first_f.size() * sizeof(float));
  if (adam) std::memcpy(second, second_f.data(), second_f.size() * sizeof(float));

  // the batch: entry k names row 100 + k; every element of its gradient row is +-magnitude
  std::vector<IndexT> ids_h(kBatch);
  std::vector<int64_t> names_h(kBatch);
  std::vector<ElemT> grad_h(static_cast<size_t>(kBatch) * width);
  std::vector<uint16_t> want_table(table_f.size()), nearest_table(table_f.size());
  for (size_t i = 0; i < table_f.size(); ++i) want_table[i] = nearest_table[i] = Bits(From<ElemT>(table_f[i]));
  std::vector<float> want_first = first_f, want_second = second_f;
  for (int k = 0; k < kBatch; ++k) {
    const int r = kFirstRow + k;
    ids_h[k] = static_cast<IndexT>(r);
    names_h[k] = r;
    const float mag = kMagnitude[r % 3];
    const float second_new = adam ? 0.5f * kSecond[r % 3] + 0.5f * (mag * mag) : kAccumulator[r % 3] + mag * mag;
    const float denominator = std::sqrt(second_new) + kEps;       // 4, 8 or 16
    for (int j = 0; j < width; ++j) {
      const float g = ((k + j) % 2 ? -1.f : 1.f) * mag;
      grad_h[static_cast<size_t>(k) * width + j] = From<ElemT>(g);
      float x;
      if (adam) {
        const float m_new = 0.5f * first_f[r * width + j] + 0.5f * g;
        want_first[r * width + j] = m_new;
        want_second[r * width + j] = second_new;
        x = table_f[r * width + j] - kLr * m_new / denominator;
      } else {
        x = table_f[r * width + j] - (kLr / denominator) * g;
      }
      want_table[r * width + j] = Rounded<ElemT>(x, r, j);
      nearest_table[r * width + j] = Bits(From<ElemT>(x));
    }
    if (!adam) want_first[r] = second_new;
  }
  size_t differ = 0;
  for (size_t i = 0; i < want_table.size(); ++i) differ += want_table[i] != nearest_table[i];
  Expect(differ * 8 >= static_cast<size_t>(kBatch) * width, what, "the data: stochastic and nearest differ often");

  cuembed::RowCache c;
  c.table = table;
  c.row_bytes = static_cast<int64_t>(width) * sizeof(ElemT);
  c.num_rows = kRows;
  c.num_sets = 1;
  c.state = first;
  c.state_row_bytes = 4 * first_width;
  char *raw_rows = nullptr, *raw_first = nullptr, *raw_second = nullptr;
  c.cache_rows = PlaneBehind(table, c.row_bytes, &raw_rows);
  c.state_cache = reinterpret_cast<float*>(PlaneBehind(first, c.state_row_bytes, &raw_first));
  if (adam) {
    c.state2 = second;
    c.state2_row_bytes = 4 * width;
    c.state2_cache = reinterpret_cast<float*>(PlaneBehind(second, c.state2_row_bytes, &raw_second));
  }
  c.tags = Device(std::vector<int64_t>(kSlots, -1));
  c.stamps = Device(std::vector<uint32_t>(kSlots, 0));
  c.dirty = Device(std::vector<uint8_t>(kSlots, 0));
  c.slot_of_row = Device(std::vector<int32_t>(kRows, -1));
  std::vector<unsigned long long> words_h(cuembed::kCacheWords, 0);
  words_h[cuembed::kCacheClock] = 1;
  c.words = Device(words_h);
  IndexT* ids = Device(ids_h);
  int64_t* names = Device(names_h);
  ElemT* grad = Device(grad_h);
  int64_t* step_word = Device(std::vector<int64_t>{static_cast<int64_t>(kStep)});
  int64_t* placed_rows = Device(std::vector<int64_t>(kBatch, -7));
  int64_t* placed_first = Device(std::vector<int64_t>(kBatch, -7));
  int64_t* placed_second = Device(std::vector<int64_t>(kBatch, -7));

  // 1. the prefetch
  cuembed::RowCacheCounts counts;
  counts.num_valid = kBatch;
  size_t lwork = 0;
  cuembed::RowCachePrefetch<IndexT>(c, ids, kBatch, counts, true, nullptr, &lwork, stream);
  char* work = nullptr;
  HIP_OK(hipMalloc(reinterpret_cast<void**>(&work), lwork ? lwork : 1));
  cuembed::RowCachePrefetch<IndexT>(c, ids, kBatch, counts, true, work, &lwork, stream);
  // 2. one translate for the planes, one named step (the count as the prefetch resolved it; the step in a device word)
  const int64_t row_offset = (static_cast<char*>(c.cache_rows) - reinterpret_cast<char*>(table)) / c.row_bytes;
  const int64_t first_offset =
      (reinterpret_cast<char*>(c.state_cache) - reinterpret_cast<char*>(first)) / c.state_row_bytes;
  const int64_t second_offset =
      adam ? (reinterpret_cast<char*>(c.state2_cache) - reinterpret_cast<char*>(second)) / c.state2_row_bytes : 0;
  cuembed::TranslateIndicesForRowCachePlanes<IndexT>(ids, kBatch, c.slot_of_row, kRows, row_offset, placed_rows,
                                                     first_offset, placed_first, second_offset,
                                                     adam ? placed_second : nullptr, stream);
  if (adam) {
    cuembed::SparseAdamOptions o;
    o.rule = cuembed::AdamRule::kAdam;
    o.lr = kLr;
    o.bias_factor = 1.f;
    o.beta1 = o.one_minus_beta1 = 0.5f;
    o.beta2 = o.one_minus_beta2 = 0.5f;
    o.eps = kEps;
    o.piece_rows = kBatch;
    o.counts = c.words + cuembed::kCacheBatchCount;
    o.counts_are_int64 = true;
    o.stochastic_rounding = true;
    o.rounding_seed = kSeed;
    o.rounding_step = 77;   // (ignored: the device word holds the step)
    o.rounding_step_device = step_word;
    cuembed::SparseRowAdam<ElemT, int64_t>(table, first, second, width, placed_rows, grad, o, stream, placed_first,
                                           placed_second, names);
  } else {
    cuembed::SparseUpdateOptions o;
    o.rule = cuembed::UpdateRule::kRowwiseAdagrad;
    o.lr = kLr;
    o.eps = kEps;
    o.piece_rows = kBatch;
    o.counts = c.words + cuembed::kCacheBatchCount;
    o.counts_are_int64 = true;
    o.stochastic_rounding = true;
    o.rounding_seed = kSeed;
    o.rounding_step = 77;
    o.rounding_step_device = step_word;
    cuembed::SparseRowUpdate<ElemT, int64_t>(table, first, width, placed_rows, grad, o, stream, placed_first, names);
  }
  HIP_OK(hipStreamSynchronize(stream));
  HIP_OK(hipGetLastError());

  // no resident row sits in the slot of its own number, or is named by its translated id
  std::vector<int64_t> got_rows(kBatch);
  HIP_OK(hipMemcpy(got_rows.data(), placed_rows, kBatch * sizeof(int64_t), hipMemcpyDeviceToHost));
  for (int k = 0; k < kBatch; ++k) {
    const bool resident = k < kSlots;
    Expect(got_rows[k] == (resident ? row_offset + k : kFirstRow + k), what, "translated id, table plane", k);
    Expect(!resident || got_rows[k] != names_h[k], what, "a resident row's name is not its placed id", k);
  }
  // before the flush: the six rows without a way are updated in host memory, with their own bits
  for (int r = 0; r < kRows; ++r) {
    const bool direct = r >= kFirstRow + kSlots && r < kFirstRow + kBatch;
    for (int j = 0; j < width; ++j)
      Expect(Bits(table[r * width + j]) == (direct ? want_table[r * width + j] : Bits(From<ElemT>(table_f[r * width + j]))),
             what, "host table before the flush", r);
  }

  // 3. the flush
  cuembed::RowCacheFlush(c, stream);
  HIP_OK(hipStreamSynchronize(stream));
  HIP_OK(hipGetLastError());
  for (size_t i = 0; i < want_table.size(); ++i)
    Expect(Bits(table[i]) == want_table[i], what, "host table after the flush", static_cast<long>(i / width));
  for (size_t i = 0; i < want_first.size(); ++i)
    Expect(first[i] == want_first[i], what, "first state plane after the flush", static_cast<long>(i / first_width));
  for (size_t i = 0; i < want_second.size(); ++i)
    Expect(second[i] == want_second[i], what, "second state plane after the flush", static_cast<long>(i / width));
  HIP_OK(hipMemcpy(words_h.data(), c.words, words_h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  Expect(words_h[cuembed::kCacheMisses] == kBatch && words_h[cuembed::kCacheUnplaced] == kBatch - kSlots, what,
         "misses / unplaced");
  Expect(words_h[cuembed::kCacheWriteBacks] == kSlots && words_h[cuembed::kCacheOverflow] == 0, what,
         "write-backs / overflow");

  for (void* p : {static_cast<void*>(raw_rows), static_cast<void*>(raw_first), static_cast<void*>(raw_second),
                  static_cast<void*>(c.tags), static_cast<void*>(c.stamps), static_cast<void*>(c.dirty),
                  static_cast<void*>(c.slot_of_row), static_cast<void*>(c.words), static_cast<void*>(ids),
                  static_cast<void*>(names), static_cast<void*>(grad), static_cast<void*>(step_word),
                  static_cast<void*>(placed_rows), static_cast<void*>(placed_first), static_cast<void*>(placed_second),
                  static_cast<void*>(work)})
    if (p != nullptr) HIP_OK(hipFree(p));
  HIP_OK(hipHostFree(table));
  HIP_OK(hipHostFree(first));
  if (second != nullptr) HIP_OK(hipHostFree(second));
}

int main() {
  hipStream_t stream;
  HIP_OK(hipStreamCreate(&stream));
  // 8: one 16-byte lane per row; 40: five lanes in a group of eight, two entries in flight
  for (const int width : {8, 40}) {
    Case<__half, int32_t>(false, width, stream, "row-wise Adagrad, fp16, int32");
    Case<__half, int32_t>(true, width, stream, "lazy Adam, fp16, int32");
    Case<__hip_bfloat16, int64_t>(false, width, stream, "row-wise Adagrad, bf16, int64");
    Case<__hip_bfloat16, int64_t>(true, width, stream, "lazy Adam, bf16, int64");
  }
  HIP_OK(hipStreamDestroy(stream));
  if (g_failures) {
    std::fprintf(stderr, "%d of %d checks FAILED\n", g_failures, g_checks);
    return 1;
  }
  std::printf("row cache stochastic rounding: %d known-answer checks passed\n", g_checks);
  return 0;
}
