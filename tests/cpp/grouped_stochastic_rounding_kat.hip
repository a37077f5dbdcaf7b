// Stochastic rounding in the grouped optimizer step through the HEADER-ONLY API: cuembed::SparseRowUpdateGrouped (SGD)
// and cuembed::SparseRowAdamGrouped (row-wise Adam) with options.stochastic_rounding and ONE SEED PER TABLE on a group of
// three separate tables with 1, 5 and 70 rows, against a host recomputation that calls stochastic_rounding.hpp's own host
// functions with (seeds[t], step, row INSIDE table t, column).  The data are exactly representable and every fp32 step of
// the rules is exact on them, so the host's value is the kernel's whatever the host compiler contracts; what is checked is
// the naming of the bits.  SGD takes the step as an immediate, row-wise Adam from a device word.  Rows that no entry
// names, and entries past the count, must leave no trace.
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "cuembed/include/grouped_sparse_update.hpp"

#define HIP_OK(call)                                                                              \
  do {                                                                                            \
    const hipError_t e_ = (call);                                                                 \
    if (e_ != hipSuccess) {                                                                       \
      std::fprintf(stderr, "%s failed: %s (%s:%d)\n", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
      std::exit(2);                                                                               \
    }                                                                                             \
  } while (0)

namespace {

constexpr int kTables = 3;
const int64_t kRows[kTables] = {1, 5, 70};
const int64_t kBase[kTables + 1] = {0, 1, 6, 76};
// one seed per table: one at or above 2^63, one with a non-zero high word, a small one
const uint64_t kSeeds[kTables] = {0xF00DFACE12345678ull, 0x0000000500000007ull, 3ull};
constexpr uint64_t kStep = 0x100000005ull;       // (the high word goes into the key)
constexpr float kLr = 0.75f / 64.f;               // row-wise Adam: divided by 4, 8 or 16 before it meets a moment
// SGD: lr * g is 3/8 to 9/8 of the type's spacing at 4 (2^-8 for fp16, 2^-5 for bf16), so that w - lr * g falls between
// two values of the type for most weights and the two roundings part on a good share of the elements
inline float SgdLr(__half) { return 0.75f / 4096.f; }
inline float SgdLr(__hip_bfloat16) { return 0.75f / 512.f; }
constexpr float kEps = 1.0f;
// (second moment of the row before, gradient magnitude): sqrt(v / 2 + g^2 / 2) + eps = 4, 8, 16
constexpr float kSecond[3] = {2.f, 62.f, 446.f};
constexpr float kMagnitude[3] = {4.f, 6.f, 2.f};
constexpr int kTail = 5;                         // entries past the count

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

int g_failures = 0;
int g_checks = 0;

void Expect(const bool ok, const char* what, const char* detail, const long at = -1) {
  ++g_checks;
  if (ok) return;
  ++g_failures;
  std::fprintf(stderr, "FAILED %s: %s (at %ld)\n", what, detail, at);
}

template <typename T>
T* ToDevice(const std::vector<T>& v) {
  T* p = nullptr;
  HIP_OK(hipMalloc(reinterpret_cast<void**>(&p), (v.empty() ? 1 : v.size()) * sizeof(T)));
  if (!v.empty()) HIP_OK(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  return p;
}

template <typename T>
std::vector<T> ToHost(const T* p, const size_t n) {
  std::vector<T> v(n);
  HIP_OK(hipMemcpy(v.data(), p, n * sizeof(T), hipMemcpyDeviceToHost));
  return v;
}

//! Whether row r of table t is named by an entry: all of table 0, rows 1..3 of table 1, rows 0..63 of table 2.
bool Named(const int t, const int64_t r) { return t == 0 || (t == 1 && r >= 1 && r <= 3) || (t == 2 && r < 64); }

float WeightOf(const int t, const int64_t r, const int j) { return static_cast<float>((r * 5 + j * 3 + t * 7) % 17 - 8); }
//! The first moment before the step: an even integer in [-4, 4] (m / 2 + g / 2 is exact).
float FirstOf(const int t, const int64_t r, const int j) { return static_cast<float>(((r + j + t) % 5) * 2 - 4); }

//! The stochastic rounding of x for (table t, row r inside it, column), as the specification's host functions give it.
template <typename ElemT>
uint16_t Rounded(const float x, const int t, const int64_t r, const int column) {
  const cuembed::detail::PhiloxWords p =
      cuembed::detail::RoundingWords(kSeeds[t], kStep, static_cast<uint64_t>(r), static_cast<uint32_t>(column) / 8);
  return RoundBits(ElemT(), x, cuembed::detail::RoundingField(p, column % 8));
}

template <typename ElemT, typename IndexT>
void Case(const bool adam, const int width, const char* what) {
  // the tensors of every table, on the host (what they hold before; what they must hold after) and on the device
  std::vector<ElemT> table_h[kTables];
  std::vector<uint16_t> want_table[kTables];
  std::vector<float> first_h[kTables], second_h[kTables], want_first[kTables], want_second[kTables];
  ElemT* tables[kTables];
  float* first[kTables];
  float* second[kTables];
  std::vector<IndexT> ids;
  std::vector<ElemT> grad;
  size_t differ = 0, rounded = 0;
  for (int t = 0; t < kTables; ++t) {
    table_h[t].resize(kRows[t] * width);
    first_h[t].resize(kRows[t] * width);
    second_h[t].resize(kRows[t]);
    for (int64_t r = 0; r < kRows[t]; ++r) {
      second_h[t][r] = kSecond[r % 3];
      for (int j = 0; j < width; ++j) {
        table_h[t][r * width + j] = From<ElemT>(WeightOf(t, r, j));
        first_h[t][r * width + j] = FirstOf(t, r, j);
      }
    }
    want_table[t].resize(table_h[t].size());
    for (size_t i = 0; i < table_h[t].size(); ++i) want_table[t][i] = Bits(table_h[t][i]);
    want_first[t] = first_h[t];
    want_second[t] = second_h[t];
    for (int64_t r = 0; r < kRows[t]; ++r) {
      if (!Named(t, r)) continue;
      const int64_t k = static_cast<int64_t>(ids.size());
      ids.push_back(static_cast<IndexT>(kBase[t] + r));
      const float mag = kMagnitude[r % 3];
      const float second_new = 0.5f * kSecond[r % 3] + 0.5f * (mag * mag);
      const float denominator = std::sqrt(second_new) + kEps;       // 4, 8 or 16
      if (adam) want_second[t][r] = second_new;
      for (int j = 0; j < width; ++j) {
        const float g = ((k + j) % 2 ? -1.f : 1.f) * mag;
        grad.push_back(From<ElemT>(g));
        float x;
        if (adam) {
          const float m_new = 0.5f * FirstOf(t, r, j) + 0.5f * g;
          want_first[t][r * width + j] = m_new;
          x = WeightOf(t, r, j) - (kLr / denominator) * m_new;
        } else {
          x = WeightOf(t, r, j) - SgdLr(ElemT()) * g;
        }
        want_table[t][r * width + j] = Rounded<ElemT>(x, t, r, j);
        differ += want_table[t][r * width + j] != Bits(From<ElemT>(x));
        ++rounded;
      }
    }
    tables[t] = ToDevice(table_h[t]);
    first[t] = ToDevice(first_h[t]);
    second[t] = ToDevice(second_h[t]);
  }
  const int64_t entries = static_cast<int64_t>(ids.size());
  Expect(entries == 1 + 3 + 64, what, "the data: 68 entries");
  Expect(differ * 8 >= rounded, what, "the data: stochastic and nearest differ often");
  for (int k = 0; k < kTail; ++k) {      // past the count: never looked at, whatever they hold
    ids.push_back(static_cast<IndexT>(k % 2 ? -1 : 5));
    for (int j = 0; j < width; ++j) grad.push_back(From<ElemT>(100.f));
  }
  IndexT* d_ids = ToDevice(ids);
  ElemT* d_grad = ToDevice(grad);
  int64_t* d_base = ToDevice(std::vector<int64_t>(kBase, kBase + kTables + 1));
  uint64_t* d_seeds = ToDevice(std::vector<uint64_t>(kSeeds, kSeeds + kTables));
  int64_t* d_step = ToDevice(std::vector<int64_t>{static_cast<int64_t>(kStep)});
  IndexT* d_last = ToDevice(std::vector<IndexT>{static_cast<IndexT>(entries - 1)});
  ElemT** d_tables = ToDevice(std::vector<ElemT*>(tables, tables + kTables));
  float** d_first = ToDevice(std::vector<float*>(first, first + kTables));
  float** d_second = ToDevice(std::vector<float*>(second, second + kTables));

  if (adam) {
    cuembed::SparseAdamOptions o;
    o.rule = cuembed::AdamRule::kRowwiseAdam;
    o.lr = kLr;
    o.bias_factor = 1.f;
    o.beta1 = o.one_minus_beta1 = o.beta2 = o.one_minus_beta2 = 0.5f;
    o.eps = kEps;
    o.weight_decay = 0.f;
    o.last_id = d_last;
    o.stochastic_rounding = true;
    o.rounding_seed = 0xBADull;           // (not read: the seeds are the tables')
    o.rounding_step = 77;                 // (not read either: the device word holds the step)
    o.rounding_step_device = d_step;
    cuembed::SparseRowAdamGrouped<ElemT, IndexT>(tables, d_tables, first, d_first, second, d_second, kTables, d_base, width,
                                                 d_ids, d_grad, entries + kTail, o, 0, d_seeds);
  } else {
    cuembed::SparseUpdateOptions o;
    o.rule = cuembed::UpdateRule::kSgd;
    o.lr = SgdLr(ElemT());
    o.num_rows = entries;
    o.stochastic_rounding = true;
    o.rounding_seed = 0xBADull;
    o.rounding_step = kStep;
    cuembed::SparseRowUpdateGrouped<ElemT, IndexT>(tables, d_tables, nullptr, nullptr, kTables, d_base, width, d_ids, d_grad,
                                                   entries + kTail, o, 0, d_seeds);
  }
  HIP_OK(hipDeviceSynchronize());
  HIP_OK(hipGetLastError());

  for (int t = 0; t < kTables; ++t) {
    const std::vector<ElemT> got = ToHost(tables[t], table_h[t].size());
    long bad = -1;
    for (size_t i = 0; i < got.size() && bad < 0; ++i)
      if (Bits(got[i]) != want_table[t][i]) bad = static_cast<long>(i);
    Expect(bad < 0, what, "a table element is not the rounding of (seeds[t], step, local row, column)", bad + 1000000L * t);
    const std::vector<float> got_first = ToHost(first[t], first_h[t].size());
    const std::vector<float> got_second = ToHost(second[t], second_h[t].size());
    const std::vector<float>& first_after = adam ? want_first[t] : first_h[t];
    Expect(std::memcmp(got_first.data(), first_after.data(), got_first.size() * sizeof(float)) == 0, what,
           adam ? "the first moments" : "SGD touched a state tensor it was not given", t);
    Expect(std::memcmp(got_second.data(), want_second[t].data(), got_second.size() * sizeof(float)) == 0, what,
           "the second moments' row words", t);
  }
  for (int t = 0; t < kTables; ++t) {
    (void)hipFree(tables[t]);
    (void)hipFree(first[t]);
    (void)hipFree(second[t]);
  }
  for (void* p : {static_cast<void*>(d_ids), static_cast<void*>(d_grad), static_cast<void*>(d_base),
                  static_cast<void*>(d_seeds), static_cast<void*>(d_step), static_cast<void*>(d_last),
                  static_cast<void*>(d_tables), static_cast<void*>(d_first), static_cast<void*>(d_second)})
    (void)hipFree(p);
  std::printf("%s: done\n", what);
}

}  // namespace

int main() {
  Case<__half, int32_t>(false, 8, "sgd half width 8 int32 ids, immediate step");
  Case<__hip_bfloat16, int64_t>(false, 40, "sgd bfloat16 width 40 int64 ids, immediate step");
  Case<__half, int64_t>(true, 40, "row-wise adam half width 40 int64 ids, device step word");
  Case<__hip_bfloat16, int32_t>(true, 8, "row-wise adam bfloat16 width 8 int32 ids, device step word");
  if (g_failures != 0) {
    std::printf("FAILED: %d of %d checks\n", g_failures, g_checks);
    return 1;
  }
  std::printf("grouped stochastic rounding: all %d known-answer checks passed\n", g_checks);
  return 0;
}
