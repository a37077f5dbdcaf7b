// Header-only API check of the sparse optimizer step (cuembed::SparseRowUpdate, sparse_update.hpp): every rule with
// fp32 / fp16 / bf16 tables and int32 / int64 ids, every source of the entry count, on data whose arithmetic is exact
// (small integers, power-of-two denominators), so that the table and the state must equal a host recomputation bit
// for bit.  The entries behind the count hold valid ids that repeat earlier ones with large rows: they must have no
// effect.  Built by __graft_entry__.build() (compile check, no GPU needed), run by tests/test_gpu_cpp_sparse_update.py.
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include <cmath>
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
template <> float From<float>(float v) { return v; }
template <> __half From<__half>(float v) { return __float2half(v); }
template <> __hip_bfloat16 From<__hip_bfloat16>(float v) { return __float2bfloat16(v); }
inline float ToF(float v) { return v; }
inline float ToF(__half v) { return __half2float(v); }
inline float ToF(__hip_bfloat16 v) { return __bfloat162float(v); }

static int g_failures = 0;
static int g_checks = 0;

constexpr int kRows = 16;      // table rows
constexpr int kCapacity = 8;   // entries the gradient buffers hold
constexpr float kLr = 0.75f;
constexpr float kEps = 1.0f;   // sqrt(state) + eps is a power of two for magnitudes 1, 3, 7

enum class Source { kHostCount, kCountWord32, kCountWord64, kLastId, kTwoPieces };

template <typename ElemT, typename IndexT>
void Case(const cuembed::UpdateRule rule, const int width, const Source source, hipStream_t stream, const char* what) {
  // entries 0..4 are the gradient (two pieces: 0..2 and 4..5); the last two repeat rows 7 and 3 with large rows
  const int ids_h[kCapacity] = {3, 7, 0, 12, 5, 9, 7, 3};
  const float magnitude[kCapacity] = {1.f, 3.f, 7.f, 3.f, 1.f, 7.f, 64.f, 64.f};
  std::vector<int> valid;
  if (source == Source::kTwoPieces) valid = {0, 1, 2, 4, 5};   // counts {3, 2} of two pieces of four
  else valid = {0, 1, 2, 3, 4};
  std::vector<float> table(kRows * width), grad(kCapacity * width);
  for (int r = 0; r < kRows; ++r)
    for (int j = 0; j < width; ++j) table[r * width + j] = static_cast<float>((r * 5 + j * 3) % 17 - 8);
  for (int k = 0; k < kCapacity; ++k)
    for (int j = 0; j < width; ++j) grad[k * width + j] = ((k + j) % 2 ? -1.f : 1.f) * magnitude[k];
  const bool per_element = rule == cuembed::UpdateRule::kAdagrad;
  const bool has_state = rule != cuembed::UpdateRule::kSgd;
  std::vector<float> state(has_state ? (per_element ? kRows * width : kRows) : 0, 0.f);
  // host recomputation (every operation is exact on this data)
  std::vector<float> want_table = table, want_state = state;
  for (int k : valid) {
    const int r = ids_h[k];
    const float m = magnitude[k];
    for (int j = 0; j < width; ++j) {
      const float g = grad[k * width + j];
      const float d = has_state ? kLr * g / (std::sqrt(m * m) + kEps) : kLr * g;
      want_table[r * width + j] = ToF(From<ElemT>(want_table[r * width + j] - d));   // the one rounding to ElemT
      if (per_element) want_state[r * width + j] += g * g;
    }
    if (has_state && !per_element) want_state[r] += m * m;   // the mean of `width` equal squares
  }
  std::vector<ElemT> table_e, grad_e;
  for (float v : table) table_e.push_back(From<ElemT>(v));
  for (float v : grad) grad_e.push_back(From<ElemT>(v));
  std::vector<IndexT> ids_e(ids_h, ids_h + kCapacity);
  DeviceArray<ElemT> d_table(table_e), d_grad(grad_e);
  DeviceArray<IndexT> d_ids(ids_e);
  DeviceArray<float> d_state(state);
  DeviceArray<int32_t> d_count32(std::vector<int32_t>{5});
  DeviceArray<int64_t> d_count64(std::vector<int64_t>{5});
  DeviceArray<int64_t> d_piece_counts(std::vector<int64_t>{3, 2});
  DeviceArray<IndexT> d_last(std::vector<IndexT>{4});
  DeviceArray<float> d_lr(std::vector<float>{kLr});

  cuembed::SparseUpdateOptions o;
  o.rule = rule;
  o.eps = kEps;
  o.piece_rows = kCapacity;
  switch (source) {
    case Source::kHostCount: o.num_rows = 5; o.lr = kLr; break;
    case Source::kCountWord32: o.counts = d_count32.ptr; o.lr = kLr; break;
    case Source::kCountWord64: o.counts = d_count64.ptr; o.counts_are_int64 = true; o.lr_device = d_lr.ptr; break;
    case Source::kLastId: o.last_id = d_last.ptr; o.lr_device = d_lr.ptr; break;
    case Source::kTwoPieces:
      o.pieces = 2; o.piece_rows = kCapacity / 2; o.counts = d_piece_counts.ptr; o.counts_are_int64 = true; o.lr = kLr;
      break;
  }
  cuembed::SparseRowUpdate<ElemT, IndexT>(d_table.ptr, has_state ? d_state.ptr : nullptr, width, d_ids.ptr, d_grad.ptr, o,
                                          stream);
  HIP_OK(hipGetLastError());
  HIP_OK(hipStreamSynchronize(stream));
  const std::vector<ElemT> got_table = d_table.host();
  const std::vector<float> got_state = d_state.host();
  bool ok = true;
  for (size_t i = 0; i < got_table.size(); ++i) ok = ok && ToF(got_table[i]) == want_table[i];
  for (size_t i = 0; i < got_state.size(); ++i) ok = ok && got_state[i] == want_state[i];
  ++g_checks;
  if (!ok) {
    ++g_failures;
    std::fprintf(stderr, "MISMATCH %s rule %d width %d source %d\n", what, static_cast<int>(rule), width,
                 static_cast<int>(source));
  }
}

template <typename ElemT, typename IndexT>
void UpdateKat(hipStream_t stream, const char* what) {
  const cuembed::UpdateRule rules[] = {cuembed::UpdateRule::kSgd, cuembed::UpdateRule::kAdagrad,
                                       cuembed::UpdateRule::kRowwiseAdagrad};
  const Source sources[] = {Source::kHostCount, Source::kCountWord32, Source::kCountWord64, Source::kLastId,
                            Source::kTwoPieces};
  // 8: 16-byte lanes; 6: 8-byte (fp32) / 4-byte (16-bit) lanes; 520: several slices per lane; 1032: fp32 rows take
  // the run-time loop over slices
  const int widths[] = {8, 6, 520, 1032};
  for (const auto rule : rules)
    for (const int width : widths)
      for (const auto source : sources) Case<ElemT, IndexT>(rule, width, source, stream, what);
}

// The widest overload with every id array nullptr is the plain overload: on copies of the same tensors the two calls
// must leave the same bits.  An fp16 table of width 8 (one 16-byte slice per row: two entries in flight), 5 valid
// entries of 8 (the last group's second entry is dead), the count from last_id, both roundings.  Forwarding is host
// code: no other shape is needed.
void NullIdsForward(const cuembed::UpdateRule rule, const bool stochastic, hipStream_t stream) {
  constexpr int kWidth = 8;
  const int ids_h[kCapacity] = {3, 7, 0, 12, 5, 9, 7, 3};
  std::vector<__half> table, grad;
  for (int i = 0; i < kRows * kWidth; ++i) table.push_back(__float2half(static_cast<float>(i % 17 - 8) / 3.f));
  for (int i = 0; i < kCapacity * kWidth; ++i) grad.push_back(__float2half(static_cast<float>(i % 11 - 5) / 7.f));
  const std::vector<float> state(rule == cuembed::UpdateRule::kAdagrad ? kRows * kWidth : kRows, 0.25f);
  DeviceArray<__half> d_wide(table), d_plain(table), d_grad(grad);
  DeviceArray<float> d_wide_state(state), d_plain_state(state);
  DeviceArray<int32_t> d_ids(std::vector<int32_t>(ids_h, ids_h + kCapacity));
  DeviceArray<int32_t> d_last(std::vector<int32_t>{4});
  cuembed::SparseUpdateOptions o;
  o.rule = rule;
  o.lr = 0.3f;
  o.piece_rows = kCapacity;
  o.last_id = d_last.ptr;
  o.stochastic_rounding = stochastic;
  o.rounding_seed = 11;
  o.rounding_step = 3;
  cuembed::SparseRowUpdate<__half, int32_t>(d_wide.ptr, d_wide_state.ptr, kWidth, d_ids.ptr, d_grad.ptr, o, stream, nullptr,
                                            nullptr);
  cuembed::SparseRowUpdate<__half, int32_t>(d_plain.ptr, d_plain_state.ptr, kWidth, d_ids.ptr, d_grad.ptr, o, stream);
  HIP_OK(hipGetLastError());
  HIP_OK(hipStreamSynchronize(stream));
  const std::vector<__half> wide = d_wide.host(), plain = d_plain.host();
  const bool same = std::memcmp(wide.data(), plain.data(), wide.size() * sizeof(__half)) == 0 &&
                    std::memcmp(wide.data(), table.data(), wide.size() * sizeof(__half)) != 0 &&   // (and something moved)
                    d_wide_state.host() == d_plain_state.host();
  ++g_checks;
  if (!same) {
    ++g_failures;
    std::fprintf(stderr, "MISMATCH null ids do not forward to the plain overload: rule %d stochastic %d\n",
                 static_cast<int>(rule), static_cast<int>(stochastic));
  }
}

int main() {
  hipStream_t stream;
  HIP_OK(hipStreamCreate(&stream));
  for (const auto rule : {cuembed::UpdateRule::kAdagrad, cuembed::UpdateRule::kRowwiseAdagrad})
    for (const bool stochastic : {false, true}) NullIdsForward(rule, stochastic, stream);
  UpdateKat<float, int32_t>(stream, "float/int32");
  UpdateKat<float, int64_t>(stream, "float/int64");
  UpdateKat<__half, int32_t>(stream, "half/int32");
  UpdateKat<__half, int64_t>(stream, "half/int64");
  UpdateKat<__hip_bfloat16, int32_t>(stream, "bf16/int32");
  UpdateKat<__hip_bfloat16, int64_t>(stream, "bf16/int64");
  // an empty gradient and a count above the capacity are no-ops (no launch / nothing applied)
  {
    std::vector<float> t(kRows * 8, 1.f), g(kCapacity * 8, 1.f);
    DeviceArray<float> d_t(t), d_g(g);
    DeviceArray<int32_t> d_ids(std::vector<int32_t>(kCapacity, 2));
    DeviceArray<int32_t> d_over(std::vector<int32_t>{kCapacity + 1});
    cuembed::SparseUpdateOptions o;
    o.lr = 1.f;
    o.piece_rows = kCapacity;
    o.num_rows = 0;
    cuembed::SparseRowUpdate<float, int32_t>(d_t.ptr, nullptr, 8, d_ids.ptr, d_g.ptr, o, stream);
    o.num_rows = -1;
    o.counts = d_over.ptr;
    cuembed::SparseRowUpdate<float, int32_t>(d_t.ptr, nullptr, 8, d_ids.ptr, d_g.ptr, o, stream);
    HIP_OK(hipStreamSynchronize(stream));
    ++g_checks;
    if (d_t.host() != t) {
      ++g_failures;
      std::fprintf(stderr, "MISMATCH empty / over-capacity gradient changed the table\n");
    }
  }
  HIP_OK(hipStreamDestroy(stream));
  if (g_failures) {
    std::fprintf(stderr, "%d of %d sparse-update checks failed\n", g_failures, g_checks);
    return 1;
  }
  std::printf("sparse update: all %d known-answer checks passed\n", g_checks);
  return 0;
}
