// Header-only API check of the sparse Adam step (cuembed::SparseRowAdam, cuembed::AdamClockAdvance; sparse_adam.hpp):
// both rules with fp32 / fp16 / bf16 tables and int32 / int64 ids, every source of the entry count, lr and the bias
// factor as values and as device words, with and without weight decay and starting moments -- on data whose fp32
// arithmetic is exact, so that the expected table and moments are written down here and must be met bit for bit:
//
//   beta1 = 0.5, beta2 = 0.75, eps = 0, lr = 0.5, c = 0.5 (step size 0.25), g = +-a with a in {2, 4, 8}
//   from m = v = 0:            m' = g / 2,  v' = a^2 / 4 = (a / 2)^2,  w' = w - 0.25 * sign(g)
//   from m = 3 g, v = 5 a^2:   m' = 2 g,    v' = 4 a^2   = (2 a)^2,    w' = w - 0.25 * sign(g)
//   weight decay 0.25:         w is first replaced by w - 0.125 * w (w a small integer: exact in bf16 too)
//   row-wise: every element of a row has the same magnitude, so the mean of the squares is a^2 and v_r as above.
//
// The entries behind the count hold valid ids that repeat earlier ones with large rows: they must have no effect.
// Built by __graft_entry__.build() (compile check, no GPU needed), run by tests/test_gpu_cpp_sparse_adam.py.
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "cuembed/include/sparse_adam.hpp"

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
constexpr float kLr = 0.5f, kBias = 0.5f, kDecay = 0.25f;

enum class Source { kHostCount, kCountWord32, kCountWord64, kLastId, kTwoPieces };

template <typename ElemT, typename IndexT>
void Case(const cuembed::AdamRule rule, const int width, const Source source, const bool warm, hipStream_t stream,
          const char* what) {
  // entries 0..4 are the gradient (two pieces: 0..2 and 4..5); the last two repeat rows 7 and 3 with large rows
  const int ids_h[kCapacity] = {3, 7, 0, 12, 5, 9, 7, 3};
  const float magnitude[kCapacity] = {2.f, 4.f, 8.f, 4.f, 2.f, 8.f, 64.f, 64.f};
  std::vector<int> valid;
  if (source == Source::kTwoPieces) valid = {0, 1, 2, 4, 5};   // counts {3, 2} of two pieces of four
  else valid = {0, 1, 2, 3, 4};
  const bool rowwise = rule == cuembed::AdamRule::kRowwiseAdam;
  std::vector<float> table(kRows * width), grad(kCapacity * width);
  for (int r = 0; r < kRows; ++r)
    for (int j = 0; j < width; ++j) table[r * width + j] = static_cast<float>((r * 5 + j * 3) % 17 - 8);
  for (int k = 0; k < kCapacity; ++k)
    for (int j = 0; j < width; ++j) grad[k * width + j] = ((k + j) % 2 ? -1.f : 1.f) * magnitude[k];
  // moments: rows that are not named keep the marker 0.375 (a warm run gives the named rows m = 3 g, v = 5 a^2)
  std::vector<float> m(kRows * width, 0.375f), v(rowwise ? kRows : kRows * width, 0.375f);
  for (int k : valid) {
    const int r = ids_h[k];
    const float a = magnitude[k];
    for (int j = 0; j < width; ++j) {
      m[r * width + j] = warm ? 3.f * grad[k * width + j] : 0.f;
      if (!rowwise) v[r * width + j] = warm ? 5.f * a * a : 0.f;
    }
    if (rowwise) v[r] = warm ? 5.f * a * a : 0.f;
  }
  // the expected values, as derived above
  std::vector<float> want_table = table, want_m = m, want_v = v;
  for (int k : valid) {
    const int r = ids_h[k];
    const float a = magnitude[k];
    for (int j = 0; j < width; ++j) {
      const float g = grad[k * width + j];
      float w = want_table[r * width + j];
      if (warm) w = w - (kLr * kDecay) * w;
      want_table[r * width + j] = ToF(From<ElemT>(w - (g > 0.f ? 0.25f : -0.25f)));   // the one rounding to ElemT
      want_m[r * width + j] = warm ? 2.f * g : 0.5f * g;
      if (!rowwise) want_v[r * width + j] = warm ? 4.f * a * a : 0.25f * a * a;
    }
    if (rowwise) want_v[r] = warm ? 4.f * a * a : 0.25f * a * a;
  }
  std::vector<ElemT> table_e, grad_e;
  for (float x : table) table_e.push_back(From<ElemT>(x));
  for (float x : grad) grad_e.push_back(From<ElemT>(x));
  std::vector<IndexT> ids_e(ids_h, ids_h + kCapacity);
  DeviceArray<ElemT> d_table(table_e), d_grad(grad_e);
  DeviceArray<IndexT> d_ids(ids_e);
  DeviceArray<float> d_m(m), d_v(v);
  DeviceArray<int32_t> d_count32(std::vector<int32_t>{5});
  DeviceArray<int64_t> d_count64(std::vector<int64_t>{5});
  DeviceArray<int64_t> d_piece_counts(std::vector<int64_t>{3, 2});
  DeviceArray<IndexT> d_last(std::vector<IndexT>{4});
  DeviceArray<float> d_lr(std::vector<float>{kLr}), d_bias(std::vector<float>{kBias});

  cuembed::SparseAdamOptions o;
  o.rule = rule;
  o.beta1 = 0.5f, o.one_minus_beta1 = 0.5f;
  o.beta2 = 0.75f, o.one_minus_beta2 = 0.25f;
  o.eps = 0.f;
  o.weight_decay = warm ? kDecay : 0.f;
  o.piece_rows = kCapacity;
  o.lr = kLr;
  o.bias_factor = kBias;
  switch (source) {
    case Source::kHostCount: o.num_rows = 5; break;
    case Source::kCountWord32: o.counts = d_count32.ptr; o.bias_factor = 7.f; o.bias_factor_device = d_bias.ptr; break;
    case Source::kCountWord64: o.counts = d_count64.ptr; o.counts_are_int64 = true; o.lr = 7.f; o.lr_device = d_lr.ptr; break;
    case Source::kLastId:
      o.last_id = d_last.ptr; o.lr_device = d_lr.ptr; o.bias_factor_device = d_bias.ptr;
      break;
    case Source::kTwoPieces:
      o.pieces = 2; o.piece_rows = kCapacity / 2; o.counts = d_piece_counts.ptr; o.counts_are_int64 = true;
      break;
  }
  cuembed::SparseRowAdam<ElemT, IndexT>(d_table.ptr, d_m.ptr, d_v.ptr, width, d_ids.ptr, d_grad.ptr, o, stream);
  HIP_OK(hipGetLastError());
  HIP_OK(hipStreamSynchronize(stream));
  const std::vector<ElemT> got_table = d_table.host();
  const std::vector<float> got_m = d_m.host(), got_v = d_v.host();
  bool ok = true;
  for (size_t i = 0; i < got_table.size(); ++i) ok = ok && ToF(got_table[i]) == want_table[i];
  for (size_t i = 0; i < got_m.size(); ++i) ok = ok && got_m[i] == want_m[i];
  for (size_t i = 0; i < got_v.size(); ++i) ok = ok && got_v[i] == want_v[i];
  ++g_checks;
  if (!ok) {
    ++g_failures;
    std::fprintf(stderr, "MISMATCH %s rule %d width %d source %d warm %d\n", what, static_cast<int>(rule), width,
                 static_cast<int>(source), static_cast<int>(warm));
  }
}

template <typename ElemT, typename IndexT>
void AdamKat(hipStream_t stream, const char* what) {
  const cuembed::AdamRule rules[] = {cuembed::AdamRule::kAdam, cuembed::AdamRule::kRowwiseAdam};
  const Source sources[] = {Source::kHostCount, Source::kCountWord32, Source::kCountWord64, Source::kLastId,
                            Source::kTwoPieces};
  // 8: 16-byte lanes; 6: 8-byte (fp32) / 4-byte (16-bit) lanes; 520: several slices per lane; 1032: fp32 rows take
  // the run-time loop over slices
  const int widths[] = {8, 6, 520, 1032};
  for (const auto rule : rules)
    for (const int width : widths)
      for (const auto source : sources)
        for (const bool warm : {false, true}) Case<ElemT, IndexT>(rule, width, source, warm, stream, what);
}

// The widest overload with every id array nullptr is the plain overload: on copies of the same tensors the two calls
// must leave the same bits.  An fp16 table of width 8 (one 16-byte slice per row: two entries in flight), 5 valid
// entries of 8 (the last group's second entry is dead), the count from last_id, both roundings.  Forwarding is host
// code: no other shape is needed.
void NullIdsForward(const cuembed::AdamRule rule, const bool stochastic, hipStream_t stream) {
  constexpr int kWidth = 8;
  const int ids_h[kCapacity] = {3, 7, 0, 12, 5, 9, 7, 3};
  std::vector<__half> table, grad;
  for (int i = 0; i < kRows * kWidth; ++i) table.push_back(__float2half(static_cast<float>(i % 17 - 8) / 3.f));
  for (int i = 0; i < kCapacity * kWidth; ++i) grad.push_back(__float2half(static_cast<float>(i % 11 - 5) / 7.f));
  const std::vector<float> m(kRows * kWidth, 0.125f), v(rule == cuembed::AdamRule::kAdam ? kRows * kWidth : kRows, 0.25f);
  DeviceArray<__half> d_wide(table), d_plain(table), d_grad(grad);
  DeviceArray<float> d_wide_m(m), d_wide_v(v), d_plain_m(m), d_plain_v(v);
  DeviceArray<int32_t> d_ids(std::vector<int32_t>(ids_h, ids_h + kCapacity));
  DeviceArray<int32_t> d_last(std::vector<int32_t>{4});
  cuembed::SparseAdamOptions o;
  o.rule = rule;
  o.lr = 0.3f;
  o.weight_decay = 0.01f;
  o.piece_rows = kCapacity;
  o.last_id = d_last.ptr;
  o.stochastic_rounding = stochastic;
  o.rounding_seed = 11;
  o.rounding_step = 3;
  cuembed::SparseRowAdam<__half, int32_t>(d_wide.ptr, d_wide_m.ptr, d_wide_v.ptr, kWidth, d_ids.ptr, d_grad.ptr, o, stream,
                                          nullptr, nullptr, nullptr);
  cuembed::SparseRowAdam<__half, int32_t>(d_plain.ptr, d_plain_m.ptr, d_plain_v.ptr, kWidth, d_ids.ptr, d_grad.ptr, o, stream);
  HIP_OK(hipGetLastError());
  HIP_OK(hipStreamSynchronize(stream));
  const std::vector<__half> wide = d_wide.host(), plain = d_plain.host();
  const bool same = std::memcmp(wide.data(), plain.data(), wide.size() * sizeof(__half)) == 0 &&
                    std::memcmp(wide.data(), table.data(), wide.size() * sizeof(__half)) != 0 &&   // (and something moved)
                    d_wide_m.host() == d_plain_m.host() && d_wide_v.host() == d_plain_v.host();
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
  for (const auto rule : {cuembed::AdamRule::kAdam, cuembed::AdamRule::kRowwiseAdam})
    for (const bool stochastic : {false, true}) NullIdsForward(rule, stochastic, stream);
  AdamKat<float, int32_t>(stream, "float/int32");
  AdamKat<float, int64_t>(stream, "float/int64");
  AdamKat<__half, int32_t>(stream, "half/int32");
  AdamKat<__half, int64_t>(stream, "half/int64");
  AdamKat<__hip_bfloat16, int32_t>(stream, "bf16/int32");
  AdamKat<__hip_bfloat16, int64_t>(stream, "bf16/int64");
  // an empty gradient and a count above the capacity are no-ops (no launch / nothing applied)
  {
    std::vector<float> t(kRows * 8, 1.f), g(kCapacity * 8, 1.f), s(kRows * 8, 0.5f);
    DeviceArray<float> d_t(t), d_g(g), d_m(s), d_v(s);
    DeviceArray<int32_t> d_ids(std::vector<int32_t>(kCapacity, 2));
    DeviceArray<int32_t> d_over(std::vector<int32_t>{kCapacity + 1});
    cuembed::SparseAdamOptions o;
    o.lr = 1.f;
    o.piece_rows = kCapacity;
    o.num_rows = 0;
    cuembed::SparseRowAdam<float, int32_t>(d_t.ptr, d_m.ptr, d_v.ptr, 8, d_ids.ptr, d_g.ptr, o, stream);
    o.num_rows = -1;
    o.counts = d_over.ptr;
    cuembed::SparseRowAdam<float, int32_t>(d_t.ptr, d_m.ptr, d_v.ptr, 8, d_ids.ptr, d_g.ptr, o, stream);
    HIP_OK(hipStreamSynchronize(stream));
    ++g_checks;
    if (d_t.host() != t || d_m.host() != s || d_v.host() != s) {
      ++g_failures;
      std::fprintf(stderr, "MISMATCH empty / over-capacity gradient changed the table or the moments\n");
    }
  }
  // the clock: beta1 = 0.5, beta2 = 0.75 -> after one step (1, 0.5, 0.75) and c = sqrt(0.25) / 0.5 = 1 exactly; after
  // two (2, 0.25, 0.5625) and c = sqrt(0.4375) / 0.75, compared with the host's double computation to one fp32 ulp
  {
    DeviceArray<double> d_p(std::vector<double>{0.0, 1.0, 1.0});
    DeviceArray<float> d_c(std::vector<float>{-1.f});
    cuembed::AdamClockAdvance(d_p.ptr, d_c.ptr, 0.5, 0.75, stream);
    HIP_OK(hipStreamSynchronize(stream));
    const std::vector<double> p1 = d_p.host();
    const float c1 = d_c.host()[0];
    cuembed::AdamClockAdvance(d_p.ptr, d_c.ptr, 0.5, 0.75, stream);
    HIP_OK(hipGetLastError());
    HIP_OK(hipStreamSynchronize(stream));
    const std::vector<double> p2 = d_p.host();
    const float c2 = d_c.host()[0];
    const float want2 = static_cast<float>(std::sqrt(0.4375) / 0.75);
    ++g_checks;
    const bool ok = p1[0] == 1.0 && p1[1] == 0.5 && p1[2] == 0.75 && c1 == 1.f && p2[0] == 2.0 && p2[1] == 0.25 &&
                    p2[2] == 0.5625 && c2 >= std::nextafter(want2, 0.f) && c2 <= std::nextafter(want2, 2.f);
    if (!ok) {
      ++g_failures;
      std::fprintf(stderr, "MISMATCH clock: (%g %g %g) c %.9g, then (%g %g %g) c %.9g (want %.9g)\n", p1[0], p1[1], p1[2],
                   c1, p2[0], p2[1], p2[2], c2, want2);
    }
  }
  HIP_OK(hipStreamDestroy(stream));
  if (g_failures) {
    std::fprintf(stderr, "%d of %d sparse-Adam checks failed\n", g_failures, g_checks);
    return 1;
  }
  std::printf("sparse Adam: all %d known-answer checks passed\n", g_checks);
  return 0;
}
