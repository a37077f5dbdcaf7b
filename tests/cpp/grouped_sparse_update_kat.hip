// The grouped optimizer step through the HEADER-ONLY API: cuembed::SparseRowUpdateGrouped / SparseRowAdamGrouped on a
// group of three separate tables with 1, 5 and 70 rows, against cuembed::SparseRowUpdate / SparseRowAdam called once per
// table on copies of the same data, inside this program.  Every row of every table is named, so both table boundaries
// fall inside one wavefront's entries; the count comes from a device word (last_id) and the arrays have a tail of
// entries past it that name no row.  Tables and every state tensor must agree BIT FOR BIT.  Data are hashed values.
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

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
constexpr int64_t kEntries = 76;    // every row
constexpr int64_t kCapacity = 83;   // + a tail past the count

float Hashed(uint32_t i, uint32_t salt) {
  uint32_t h = (i + 1u) * 2654435761u ^ (salt + 1u) * 0x9E3779B9u;
  h ^= h >> 15;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return static_cast<float>(h >> 8) * (1.0f / 16777216.0f) - 0.5f;
}

template <typename ElemT>
ElemT FromFloat(float x);
template <>
float FromFloat<float>(float x) { return x; }
template <>
__half FromFloat<__half>(float x) { return __float2half(x); }
template <>
__hip_bfloat16 FromFloat<__hip_bfloat16>(float x) { return __float2bfloat16(x); }

template <typename T>
T* ToDevice(const std::vector<T>& v) {
  T* p = nullptr;
  HIP_OK(hipMalloc(&p, (v.empty() ? 1 : v.size()) * sizeof(T)));
  if (!v.empty()) HIP_OK(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  return p;
}

template <typename T>
bool SameBits(const T* a, const T* b, size_t n) {
  std::vector<T> ha(n), hb(n);
  HIP_OK(hipMemcpy(ha.data(), a, n * sizeof(T), hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(hb.data(), b, n * sizeof(T), hipMemcpyDeviceToHost));
  return std::memcmp(ha.data(), hb.data(), n * sizeof(T)) == 0;
}

// One tensor per table, twice (side 0: the grouped call's, side 1: the per-table calls'), with the same hashed values.
template <typename T>
struct PerTable {
  T* at[2][kTables];
  size_t elems[kTables];
  PerTable(int row_elems, uint32_t salt, bool positive) {
    for (int t = 0; t < kTables; ++t) {
      elems[t] = static_cast<size_t>(kRows[t]) * row_elems;
      std::vector<T> v(elems[t]);
      for (size_t i = 0; i < v.size(); ++i) {
        const float x = Hashed(static_cast<uint32_t>(i), salt + 17u * t);
        v[i] = FromFloat<T>(positive ? x + 0.5f : x);
      }
      at[0][t] = ToDevice(v);
      at[1][t] = ToDevice(v);
    }
  }
  ~PerTable() {
    for (auto& side : at)
      for (T* p : side) (void)hipFree(p);
  }
  bool Same() const {
    bool same = true;
    for (int t = 0; t < kTables; ++t) same = same && SameBits(at[0][t], at[1][t], elems[t]);
    return same;
  }
  T** Pointers(int side) { return at[side]; }
};

template <typename T>
T** DevicePointers(T* const* host) {
  return ToDevice(std::vector<T*>(host, host + kTables));
}

// rule: 0 sgd, 1 adagrad, 2 row-wise adagrad, 3 adam, 4 row-wise adam
template <typename ElemT>
bool Case(const char* name, int width, int rule) {
  PerTable<ElemT> tables(width, 100u + rule, false);
  const bool rowwise = rule == 2 || rule == 4;
  PerTable<float> state0(rule == 2 ? 1 : width, 200u + rule, true);           // adagrad state / exp_avg
  PerTable<float> state1(rowwise ? 1 : width, 300u + rule, true);             // exp_avg_sq
  std::vector<int32_t> ids(kCapacity), local(kCapacity);
  for (int64_t k = 0; k < kCapacity; ++k) ids[k] = k < kEntries ? static_cast<int32_t>(k) : (k % 2 ? -1 : 81);
  int64_t cut[kTables + 1];
  for (int t = 0; t <= kTables; ++t) cut[t] = kBase[t];   // (every row is named: entry k names global row k)
  for (int t = 0; t < kTables; ++t)
    for (int64_t k = cut[t]; k < cut[t + 1]; ++k) local[k] = static_cast<int32_t>(ids[k] - kBase[t]);
  std::vector<ElemT> rows(kCapacity * width);
  for (size_t i = 0; i < rows.size(); ++i) rows[i] = FromFloat<ElemT>(Hashed(static_cast<uint32_t>(i), 400u + rule));
  int32_t* d_ids = ToDevice(ids);
  int32_t* d_local = ToDevice(local);
  ElemT* d_rows = ToDevice(rows);
  int32_t* d_last = ToDevice(std::vector<int32_t>{static_cast<int32_t>(kEntries - 1)});
  int64_t* d_base = ToDevice(std::vector<int64_t>(kBase, kBase + kTables + 1));
  ElemT** d_tables = DevicePointers(tables.Pointers(0));
  float** d_state0 = DevicePointers(state0.Pointers(0));
  float** d_state1 = DevicePointers(state1.Pointers(0));

  if (rule <= 2) {
    cuembed::SparseUpdateOptions o;
    o.rule = static_cast<cuembed::UpdateRule>(rule);
    o.lr = 0.0371f;
    o.eps = 1e-3f;
    cuembed::SparseUpdateOptions grouped = o;
    grouped.last_id = d_last;
    cuembed::SparseRowUpdateGrouped<ElemT, int32_t>(tables.Pointers(0), d_tables, rule == 0 ? nullptr : state0.Pointers(0),
                                                    rule == 0 ? nullptr : d_state0, kTables, d_base, width, d_ids, d_rows,
                                                    kCapacity, grouped);
    for (int t = 0; t < kTables; ++t) {
      cuembed::SparseUpdateOptions one = o;
      one.piece_rows = one.num_rows = cut[t + 1] - cut[t];
      cuembed::SparseRowUpdate<ElemT, int32_t>(tables.at[1][t], rule == 0 ? nullptr : state0.at[1][t], width,
                                               d_local + cut[t], d_rows + cut[t] * width, one);
    }
  } else {
    cuembed::SparseAdamOptions o;
    o.rule = rule == 3 ? cuembed::AdamRule::kAdam : cuembed::AdamRule::kRowwiseAdam;
    o.lr = 0.0371f;
    o.bias_factor = 0.7316f;
    o.eps = 1e-3f;
    o.weight_decay = 0.0125f;
    cuembed::SparseAdamOptions grouped = o;
    grouped.last_id = d_last;
    cuembed::SparseRowAdamGrouped<ElemT, int32_t>(tables.Pointers(0), d_tables, state0.Pointers(0), d_state0,
                                                  state1.Pointers(0), d_state1, kTables, d_base, width, d_ids, d_rows,
                                                  kCapacity, grouped);
    for (int t = 0; t < kTables; ++t) {
      cuembed::SparseAdamOptions one = o;
      one.piece_rows = one.num_rows = cut[t + 1] - cut[t];
      cuembed::SparseRowAdam<ElemT, int32_t>(tables.at[1][t], state0.at[1][t], state1.at[1][t], width, d_local + cut[t],
                                             d_rows + cut[t] * width, one);
    }
  }
  HIP_OK(hipDeviceSynchronize());
  HIP_OK(hipGetLastError());
  const bool ok = tables.Same() && state0.Same() && state1.Same();
  std::printf("%s width %d rule %d: %s\n", name, width, rule, ok ? "ok" : "MISMATCH");
  for (void* p : {static_cast<void*>(d_ids), static_cast<void*>(d_local), static_cast<void*>(d_rows),
                  static_cast<void*>(d_last), static_cast<void*>(d_base), static_cast<void*>(d_tables),
                  static_cast<void*>(d_state0), static_cast<void*>(d_state1)})
    (void)hipFree(p);
  return ok;
}

}  // namespace

int main() {
  bool ok = true;
  for (int rule = 0; rule < 5; ++rule) {
    ok = Case<float>("float", 4, rule) && ok;
    ok = Case<__half>("half", 8, rule) && ok;
    ok = Case<__hip_bfloat16>("bfloat16", 36, rule) && ok;
    ok = Case<__half>("half", 128, rule) && ok;
  }
  if (!ok) {
    std::printf("FAILED\n");
    return 1;
  }
  std::printf("all grouped sparse update known-answer checks passed\n");
  return 0;
}
