// Stochastic rounding of an fp32 value to fp16 / bf16, and the counter-based random bits that drive it -- one
// definition for host and device (the sparse optimizer step uses it on the device, the C ABI's helpers and the CPU
// tests run the same text on the host).
//
//   * The bits: Philox4x32-10 (Salmon et al., SC'11; the constants are Random123's).  One call serves the 8 elements of
//     column group c / 8 of table row `row`:
//         counter = (row low 32, row high 32, c / 8, step low 32)      key = (seed low 32, seed high 32 ^ step high 32)
//     and element c takes the 16-bit field c % 8: half (c % 8) % 2 (low half first) of output word (c % 8) / 2.  A field
//     depends on nothing but (seed, step, table row, column): no generator state lives in memory.
//   * The rule, for the fp32 value x the kernel would store and a 16-bit field r:
//       fp16  q = spacing of fp16 at |x| (2^(e-10) for |x| >= 2^-14, else 2^-24), m = |x| / q, i = floor(m),
//             t = floor((m - i) * 2^13); away from zero iff t + (r & 0x1FFF) >= 2^13; result +-(i + up) * q.
//             In fp16's normal range t is the 13 discarded mantissa bits (P(up) is exactly the fractional position), in
//             its subnormal range the first 13 bits of the fraction (within 2^-13 of it).
//       bf16  r is added to the low 16 bits of the fp32 pattern, which are then dropped: exact everywhere.
//     A value the 16-bit type represents comes back unchanged for every r; a result past the largest finite value is
//     +-inf; inf and NaN take the ordinary conversion; the sign of zero is kept.
//     Everything is integer work on the bit pattern, so it does not depend on the denormal mode.
#ifndef CUEMBED_INCLUDE_STOCHASTIC_ROUNDING_HPP_
#define CUEMBED_INCLUDE_STOCHASTIC_ROUNDING_HPP_

#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

namespace cuembed {
namespace detail {

//! The four output words of one Philox4x32-10 call.
struct PhiloxWords {
  uint32_t w[4];
};

//! Philox4x32-10.  Each round is two 32 x 32 -> 64 products (one v_mad_u64_u32 each on gfx950).
__host__ __device__ __forceinline__ PhiloxWords Philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                                              uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint64_t p0 = static_cast<uint64_t>(0xD2511F53u) * c0;
    const uint64_t p1 = static_cast<uint64_t>(0xCD9E8D57u) * c2;
    const uint32_t n0 = static_cast<uint32_t>(p1 >> 32) ^ c1 ^ k0;
    const uint32_t n2 = static_cast<uint32_t>(p0 >> 32) ^ c3 ^ k1;
    c1 = static_cast<uint32_t>(p1);
    c3 = static_cast<uint32_t>(p0);
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return PhiloxWords{{c0, c1, c2, c3}};
}

//! The call that serves columns [8 * column_group, 8 * column_group + 8) of table row `row` at (seed, step).
__host__ __device__ __forceinline__ PhiloxWords RoundingWords(const uint64_t seed, const uint64_t step, const uint64_t row,
                                                              const uint32_t column_group) {
  return Philox4x32_10(static_cast<uint32_t>(row), static_cast<uint32_t>(row >> 32), column_group,
                       static_cast<uint32_t>(step), static_cast<uint32_t>(seed),
                       static_cast<uint32_t>(seed >> 32) ^ static_cast<uint32_t>(step >> 32));
}

//! Field j (0..7) of a call: half j % 2 (low half first) of word j / 2.
__host__ __device__ __forceinline__ uint32_t RoundingField(const PhiloxWords& p, const int j) {
  return (p.w[j >> 1] >> ((j & 1) * 16)) & 0xFFFFu;
}

__host__ __device__ __forceinline__ uint32_t FloatBits(const float x) { return __builtin_bit_cast(uint32_t, x); }

//! fp32 -> fp16 pattern by the rule above.
__host__ __device__ __forceinline__ uint16_t StochasticRoundToHalfBits(const float x, const uint32_t r) {
  const uint32_t bits = FloatBits(x);
  const uint32_t mag = bits & 0x7FFFFFFFu;
  if (mag >= 0x7F800000u) return __builtin_bit_cast(uint16_t, static_cast<_Float16>(x));   // inf, NaN
  const uint32_t sign = (bits >> 16) & 0x8000u;
  const uint32_t r13 = r & 0x1FFFu;
  const uint32_t exponent = mag >> 23;
  uint32_t h;
  if (exponent >= 113u) {
    // fp16's normal range: add into the 13 bits that fp16 drops, truncate, re-bias (127 - 15 = 112)
    const uint32_t sum = mag + r13;
    h = sum >= 0x47800000u ? 0x7C00u : (sum - 0x38000000u) >> 13;
  } else {
    // below 2^-14: |x| in units of 2^-37 (2^-24 / 2^13), truncated; at most 2^23 - 1
    const uint32_t mantissa = (mag & 0x7FFFFFu) | (exponent != 0u ? 0x800000u : 0u);
    const uint32_t shift = 113u - (exponent != 0u ? exponent : 1u);
    const uint32_t units = shift < 32u ? mantissa >> shift : 0u;
    h = (units + r13) >> 13;
  }
  return static_cast<uint16_t>(sign | h);
}

//! fp32 -> bf16 pattern by the rule above (a finite value's carry into 0x7F80 is the overflow to inf).
__host__ __device__ __forceinline__ uint16_t StochasticRoundToBf16Bits(const float x, const uint32_t r) {
  const uint32_t bits = FloatBits(x);
  if ((bits & 0x7FFFFFFFu) >= 0x7F800000u) return __builtin_bit_cast(uint16_t, static_cast<__bf16>(x));   // inf, NaN
  return static_cast<uint16_t>((bits + (r & 0xFFFFu)) >> 16);
}

//! The same, typed for the kernels (ElemT = _Float16 or __bf16).
template <typename ElemT>
__host__ __device__ __forceinline__ ElemT StochasticRound(const float x, const uint32_t r) {
  static_assert(std::is_same<ElemT, _Float16>::value || std::is_same<ElemT, __bf16>::value,
                "stochastic rounding is for the 16-bit table types");
  if constexpr (std::is_same<ElemT, _Float16>::value) return __builtin_bit_cast(_Float16, StochasticRoundToHalfBits(x, r));
  else return __builtin_bit_cast(__bf16, StochasticRoundToBf16Bits(x, r));
}

}  // namespace detail
}  // namespace cuembed

#endif  // CUEMBED_INCLUDE_STOCHASTIC_ROUNDING_HPP_
