// C ABI: the sparse optimizer step with stochastic rounding (16-bit tables) = the kStochastic instantiations of
// cuembed::SparseRowUpdate, in a unit of their own so that they compile next to the round-to-nearest ones; and the
// host-only helpers that expose the specification (the random bits, the rounding rule) to tests and FFI users.
#include "c_api_optimizer_common.hpp"

extern "C" {

void cuembed_sparse_row_update_stochastic(void* table, int elem_type, int embed_width, float* state, int rule,
                                          const void* ids, int index_type, const void* rows, int64_t piece_rows,
                                          int pieces, int64_t num_rows, const void* counts, int counts_are_int64,
                                          const void* last_id, float lr, const float* lr_device, float eps,
                                          uint64_t seed, uint64_t step, const int64_t* step_device,
                                          cuembed_stream_t stream) {
  cuembed::SparseUpdateOptions o = cuembed_c_api::UpdateOptions(rule, piece_rows, pieces, num_rows, counts,
                                                                counts_are_int64, last_id, lr, lr_device, eps);
  cuembed_c_api::FillStochasticRounding(o, seed, step, step_device);
  const bool known = cuembed_c_api::DispatchTypes<false>(elem_type, index_type, [&](auto elem, auto index) {
    using E = typename decltype(elem)::type;
    using I = typename decltype(index)::type;
    cuembed_c_api::Update<E, I, cuembed::UpdateRoundings::kStochasticOnly>(table, state, embed_width, ids, rows, o, stream);
  });
  if (!known) CUEMBED_C_API_BAD_TYPE();   // (float tables have no rounding to randomise)
}

void cuembed_stochastic_rounding_words(uint64_t seed, uint64_t step, int64_t row, uint32_t column_group, uint32_t* out) {
  const cuembed::detail::PhiloxWords p =
      cuembed::detail::RoundingWords(seed, step, static_cast<uint64_t>(row), column_group);
  for (int i = 0; i < 4; ++i) out[i] = p.w[i];
}

uint16_t cuembed_stochastic_round(int elem_type, float x, uint32_t r16) {
  if (elem_type == CUEMBED_F16) return cuembed::detail::StochasticRoundToHalfBits(x, r16);
  if (elem_type == CUEMBED_BF16) return cuembed::detail::StochasticRoundToBf16Bits(x, r16);
  CUEMBED_C_API_BAD_TYPE();
}

void cuembed_stochastic_round_array(int elem_type, const float* x, const uint32_t* r16, int64_t n, uint16_t* out) {
  if (elem_type != CUEMBED_F16 && elem_type != CUEMBED_BF16) CUEMBED_C_API_BAD_TYPE();
  for (int64_t i = 0; i < n; ++i)
    out[i] = elem_type == CUEMBED_F16 ? cuembed::detail::StochasticRoundToHalfBits(x[i], r16[i])
                                      : cuembed::detail::StochasticRoundToBf16Bits(x[i], r16[i]);
}

}  // extern "C"
