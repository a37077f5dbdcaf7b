// C ABI: the sparse Adam step with stochastic rounding (16-bit tables) = the kStochastic instantiations of
// cuembed::SparseRowAdam, in a unit of their own so that they compile next to the round-to-nearest ones.
#include "c_api_optimizer_adam_common.hpp"

extern "C" {

void cuembed_sparse_row_adam_stochastic(void* table, int elem_type, int embed_width, float* exp_avg, float* exp_avg_sq,
                                        int rule, const void* ids, int index_type, const void* rows, int64_t piece_rows,
                                        int pieces, int64_t num_rows, const void* counts, int counts_are_int64,
                                        const void* last_id, float lr, const float* lr_device, float bias_factor,
                                        const float* bias_factor_device, float beta1, float one_minus_beta1, float beta2,
                                        float one_minus_beta2, float eps, float weight_decay, uint64_t seed,
                                        uint64_t step, const int64_t* step_device, cuembed_stream_t stream) {
  cuembed::SparseAdamOptions o = cuembed_c_api::AdamOptions(
      rule, piece_rows, pieces, num_rows, counts, counts_are_int64, last_id, lr, lr_device, bias_factor,
      bias_factor_device, beta1, one_minus_beta1, beta2, one_minus_beta2, eps, weight_decay);
  cuembed_c_api::FillStochasticRounding(o, seed, step, step_device);
  const bool known = cuembed_c_api::DispatchTypes<false>(elem_type, index_type, [&](auto elem, auto index) {
    using E = typename decltype(elem)::type;
    using I = typename decltype(index)::type;
    cuembed_c_api::Adam<E, I, cuembed::UpdateRoundings::kStochasticOnly>(table, exp_avg, exp_avg_sq, embed_width, ids, rows,
                                                                         o, stream);
  });
  if (!known) CUEMBED_C_API_BAD_TYPE();   // (float tables have no rounding to randomise)
}

}  // extern "C"
