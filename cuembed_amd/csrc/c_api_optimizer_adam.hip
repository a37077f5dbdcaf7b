// C ABI: the sparse Adam step = explicit instantiations of cuembed::SparseRowAdam (round to nearest; the stochastic
// kernels are c_api_optimizer_adam_stochastic.hip's), with or without placed moments, and the bias-factor clock.
#include "c_api_optimizer_adam_common.hpp"

extern "C" {

void cuembed_sparse_row_adam(void* table, int elem_type, int embed_width, float* exp_avg, float* exp_avg_sq, int rule,
                             const void* ids, int index_type, const void* rows, int64_t piece_rows, int pieces,
                             int64_t num_rows, const void* counts, int counts_are_int64, const void* last_id, float lr,
                             const float* lr_device, float bias_factor, const float* bias_factor_device, float beta1,
                             float one_minus_beta1, float beta2, float one_minus_beta2, float eps, float weight_decay,
                             cuembed_stream_t stream) {
  const cuembed::SparseAdamOptions o = cuembed_c_api::AdamOptions(
      rule, piece_rows, pieces, num_rows, counts, counts_are_int64, last_id, lr, lr_device, bias_factor,
      bias_factor_device, beta1, one_minus_beta1, beta2, one_minus_beta2, eps, weight_decay);
  const bool known = cuembed_c_api::DispatchTypes<true>(elem_type, index_type, [&](auto elem, auto index) {
    using E = typename decltype(elem)::type;
    using I = typename decltype(index)::type;
    cuembed_c_api::Adam<E, I, cuembed::UpdateRoundings::kNearestOnly>(table, exp_avg, exp_avg_sq, embed_width, ids, rows, o,
                                                                      stream);
  });
  if (!known) CUEMBED_C_API_BAD_TYPE();
}

void cuembed_sparse_row_adam_placed(void* table, int elem_type, int embed_width, float* exp_avg, float* exp_avg_sq,
                                    int rule, const void* ids, int index_type, const void* rows, int64_t piece_rows,
                                    int pieces, int64_t num_rows, const void* counts, int counts_are_int64,
                                    const void* last_id, float lr, const float* lr_device, float bias_factor,
                                    const float* bias_factor_device, float beta1, float one_minus_beta1, float beta2,
                                    float one_minus_beta2, float eps, float weight_decay, cuembed_stream_t stream,
                                    const int64_t* exp_avg_ids, const int64_t* exp_avg_sq_ids) {
  const cuembed::SparseAdamOptions o = cuembed_c_api::AdamOptions(
      rule, piece_rows, pieces, num_rows, counts, counts_are_int64, last_id, lr, lr_device, bias_factor,
      bias_factor_device, beta1, one_minus_beta1, beta2, one_minus_beta2, eps, weight_decay);
  const bool known = cuembed_c_api::DispatchTypes<true>(elem_type, index_type, [&](auto elem, auto index) {
    using E = typename decltype(elem)::type;
    using I = typename decltype(index)::type;
    cuembed::SparseRowAdam<E, I, cuembed::UpdateRoundings::kNearestOnly>(
        static_cast<E*>(table), exp_avg, exp_avg_sq, embed_width, static_cast<const I*>(ids), static_cast<const E*>(rows), o,
        cuembed_c_api::Stream(stream), exp_avg_ids, exp_avg_sq_ids);
  });
  if (!known) CUEMBED_C_API_BAD_TYPE();
}

void cuembed_adam_clock_advance(double* powers, float* bias_factor, double beta1, double beta2, cuembed_stream_t stream) {
  cuembed::AdamClockAdvance(powers, bias_factor, beta1, beta2, cuembed_c_api::Stream(stream));
}

}  // extern "C"
