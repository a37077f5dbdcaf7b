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
#define ADAM(E, I) \
  cuembed_c_api::Adam<E, I, cuembed::UpdateRoundings::kNearestOnly>(table, exp_avg, exp_avg_sq, embed_width, ids, rows, o, stream)
  switch ((elem_type << 1) | index_type) {
    case 0: ADAM(float, int32_t); break;
    case 1: ADAM(float, int64_t); break;
    case 2: ADAM(__half, int32_t); break;
    case 3: ADAM(__half, int64_t); break;
    case 4: ADAM(__hip_bfloat16, int32_t); break;
    case 5: ADAM(__hip_bfloat16, int64_t); break;
    default: CUEMBED_C_API_BAD_TYPE();
  }
#undef ADAM
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
#define ADAM(E, I)                                                                                                 \
  cuembed::SparseRowAdam<E, I, cuembed::UpdateRoundings::kNearestOnly>(                                            \
      static_cast<E*>(table), exp_avg, exp_avg_sq, embed_width, static_cast<const I*>(ids), static_cast<const E*>(rows), \
      o, cuembed_c_api::Stream(stream), exp_avg_ids, exp_avg_sq_ids)
  switch ((elem_type << 1) | index_type) {
    case 0: ADAM(float, int32_t); break;
    case 1: ADAM(float, int64_t); break;
    case 2: ADAM(__half, int32_t); break;
    case 3: ADAM(__half, int64_t); break;
    case 4: ADAM(__hip_bfloat16, int32_t); break;
    case 5: ADAM(__hip_bfloat16, int64_t); break;
    default: CUEMBED_C_API_BAD_TYPE();
  }
#undef ADAM
}

void cuembed_adam_clock_advance(double* powers, float* bias_factor, double beta1, double beta2, cuembed_stream_t stream) {
  cuembed::AdamClockAdvance(powers, bias_factor, beta1, beta2, cuembed_c_api::Stream(stream));
}

}  // extern "C"
