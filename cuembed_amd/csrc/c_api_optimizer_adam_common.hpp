// Shared by the two C-ABI units of the sparse Adam step (c_api_optimizer_adam.hip: round to nearest and the bias-factor
// clock; c_api_optimizer_adam_stochastic.hip: stochastic rounding): the options of a call and the call on its types.
#ifndef CUEMBED_AMD_C_API_OPTIMIZER_ADAM_COMMON_HPP_
#define CUEMBED_AMD_C_API_OPTIMIZER_ADAM_COMMON_HPP_

#include "c_api_optimizer_common.hpp"
#include "cuembed/include/sparse_adam.hpp"

namespace cuembed_c_api {

inline cuembed::SparseAdamOptions AdamOptions(int rule, int64_t piece_rows, int pieces, int64_t num_rows,
                                              const void* counts, int counts_are_int64, const void* last_id, float lr,
                                              const float* lr_device, float bias_factor, const float* bias_factor_device,
                                              float beta1, float one_minus_beta1, float beta2, float one_minus_beta2,
                                              float eps, float weight_decay) {
  cuembed::SparseAdamOptions o;
  switch (rule) {
    case CUEMBED_ADAM: o.rule = cuembed::AdamRule::kAdam; break;
    case CUEMBED_ROWWISE_ADAM: o.rule = cuembed::AdamRule::kRowwiseAdam; break;
    default:
      std::cerr << "Check failed: unknown Adam rule at " << __FILE__ << ":" << __LINE__ << std::endl;
      std::abort();
  }
  FillStepOptions(o, piece_rows, pieces, num_rows, counts, counts_are_int64, last_id, lr, lr_device);
  o.bias_factor = bias_factor;
  o.bias_factor_device = bias_factor_device;
  o.beta1 = beta1;
  o.one_minus_beta1 = one_minus_beta1;
  o.beta2 = beta2;
  o.one_minus_beta2 = one_minus_beta2;
  o.eps = eps;
  o.weight_decay = weight_decay;
  return o;
}

template <typename ElemT, typename IndexT, cuembed::UpdateRoundings kRoundings>
void Adam(void* table, float* exp_avg, float* exp_avg_sq, int embed_width, const void* ids, const void* rows,
          const cuembed::SparseAdamOptions& options, cuembed_stream_t stream) {
  cuembed::SparseRowAdam<ElemT, IndexT, kRoundings>(static_cast<ElemT*>(table), exp_avg, exp_avg_sq, embed_width,
                                                    static_cast<const IndexT*>(ids), static_cast<const ElemT*>(rows),
                                                    options, Stream(stream));
}

}  // namespace cuembed_c_api

#endif  // CUEMBED_AMD_C_API_OPTIMIZER_ADAM_COMMON_HPP_
