// Shared by the two C-ABI units of the sparse optimizer step (c_api_optimizer.hip: round to nearest;
// c_api_optimizer_stochastic.hip: stochastic rounding): the options of a call and the call on its types.
#ifndef CUEMBED_AMD_C_API_OPTIMIZER_COMMON_HPP_
#define CUEMBED_AMD_C_API_OPTIMIZER_COMMON_HPP_

#include "c_api_common.hpp"
#include "cuembed/include/sparse_update.hpp"

namespace cuembed_c_api {

//! The fields that the options of every sparse step share (also c_api_optimizer_adam_common.hpp's).
inline void FillStepOptions(cuembed::SparseStepOptions& o, int64_t piece_rows, int pieces, int64_t num_rows,
                            const void* counts, int counts_are_int64, const void* last_id, float lr,
                            const float* lr_device) {
  o.lr = lr;
  o.lr_device = lr_device;
  o.piece_rows = piece_rows;
  o.pieces = pieces;
  o.num_rows = num_rows;
  o.counts = counts;
  o.counts_are_int64 = counts_are_int64 != 0;
  o.last_id = last_id;
}

inline void FillStochasticRounding(cuembed::SparseStepOptions& o, uint64_t seed, uint64_t step, const int64_t* step_device) {
  o.stochastic_rounding = true;
  o.rounding_seed = seed;
  o.rounding_step = step;
  o.rounding_step_device = step_device;
}

inline cuembed::SparseUpdateOptions UpdateOptions(int rule, int64_t piece_rows, int pieces, int64_t num_rows,
                                                  const void* counts, int counts_are_int64, const void* last_id, float lr,
                                                  const float* lr_device, float eps) {
  cuembed::SparseUpdateOptions o;
  switch (rule) {
    case CUEMBED_UPDATE_SGD: o.rule = cuembed::UpdateRule::kSgd; break;
    case CUEMBED_UPDATE_ADAGRAD: o.rule = cuembed::UpdateRule::kAdagrad; break;
    case CUEMBED_UPDATE_ROWWISE_ADAGRAD: o.rule = cuembed::UpdateRule::kRowwiseAdagrad; break;
    default:
      std::cerr << "Check failed: unknown update rule at " << __FILE__ << ":" << __LINE__ << std::endl;
      std::abort();
  }
  FillStepOptions(o, piece_rows, pieces, num_rows, counts, counts_are_int64, last_id, lr, lr_device);
  o.eps = eps;
  return o;
}

template <typename ElemT, typename IndexT, cuembed::UpdateRoundings kRoundings>
void Update(void* table, float* state, int embed_width, const void* ids, const void* rows,
            const cuembed::SparseUpdateOptions& options, cuembed_stream_t stream) {
  cuembed::SparseRowUpdate<ElemT, IndexT, kRoundings>(static_cast<ElemT*>(table), state, embed_width,
                                                      static_cast<const IndexT*>(ids), static_cast<const ElemT*>(rows),
                                                      options, Stream(stream));
}

}  // namespace cuembed_c_api

#endif  // CUEMBED_AMD_C_API_OPTIMIZER_COMMON_HPP_
