// C ABI: the sparse optimizer step on a group of separate table tensors with stochastic rounding (16-bit tables) = the
// kStochasticOnly instantiations of cuembed::SparseRowUpdateGrouped / SparseRowAdamGrouped, in a unit of their own so that
// they compile next to the round-to-nearest ones (c_api_optimizer_grouped.hip).  One seed per table, read on the device.
#include "c_api_optimizer_adam_common.hpp"
#include "cuembed/include/grouped_sparse_update.hpp"

namespace {

constexpr cuembed::UpdateRoundings kStochasticOnly = cuembed::UpdateRoundings::kStochasticOnly;

float* const* Mutable(const void* const* p) {
  return reinterpret_cast<float* const*>(const_cast<void* const*>(reinterpret_cast<const void* const*>(p)));
}

template <typename ElemT, typename IndexT>
void UpdateGrouped(const void* const* tables_host, const void* const* tables_device, const void* const* state_host,
                   const void* const* state_device, int num_tables, const int64_t* row_base, int embed_width,
                   const void* ids, const void* rows, int64_t total_entries, const cuembed::SparseUpdateOptions& options,
                   const uint64_t* seeds_device, cuembed_stream_t stream) {
  cuembed::SparseRowUpdateGrouped<ElemT, IndexT, kStochasticOnly>(
      reinterpret_cast<const ElemT* const*>(tables_host),
      reinterpret_cast<ElemT* const*>(const_cast<void* const*>(reinterpret_cast<const void* const*>(tables_device))),
      reinterpret_cast<const float* const*>(state_host), Mutable(state_device), num_tables, row_base, embed_width,
      static_cast<const IndexT*>(ids), static_cast<const ElemT*>(rows), total_entries, options,
      cuembed_c_api::Stream(stream), seeds_device);
}

template <typename ElemT, typename IndexT>
void AdamGrouped(const void* const* tables_host, const void* const* tables_device, const void* const* exp_avg_host,
                 const void* const* exp_avg_device, const void* const* exp_avg_sq_host,
                 const void* const* exp_avg_sq_device, int num_tables, const int64_t* row_base, int embed_width,
                 const void* ids, const void* rows, int64_t total_entries, const cuembed::SparseAdamOptions& options,
                 const uint64_t* seeds_device, cuembed_stream_t stream) {
  cuembed::SparseRowAdamGrouped<ElemT, IndexT, kStochasticOnly>(
      reinterpret_cast<const ElemT* const*>(tables_host),
      reinterpret_cast<ElemT* const*>(const_cast<void* const*>(reinterpret_cast<const void* const*>(tables_device))),
      reinterpret_cast<const float* const*>(exp_avg_host), Mutable(exp_avg_device),
      reinterpret_cast<const float* const*>(exp_avg_sq_host), Mutable(exp_avg_sq_device), num_tables, row_base, embed_width,
      static_cast<const IndexT*>(ids), static_cast<const ElemT*>(rows), total_entries, options,
      cuembed_c_api::Stream(stream), seeds_device);
}

}  // namespace

extern "C" {

void cuembed_sparse_row_update_grouped_stochastic(const void* const* tables_host, const void* const* tables_device,
                                                  const void* const* state_host, const void* const* state_device,
                                                  int num_tables, int elem_type, int embed_width, const int64_t* row_base,
                                                  int rule, const void* ids, int index_type, const void* rows,
                                                  int64_t total_entries, int64_t num_rows, const void* count_word,
                                                  int count_word_is_64, const void* last_id, float lr,
                                                  const float* lr_device, float eps, const uint64_t* seeds_device,
                                                  uint64_t step, const int64_t* step_device, cuembed_stream_t stream) {
  cuembed::SparseUpdateOptions o = cuembed_c_api::UpdateOptions(rule, total_entries, 1, num_rows, count_word,
                                                                count_word_is_64, last_id, lr, lr_device, eps);
  cuembed_c_api::FillStochasticRounding(o, 0, step, step_device);   // (the seeds are the tables': seeds_device)
  const bool known = cuembed_c_api::DispatchTypes<false>(elem_type, index_type, [&](auto elem, auto index) {
    using E = typename decltype(elem)::type;
    using I = typename decltype(index)::type;
    UpdateGrouped<E, I>(tables_host, tables_device, state_host, state_device, num_tables, row_base, embed_width, ids, rows,
                        total_entries, o, seeds_device, stream);
  });
  if (!known) CUEMBED_C_API_BAD_TYPE();   // (float tables have no rounding to randomise)
}

void cuembed_sparse_row_adam_grouped_stochastic(const void* const* tables_host, const void* const* tables_device,
                                                const void* const* exp_avg_host, const void* const* exp_avg_device,
                                                const void* const* exp_avg_sq_host, const void* const* exp_avg_sq_device,
                                                int num_tables, int elem_type, int embed_width, const int64_t* row_base,
                                                int rule, const void* ids, int index_type, const void* rows,
                                                int64_t total_entries, int64_t num_rows, const void* count_word,
                                                int count_word_is_64, const void* last_id, float lr,
                                                const float* lr_device, float bias_factor,
                                                const float* bias_factor_device, float beta1, float one_minus_beta1,
                                                float beta2, float one_minus_beta2, float eps, float weight_decay,
                                                const uint64_t* seeds_device, uint64_t step, const int64_t* step_device,
                                                cuembed_stream_t stream) {
  cuembed::SparseAdamOptions o = cuembed_c_api::AdamOptions(
      rule, total_entries, 1, num_rows, count_word, count_word_is_64, last_id, lr, lr_device, bias_factor,
      bias_factor_device, beta1, one_minus_beta1, beta2, one_minus_beta2, eps, weight_decay);
  cuembed_c_api::FillStochasticRounding(o, 0, step, step_device);
  const bool known = cuembed_c_api::DispatchTypes<false>(elem_type, index_type, [&](auto elem, auto index) {
    using E = typename decltype(elem)::type;
    using I = typename decltype(index)::type;
    AdamGrouped<E, I>(tables_host, tables_device, exp_avg_host, exp_avg_device, exp_avg_sq_host, exp_avg_sq_device,
                      num_tables, row_base, embed_width, ids, rows, total_entries, o, seeds_device, stream);
  });
  if (!known) CUEMBED_C_API_BAD_TYPE();
}

}  // extern "C"
