// C ABI: the sparse optimizer step on a group of tables of DIFFERENT widths = explicit instantiations of
// cuembed::SparseRowUpdateMixedGroup / SparseRowAdamMixedGroup: element type x id type x lane width x rule, one kernel
// each, round to nearest.  (An extension: the reference ends at the gradient and takes one table.)
#include "c_api_optimizer_adam_common.hpp"
#include "cuembed/include/mixed_group_sparse_update.hpp"

namespace {

template <typename T>
T* const* Mutable(const void* const* p) {
  return reinterpret_cast<T* const*>(const_cast<void* const*>(p));
}

}  // namespace

extern "C" {

void cuembed_sparse_row_update_mixed_group(const void* const* tables_host, const void* const* tables_device,
                                           const void* const* state_host, const void* const* state_device,
                                           const int* widths_host, const int* widths_device, int num_tables,
                                           int elem_type, int max_width, const int64_t* row_base, int rule,
                                           const void* ids, int index_type, const void* rows, int64_t total_entries,
                                           int64_t num_rows, const void* count_word, int count_word_is_64,
                                           const void* last_id, float lr, const float* lr_device, float eps,
                                           cuembed_stream_t stream) {
  const cuembed::SparseUpdateOptions o = cuembed_c_api::UpdateOptions(rule, total_entries, 1, num_rows, count_word,
                                                                      count_word_is_64, last_id, lr, lr_device, eps);
  const bool known = cuembed_c_api::DispatchTypes<true>(elem_type, index_type, [&](auto elem, auto index) {
    using E = typename decltype(elem)::type;
    using I = typename decltype(index)::type;
    cuembed::SparseRowUpdateMixedGroup<E, I>(
        reinterpret_cast<const E* const*>(tables_host), Mutable<E>(tables_device),
        reinterpret_cast<const float* const*>(state_host), Mutable<float>(state_device), widths_host, widths_device,
        num_tables, row_base, max_width, static_cast<const I*>(ids), static_cast<const E*>(rows), total_entries, o,
        cuembed_c_api::Stream(stream));
  });
  if (!known) CUEMBED_C_API_BAD_TYPE();
}

void cuembed_sparse_row_adam_mixed_group(const void* const* tables_host, const void* const* tables_device,
                                         const void* const* exp_avg_host, const void* const* exp_avg_device,
                                         const void* const* exp_avg_sq_host, const void* const* exp_avg_sq_device,
                                         const int* widths_host, const int* widths_device, int num_tables, int elem_type,
                                         int max_width, const int64_t* row_base, int rule, const void* ids,
                                         int index_type, const void* rows, int64_t total_entries, int64_t num_rows,
                                         const void* count_word, int count_word_is_64, const void* last_id, float lr,
                                         const float* lr_device, float bias_factor, const float* bias_factor_device,
                                         float beta1, float one_minus_beta1, float beta2, float one_minus_beta2,
                                         float eps, float weight_decay, cuembed_stream_t stream) {
  const cuembed::SparseAdamOptions o = cuembed_c_api::AdamOptions(
      rule, total_entries, 1, num_rows, count_word, count_word_is_64, last_id, lr, lr_device, bias_factor,
      bias_factor_device, beta1, one_minus_beta1, beta2, one_minus_beta2, eps, weight_decay);
  const bool known = cuembed_c_api::DispatchTypes<true>(elem_type, index_type, [&](auto elem, auto index) {
    using E = typename decltype(elem)::type;
    using I = typename decltype(index)::type;
    cuembed::SparseRowAdamMixedGroup<E, I>(
        reinterpret_cast<const E* const*>(tables_host), Mutable<E>(tables_device),
        reinterpret_cast<const float* const*>(exp_avg_host), Mutable<float>(exp_avg_device),
        reinterpret_cast<const float* const*>(exp_avg_sq_host), Mutable<float>(exp_avg_sq_device), widths_host,
        widths_device, num_tables, row_base, max_width, static_cast<const I*>(ids), static_cast<const E*>(rows),
        total_entries, o, cuembed_c_api::Stream(stream));
  });
  if (!known) CUEMBED_C_API_BAD_TYPE();
}

void cuembed_mixed_group_update_launch_shape(const int* widths_host, int num_tables, int elem_type,
                                             int64_t total_entries, int state_tensors, size_t pointer_bits,
                                             size_t state_pointer_bits, int compute_units, int* out, int* per_table) {
  namespace d = cuembed::detail;
  d::DeviceShape dev = compute_units > 0 ? d::Mi355xShape() : d::CurrentDeviceShape();
  if (compute_units > 0) dev.compute_units = compute_units;
  const int elem_bytes = elem_type == CUEMBED_F32 ? 4 : 2;
  const int lane_bytes = d::MixedGroupUpdateLaneBytes(widths_host, num_tables, elem_bytes, pointer_bits, state_pointer_bits);
  out[0] = lane_bytes / elem_bytes;
  out[1] = static_cast<int>(d::PlanMixedGroupUpdate(total_entries, dev));
  out[2] = d::MixedGroupUpdateLdsBytes(num_tables, state_tensors);
  for (int t = 0; t < num_tables; ++t)
    d::MixedGroupPassOf(widths_host[t] * elem_bytes / lane_bytes, &per_table[2 * t], &per_table[2 * t + 1]);
}

}  // extern "C"
