// C ABI: the sparse optimizer step = explicit instantiations of cuembed::SparseRowUpdate (an extension: the
// reference ends at the gradient).
#include "c_api_optimizer_common.hpp"

extern "C" {

void cuembed_sparse_row_update(void* table, int elem_type, int embed_width, float* state, int rule, const void* ids,
                               int index_type, const void* rows, int64_t piece_rows, int pieces, int64_t num_rows,
                               const void* counts, int counts_are_int64, const void* last_id, float lr,
                               const float* lr_device, float eps, cuembed_stream_t stream) {
  // (round to nearest only: the stochastic kernels are c_api_optimizer_stochastic.hip's)
  const cuembed::SparseUpdateOptions o = cuembed_c_api::UpdateOptions(rule, piece_rows, pieces, num_rows, counts,
                                                                      counts_are_int64, last_id, lr, lr_device, eps);
  const bool known = cuembed_c_api::DispatchTypes<true>(elem_type, index_type, [&](auto elem, auto index) {
    using E = typename decltype(elem)::type;
    using I = typename decltype(index)::type;
    cuembed_c_api::Update<E, I, cuembed::UpdateRoundings::kNearestOnly>(table, state, embed_width, ids, rows, o, stream);
  });
  if (!known) CUEMBED_C_API_BAD_TYPE();
}

void cuembed_sparse_row_update_placed(void* table, int elem_type, int embed_width, float* state, int rule,
                                      const void* ids, int index_type, const void* rows, int64_t piece_rows, int pieces,
                                      int64_t num_rows, const void* counts, int counts_are_int64, const void* last_id,
                                      float lr, const float* lr_device, float eps, cuembed_stream_t stream,
                                      const int64_t* state_ids) {
  const cuembed::SparseUpdateOptions o = cuembed_c_api::UpdateOptions(rule, piece_rows, pieces, num_rows, counts,
                                                                      counts_are_int64, last_id, lr, lr_device, eps);
  const bool known = cuembed_c_api::DispatchTypes<true>(elem_type, index_type, [&](auto elem, auto index) {
    using E = typename decltype(elem)::type;
    using I = typename decltype(index)::type;
    cuembed::SparseRowUpdate<E, I, cuembed::UpdateRoundings::kNearestOnly>(
        static_cast<E*>(table), state, embed_width, static_cast<const I*>(ids), static_cast<const E*>(rows), o,
        cuembed_c_api::Stream(stream), state_ids);
  });
  if (!known) CUEMBED_C_API_BAD_TYPE();
}

void cuembed_sparse_row_update_launch_shape(int elem_type, int embed_width, int64_t total_entries, int compute_units,
                                            int* out) {
  cuembed::detail::DeviceShape dev =
      compute_units > 0 ? cuembed::detail::Mi355xShape() : cuembed::detail::CurrentDeviceShape();
  if (compute_units > 0) dev.compute_units = compute_units;
  const int row_bytes = embed_width * (elem_type == CUEMBED_F32 ? 4 : 2);
  const int lane_bytes = row_bytes % 16 == 0 ? 16 : (row_bytes % 8 == 0 ? 8 : 4);   // (aligned buffers)
  const cuembed::detail::UpdateShape s = cuembed::detail::PlanUpdate(row_bytes / lane_bytes, total_entries, dev);
  out[0] = lane_bytes;
  out[1] = s.lanes_per_row;
  out[2] = s.group;
  out[3] = s.chunks;
  out[4] = static_cast<int>(s.grid);
}

}  // extern "C"
