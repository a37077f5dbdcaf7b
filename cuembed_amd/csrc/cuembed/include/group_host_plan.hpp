// Host-only arithmetic that the entry points on a GROUP of tables share (grouped_backward.hpp, mixed_group_lookup.hpp,
// mixed_group_backward.hpp).  No kernel and no HIP call: everything here runs on the CPU.
//
//   PlanMixedGroupColumns   D, W_max and THE lane rule of a mixed-width group, from one pass over the widths
//   PlanLaneGroups          block and grid of the kernels that give a row to a power-of-two group of at most 64 lanes
#ifndef CUEMBED_INCLUDE_GROUP_HOST_PLAN_HPP_
#define CUEMBED_INCLUDE_GROUP_HOST_PLAN_HPP_

#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "cuembed/include/cuembed_assert.hpp"
#include "cuembed/include/embedding_lookup.hpp"

namespace cuembed {

namespace detail {

//! What one pass over the widths of a mixed-width group gives.
struct MixedGroupColumns {
  int out_width;    //!< D
  int max_width;    //!< W_max
  int lane_bytes;   //!< the launch's lane: 16, 8 or 4
};

//! The lane rule of a mixed-width group, the only copy: the widest of 16 / 8 / 4 bytes that the address bits `bits`
//! (every base pointer of the launch OR-ed), D * elem_bytes, every c_t * elem_bytes and every W_t * elem_bytes allow --
//! with D and W_max.  Host only.
inline MixedGroupColumns PlanMixedGroupColumns(const int* widths_host, const int num_tables, const int elem_bytes,
                                               uintptr_t bits) {
  CUEMBED_ASSERT(widths_host != nullptr && num_tables >= 1 && (elem_bytes == 2 || elem_bytes == 4));
  CUEMBED_ASSERT(bits % 4 == 0);
  int64_t column = 0;
  int max_width = 0;
  for (int t = 0; t < num_tables; ++t) {
    const int64_t row_bytes = static_cast<int64_t>(widths_host[t]) * elem_bytes;
    CUEMBED_ASSERT(widths_host[t] > 0 && row_bytes % 4 == 0);
    column += widths_host[t];                 // (c_{t+1}; the last one is D)
    CUEMBED_ASSERT(column <= INT_MAX);
    bits |= static_cast<uintptr_t>(row_bytes) | static_cast<uintptr_t>(column * elem_bytes);
    if (widths_host[t] > max_width) max_width = widths_host[t];
  }
  return MixedGroupColumns{static_cast<int>(column), max_width, bits % 16 == 0 ? 16 : (bits % 8 == 0 ? 8 : 4)};
}

//! ... the lane bytes alone.
inline int MixedGroupLaneBytesOfBits(const uintptr_t bits, const int* widths_host, const int num_tables,
                                     const int elem_bytes) {
  return PlanMixedGroupColumns(widths_host, num_tables, elem_bytes, bits).lane_bytes;
}

//! Launch shape of a kernel that gives each of `rows` rows to a lane group: the next power of two >= lanes_per_row, at
//! most 64 lanes, kDefaultBlockThreads / group rows per workgroup.
struct LaneGroupShape {
  dim3 block;   //!< (lanes of a group, rows per workgroup, 1)
  dim3 grid;
};

inline LaneGroupShape PlanLaneGroups(const int lanes_per_row, const int rows) {
  int group = 1;
  while (group < lanes_per_row && group < 64) group *= 2;
  const int rows_per_block = kDefaultBlockThreads / group;
  return LaneGroupShape{dim3(group, rows_per_block, 1), dim3((rows + rows_per_block - 1) / rows_per_block, 1, 1)};
}

}  // namespace detail

}  // namespace cuembed

#endif  // CUEMBED_INCLUDE_GROUP_HOST_PLAN_HPP_
