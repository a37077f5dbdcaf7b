// cuembed::CheckIndices (an extension): validate -- and optionally repair -- a batch's indices and offsets ON THE DEVICE,
// in front of the kernels that address table rows with them.
//
// Every row-addressing kernel of this library trusts its indices and offsets ("ids outside their table are a contract
// violation"): one id at or beyond the row count, one negative id, one decreasing offset is an illegal memory access,
// or a silent read of a neighbouring table's rows in a one-storage group.  The host cannot look at the values without a
// read-back, which the training step is built to avoid.  This call looks at them on the device: it never reads a table,
// reads nothing back, allocates nothing, can be captured in a HIP graph, and leaves a four-word report in device memory.
//
// Definitions (tests/index_check_reference.py is exactly this, in numpy):
//   n = num_tables * batch_per_table bags, table-major (bag g = t * batch_per_table + b), as in EmbeddingForwardGrouped.
//   Row counts: row_base[num_tables + 1] (int64, device; the exclusive prefix sum of the tables' row counts), or, with
//   row_base == nullptr, ONE table of num_rows rows.  Every table has at least one row.
//   Offsets (CSR: num_hots == 0, offsets[n + 1]).  Position i in 0 .. n is BAD iff o[i] < 0, or o[i] > nnz, or i > 0 and
//     o[i] < o[i - 1].  No position is bad iff 0 <= o[0] <= o[1] <= ... <= o[n] <= nnz (o[0] != 0 and o[n] != nnz are no
//     errors).  The REPAIRED offsets are the running maximum clamped into [0, nnz]: r[i] = min(nnz, max(0, max_{k<=i} o[k])),
//     always valid, and equal to o exactly when no position is bad.
//   Indices.  The checked range is [r[0], r[n]) (CSR) or [0, nnz) with nnz = n * num_hots (fixed hotness: num_hots > 0,
//     offsets == nullptr).  Position p belongs to the table t with r[t * B] <= p < r[(t + 1) * B], or t = p / (B * num_hots).
//     p is BAD iff indices[p] < 0 or indices[p] >= rows_t, compared in 64 bits.  The repaired index is 0 where bad and
//     unchanged elsewhere; positions outside the checked range are not counted and are copied through.
//   report (int64[4], device): [bad indices, first bad index position or -1, bad offsets, first bad offset position or
//     -1]; "first" = smallest.  The call initialises it on the stream; what it held does not matter.
//   indices_out / offsets_out: each nullptr (report only), its input (in place) or a separate array of the same type
//     (partial overlap is a contract violation).  On a clean batch they are bit-identical copies.
// Arbitrary garbage in either array, INT64_MIN and INT64_MAX included, is a defined input.
//
// Launches, all on `stream`: CSR -- tile maxima of the offsets (+ report init), offsets scan / repair / cuts, index pass;
// fixed hotness -- report init, index pass.  The index pass is skipped for nnz == 0.  Bytes: nnz * sizeof(IndexT) read,
// written once more when repairing out of place (in place only the pieces that hold a bad id are written); the offsets
// are read twice.
//
// Workspace (CSR only: tile maxima, tile ends, cuts), two-phase like BagOrderByLength: work == nullptr stores the bytes
// needed to *lwork and runs nothing (only nnz, num_tables, batch_per_table and num_hots are looked at besides the
// preconditions); a buffer of exactly that size holding anything is enough.  Fixed hotness needs 0 bytes but, like every
// two-phase call, a non-null `work` to run.
#ifndef CUEMBED_INCLUDE_INDEX_CHECK_HPP_
#define CUEMBED_INCLUDE_INDEX_CHECK_HPP_

#include <hip/hip_runtime.h>

#include <climits>
#include <cstddef>
#include <cstdint>

#include "cuembed/include/cuembed_assert.hpp"
#include "cuembed/include/index_check_kernels.hpp"

namespace cuembed {
namespace detail {

struct IndexCheckPlan {
  int64_t positions;   // n + 1 offsets (CSR), 0 otherwise
  int64_t tile_len;
  int tiles;
  size_t tile_bytes;   // one of the two per-tile arrays
  size_t total;
};

inline IndexCheckPlan PlanIndexCheck(const int num_tables, const int batch_per_table, const bool csr) {
  IndexCheckPlan plan = {0, 0, 0, 0, 0};
  if (!csr) return plan;
  plan.positions = static_cast<int64_t>(num_tables) * batch_per_table + 1;
  const int64_t chunks = (plan.positions + kCheckScanChunk - 1) / kCheckScanChunk;
  plan.tile_len = (chunks + kCheckMaxTiles - 1) / kCheckMaxTiles * kCheckScanChunk;
  plan.tiles = static_cast<int>((plan.positions + plan.tile_len - 1) / plan.tile_len);
  const auto align = [](const size_t v) { return (v + 255) / 256 * 256; };
  plan.tile_bytes = align(static_cast<size_t>(plan.tiles) * sizeof(int64_t));
  plan.total = 2 * plan.tile_bytes + align(static_cast<size_t>(num_tables + 1) * sizeof(int64_t));
  return plan;
}

template <typename IndexT, int kLane, bool kCsr>
inline void LaunchIndexCheck(const IndexT* indices, const int64_t nnz, const int64_t* row_base, const int64_t num_rows,
                             const int num_tables, const int64_t per_table, const int64_t* cuts, IndexT* indices_out,
                             unsigned long long* report, hipStream_t stream) {
  const int64_t per_block = static_cast<int64_t>(kCheckThreads) * kLane;
  const unsigned blocks = static_cast<unsigned>((nnz + per_block - 1) / per_block);
  hipLaunchKernelGGL((IndexCheckKernel<IndexT, kLane, kCsr>), dim3(blocks), dim3(kCheckThreads), 0, stream, indices, nnz,
                     row_base, num_rows, num_tables, per_table, cuts, indices_out, report);
}

template <typename IndexT, bool kCsr>
inline void LaunchIndexCheckByAlignment(const IndexT* indices, const int64_t nnz, const int64_t* row_base,
                                        const int64_t num_rows, const int num_tables, const int64_t per_table,
                                        const int64_t* cuts, IndexT* indices_out, unsigned long long* report,
                                        hipStream_t stream) {
  const uintptr_t both = reinterpret_cast<uintptr_t>(indices) | reinterpret_cast<uintptr_t>(indices_out);
  constexpr int kWide = 16 / static_cast<int>(sizeof(IndexT));
  if (both % 16 == 0)
    LaunchIndexCheck<IndexT, kWide, kCsr>(indices, nnz, row_base, num_rows, num_tables, per_table, cuts, indices_out,
                                          report, stream);
  else if (both % 8 == 0 && kWide > 2)
    LaunchIndexCheck<IndexT, 2, kCsr>(indices, nnz, row_base, num_rows, num_tables, per_table, cuts, indices_out, report,
                                      stream);
  else
    LaunchIndexCheck<IndexT, 1, kCsr>(indices, nnz, row_base, num_rows, num_tables, per_table, cuts, indices_out, report,
                                      stream);
}

}  // namespace detail

/**
 * @brief Is this batch safe to hand to the row-addressing kernels?  See the head of this file for the definitions.
 *
 * CUEMBED_ASSERTs, in this order, before any launch: lwork; 1 <= num_tables <= 1023, batch_per_table >= 0 and num_tables *
 * batch_per_table <= INT_MAX; num_hots >= 0 and 0 <= nnz <= 2^38 (detail::kCheckMaxLookups: the index pass is one
 * launch); row_base, or else num_tables == 1 and num_rows >= 1; nnz = n * num_hots (fixed hotness), nnz within OffsetT
 * (CSR) -- then the workspace query returns --; report; indices unless nnz == 0; offsets given exactly for CSR, offsets_out only for CSR; each output null, its input, or disjoint from it;
 * *lwork at least the queried size.
 */
template <typename IndexT, typename OffsetT>
void CheckIndices(const IndexT* indices,
                  const OffsetT* offsets,
                  const int64_t nnz,
                  const int64_t* row_base,
                  const int64_t num_rows,
                  const int num_tables,
                  const int batch_per_table,
                  const int num_hots,
                  int64_t* report,
                  IndexT* indices_out,
                  OffsetT* offsets_out,
                  char* work,
                  size_t* lwork,
                  const hipStream_t stream = 0) {
  CUEMBED_ASSERT(lwork != nullptr);
  CUEMBED_ASSERT(num_tables >= 1 && num_tables <= detail::kCheckMaxTables && batch_per_table >= 0 &&
                 static_cast<int64_t>(num_tables) * batch_per_table <= INT_MAX);
  CUEMBED_ASSERT(num_hots >= 0 && nnz >= 0 && nnz <= detail::kCheckMaxLookups);
  CUEMBED_ASSERT(row_base != nullptr || (num_tables == 1 && num_rows >= 1));
  const bool csr = num_hots == 0;
  const int64_t bags = static_cast<int64_t>(num_tables) * batch_per_table;
  if (csr) CUEMBED_ASSERT(sizeof(OffsetT) == 8 || nnz <= INT32_MAX);
  else CUEMBED_ASSERT(nnz == bags * num_hots);
  const detail::IndexCheckPlan plan = detail::PlanIndexCheck(num_tables, batch_per_table, csr);
  if (work == nullptr) {
    *lwork = plan.total;
    return;
  }
  CUEMBED_ASSERT(row_base != nullptr || (num_tables == 1 && num_rows >= 1));
  CUEMBED_ASSERT(report != nullptr);
  CUEMBED_ASSERT(nnz == 0 || indices != nullptr);
  CUEMBED_ASSERT(csr ? offsets != nullptr : (offsets == nullptr && offsets_out == nullptr));
  {
    const auto apart = [](const void* in, const void* out, const int64_t bytes) {
      const uintptr_t a = reinterpret_cast<uintptr_t>(in), b = reinterpret_cast<uintptr_t>(out);
      return out == nullptr || a == b || a + static_cast<uintptr_t>(bytes) <= b || b + static_cast<uintptr_t>(bytes) <= a;
    };
    CUEMBED_ASSERT(apart(indices, indices_out, nnz * static_cast<int64_t>(sizeof(IndexT))));
    CUEMBED_ASSERT(apart(offsets, offsets_out, (bags + 1) * static_cast<int64_t>(sizeof(OffsetT))));
  }
  CUEMBED_ASSERT(*lwork >= plan.total);
  auto* words = reinterpret_cast<unsigned long long*>(report);
  const int64_t* cuts = nullptr;
  if (csr) {
    int64_t* tile_max = reinterpret_cast<int64_t*>(work);
    int64_t* tile_last = reinterpret_cast<int64_t*>(work + plan.tile_bytes);
    int64_t* cuts_out = reinterpret_cast<int64_t*>(work + 2 * plan.tile_bytes);
    hipLaunchKernelGGL((detail::OffsetsTileMaxKernel<OffsetT>), dim3(plan.tiles), dim3(detail::kCheckThreads), 0, stream,
                       offsets, plan.positions, plan.tile_len, tile_max, tile_last, words);
    hipLaunchKernelGGL((detail::OffsetsRepairKernel<OffsetT>), dim3(plan.tiles), dim3(detail::kCheckThreads), 0, stream,
                       offsets, plan.positions, nnz, plan.tile_len, tile_max, tile_last, num_tables, batch_per_table,
                       offsets_out, cuts_out, words);
    cuts = cuts_out;
  } else {
    hipLaunchKernelGGL((detail::ClearIndexReportKernel<0>), dim3(1), dim3(64), 0, stream, words);
  }
  if (nnz == 0) return;
  const int64_t per_table = static_cast<int64_t>(batch_per_table) * num_hots;
  if (csr)
    detail::LaunchIndexCheckByAlignment<IndexT, true>(indices, nnz, row_base, num_rows, num_tables, per_table, cuts,
                                                      indices_out, words, stream);
  else
    detail::LaunchIndexCheckByAlignment<IndexT, false>(indices, nnz, row_base, num_rows, num_tables, per_table, cuts,
                                                       indices_out, words, stream);
}

}  // namespace cuembed

#endif  // CUEMBED_INCLUDE_INDEX_CHECK_HPP_
