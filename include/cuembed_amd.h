/* ============================================================================
 * cuembed_amd.h -- C ABI of the MI355X-native embedding-lookup library.
 *
 * This is the drop-in boundary for foreign-function bindings (ctypes, cgo, JNI,
 * a torch extension ...).  Every entry point is an explicit instantiation of one
 * of the header-only C++ templates in cuembed_amd/csrc/cuembed/include/, which in
 * turn mirror the reference's host API one to one:
 *
 *   cuembed_embedding_forward_*              cuembed::EmbeddingForward
 *        reference: cuembed/include/embedding_lookup.cuh:245-308
 *        (instantiation list: utils/src/embedding_gpu_forward.cu:69-76,
 *         int64 offsets: examples/pytorch/cuembed_embedding.cu:39-49)
 *   cuembed_embedding_backward_*             cuembed::EmbeddingBackward
 *        reference: cuembed/include/embedding_lookup.cuh:423-483
 *        (instantiations: utils/src/embedding_gpu_backward.cu:84-87)
 *   cuembed_transpose_*                      cuembed::Transpose
 *        reference: cuembed/include/index_transforms.cuh:224-250
 *        (instantiations: utils/src/embedding_gpu_transpose.cu:95-98)
 *   cuembed_compute_compressed_grad_indices_* cuembed::ComputeCompressedGradIndices
 *        reference: cuembed/include/index_transforms.cuh:278-323
 *   cuembed_extract_row_ids_from_fixed_*     cuembed::ExtractRowIdsFromFixed
 *        reference: cuembed/include/index_transforms.cuh:45-55
 *   cuembed_extract_row_ids_from_csr_*       cuembed::ExtractRowIdsFromCSR
 *        reference: cuembed/include/index_transforms.cuh:66-74
 *   cuembed_extract_row_ids_for_concat_*     cuembed::ExtractRowIdsForConcat
 *        reference: cuembed/include/index_transforms.cuh:85-93
 *
 * Conventions (identical to the reference's):
 *   - all data pointers are DEVICE pointers owned by the caller; the library
 *     allocates nothing and keeps no state between calls;
 *   - every call only enqueues work on `stream` (a hipStream_t passed as void*;
 *     NULL = the default stream) and returns immediately;
 *   - functions return void; violating the argument contract prints
 *     "Check failed: ..." on stderr and aborts the process;
 *   - fp16 data is IEEE binary16 (`__half`), bf16 data is bfloat16 (`__hip_bfloat16`), both
 *     passed as void pointers here;
 *   - Transpose / ComputeCompressedGradIndices are two-phase: call with
 *     work == NULL to receive the scratch size in *lwork, then again with a
 *     scratch buffer of at least that size.  The same holds for every other
 *     call with `work` / `lwork` parameters (the sample-blocked and remapped
 *     transposes, cuembed_bag_order_by_length, cuembed_row_cache_prefetch*).
 *     `work` may hold anything on entry -- nothing has to be zeroed, and a buffer
 *     may be re-used between calls of any size and type -- and its contents after
 *     the call are unspecified.  No byte outside [work, work + queried size) and
 *     outside the named outputs is written, and inputs are never written.  `work`
 *     must be aligned to 8 bytes (hipMalloc gives 256): every region inside it
 *     starts at a multiple of 256 bytes from `work`, and the widest access made
 *     to one is a 64-bit word.
 *
 * Suffix grammar:  _{f32|f16|bf16}  element type of table / gradient / weights
 *                  _{i32|i64}  lookup-index and sample-id type
 *                  _{o32|o64}  CSR offset type
 * ==========================================================================*/
#ifndef CUEMBED_AMD_H_
#define CUEMBED_AMD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* CombineMode values (reference: embedding_lookup_types.cuh:29). */
enum { CUEMBED_SUM = 0, CUEMBED_MEAN = 1, CUEMBED_CONCAT = 2 };
/* type codes for the generic (runtime-dispatched) entry points */
enum { CUEMBED_F32 = 0, CUEMBED_F16 = 1, CUEMBED_BF16 = 2 /* extension */ };
enum { CUEMBED_I32 = 0, CUEMBED_I64 = 1 };

typedef void* cuembed_stream_t; /* hipStream_t */

/* ---- forward ------------------------------------------------------------ */
/* fixed hotness: offsets == NULL, num_hots > 0; CSR: offsets[batch_size + 1],
 * num_hots == 0.  weights may be NULL.  ret: [batch x width] for sum/mean,
 * [batch x num_hots x width] for concat (fixed hotness, unweighted only).
 * fp16_math != 0 accumulates an fp16 table in fp16 (ignored for fp32). */
#define CUEMBED_DECLARE_FORWARD(SUFFIX, ELEM, INDEX, OFFSET)                           \
  void cuembed_embedding_forward_##SUFFIX(                                             \
      const ELEM* params, int embed_width, const INDEX* indices, const OFFSET* offsets, \
      const ELEM* weights, int batch_size, int num_hots, int mode, int fp16_math,      \
      ELEM* ret, cuembed_stream_t stream);
CUEMBED_DECLARE_FORWARD(f32_i32_o32, float, int32_t, int32_t)
CUEMBED_DECLARE_FORWARD(f32_i32_o64, float, int32_t, int64_t)
CUEMBED_DECLARE_FORWARD(f32_i64_o32, float, int64_t, int32_t)
CUEMBED_DECLARE_FORWARD(f32_i64_o64, float, int64_t, int64_t)
CUEMBED_DECLARE_FORWARD(f16_i32_o32, void, int32_t, int32_t)
CUEMBED_DECLARE_FORWARD(f16_i32_o64, void, int32_t, int64_t)
CUEMBED_DECLARE_FORWARD(f16_i64_o32, void, int64_t, int32_t)
CUEMBED_DECLARE_FORWARD(f16_i64_o64, void, int64_t, int64_t)
/* bf16 tables (extension; fp32 accumulation, fp16_math ignored) */
CUEMBED_DECLARE_FORWARD(bf16_i32_o32, void, int32_t, int32_t)
CUEMBED_DECLARE_FORWARD(bf16_i32_o64, void, int32_t, int64_t)
CUEMBED_DECLARE_FORWARD(bf16_i64_o32, void, int64_t, int32_t)
CUEMBED_DECLARE_FORWARD(bf16_i64_o64, void, int64_t, int64_t)
#undef CUEMBED_DECLARE_FORWARD

/* ---- backward ----------------------------------------------------------- */
/* COO lookups sorted by index (output of transpose).  Full gradient:
 * transpose_remapped_indices == NULL, grad_embedding has num_grad_embedding_rows
 * = table rows.  Compressed: remapped indices given, grad_embedding has
 * num_unique rows and inverse_mapping[num_unique] is written.  The gradient
 * buffer must be zero before the scatter: skip_grad_init != 0 means the caller
 * already zeroed it, otherwise the call zeroes it first.
 *
 * ARITHMETIC (deviation from the reference for 16-bit gradients).  The reference
 * accumulates in GradT: with fp16 every product grad_y * weight and every partial sum
 * is rounded to fp16 (embedding_lookup_ops.cuh:636-645, embedding_lookup_cpu.hpp:139-142).
 * Here the products and the partial sum of a run are kept in fp32 and rounded to GradT
 * once per flush: one flush for a run inside a workgroup; a run that crosses workgroups
 * (>= 256 lookups each) is combined with one GradT hardware atomic per workgroup.
 *   - fp32 gradients: same fp32 arithmetic in the same nz order, equal up to where a run
 *     is cut into partial sums (a few ulps of the summed magnitudes);
 *   - fp16/bf16 gradients: bit-identical to the reference whenever all partial sums are
 *     exactly representable in GradT (the reference's own test data: integer grad_y,
 *     weights 0.5/0.25); otherwise within 1e-2 (fp16) of the reference relative to
 *     sum_j |grad_y_j * w_j|, and never further from the exact sum than the reference is.
 *     Runs longer than ~2^11 lookups are where the two part for good: the reference's fp16
 *     running sum stalls, this one does not.  Measured in tests/test_gpu_backward_tolerance.py. */
#define CUEMBED_DECLARE_BACKWARD(SUFFIX, ELEM, INDEX)                                     \
  void cuembed_embedding_backward_##SUFFIX(                                               \
      const ELEM* grad_y, int embed_width, int num_grad_embedding_rows, int nnz,          \
      const INDEX* transpose_indices, const INDEX* transpose_sample_ids,                  \
      const INDEX* transpose_remapped_indices, const ELEM* transpose_weights,             \
      int skip_grad_init, ELEM* grad_embedding, INDEX* inverse_mapping,                   \
      cuembed_stream_t stream);
CUEMBED_DECLARE_BACKWARD(f32_i32, float, int32_t)
CUEMBED_DECLARE_BACKWARD(f32_i64, float, int64_t)
CUEMBED_DECLARE_BACKWARD(f16_i32, void, int32_t)
CUEMBED_DECLARE_BACKWARD(f16_i64, void, int64_t)
CUEMBED_DECLARE_BACKWARD(bf16_i32, void, int32_t)
CUEMBED_DECLARE_BACKWARD(bf16_i64, void, int64_t)
#undef CUEMBED_DECLARE_BACKWARD

/* ---- transpose ---------------------------------------------------------- */
/* Stable sort of (rows[i] [, weights[i]]) by key cols[i]; callers pass
 * rows = sample ids, cols = lookup indices.  transpose_rows receives the sorted
 * lookup indices, transpose_cols the sample ids, transpose_weights the weights
 * (untouched when weights == NULL).  The suffix names the index type and the
 * WEIGHT type.
 * Generic like the reference's (cub::DeviceRadixSort::SortPairs over all key bits,
 * index_transforms.cuh:108-136): `cols` may hold any value of the index type, keys are
 * ordered as SIGNED numbers (negative keys first); `rows` may hold any value of the
 * index type (int64 rows that are negative or >= 2^32 are carried at full width; the
 * library finds that out on the device).  nnz <= INT_MAX. */
#define CUEMBED_DECLARE_TRANSPOSE(SUFFIX, INDEX, WEIGHT)                                   \
  void cuembed_transpose_##SUFFIX(const INDEX* rows, const INDEX* cols,                    \
                                  const WEIGHT* weights, int nnz, INDEX* transpose_rows,   \
                                  INDEX* transpose_cols, WEIGHT* transpose_weights,        \
                                  char* work, size_t* lwork, cuembed_stream_t stream);
CUEMBED_DECLARE_TRANSPOSE(i32_f32, int32_t, float)
CUEMBED_DECLARE_TRANSPOSE(i64_f32, int64_t, float)
CUEMBED_DECLARE_TRANSPOSE(i32_f16, int32_t, void)
CUEMBED_DECLARE_TRANSPOSE(i64_f16, int64_t, void)
CUEMBED_DECLARE_TRANSPOSE(i32_bf16, int32_t, void)
CUEMBED_DECLARE_TRANSPOSE(i64_bf16, int64_t, void)
#undef CUEMBED_DECLARE_TRANSPOSE

/* ---- compressed-gradient remap ------------------------------------------ */
#define CUEMBED_DECLARE_COMPRESS(SUFFIX, INDEX)                                           \
  void cuembed_compute_compressed_grad_indices_##SUFFIX(                                  \
      const INDEX* indices, int nnz, INDEX* remapped_indices, char* work, size_t* lwork,  \
      cuembed_stream_t stream);
CUEMBED_DECLARE_COMPRESS(i32, int32_t)
CUEMBED_DECLARE_COMPRESS(i64, int64_t)
#undef CUEMBED_DECLARE_COMPRESS

/* ---- row-id extraction -------------------------------------------------- */
#define CUEMBED_DECLARE_EXTRACT(SUFFIX, INDEX)                                            \
  void cuembed_extract_row_ids_from_fixed_##SUFFIX(int batch_size, int num_hots,          \
                                                   INDEX* row_ids, cuembed_stream_t stream); \
  void cuembed_extract_row_ids_for_concat_##SUFFIX(int nnz, INDEX* row_ids,               \
                                                   cuembed_stream_t stream);
CUEMBED_DECLARE_EXTRACT(i32, int32_t)
CUEMBED_DECLARE_EXTRACT(i64, int64_t)
#undef CUEMBED_DECLARE_EXTRACT

#define CUEMBED_DECLARE_EXTRACT_CSR(SUFFIX, INDEX, OFFSET)                                \
  void cuembed_extract_row_ids_from_csr_##SUFFIX(const OFFSET* offsets, int batch_size,   \
                                                 INDEX* row_ids, cuembed_stream_t stream);
CUEMBED_DECLARE_EXTRACT_CSR(i32_o32, int32_t, int32_t)
CUEMBED_DECLARE_EXTRACT_CSR(i32_o64, int32_t, int64_t)
CUEMBED_DECLARE_EXTRACT_CSR(i64_o32, int64_t, int32_t)
CUEMBED_DECLARE_EXTRACT_CSR(i64_o64, int64_t, int64_t)
#undef CUEMBED_DECLARE_EXTRACT_CSR

/* ---- generic entry points (runtime type codes; same semantics) ---------- */
void cuembed_embedding_forward(const void* params, int elem_type, int embed_width,
                               const void* indices, int index_type, const void* offsets,
                               int offset_type, const void* weights, int batch_size,
                               int num_hots, int mode, int fp16_math, void* ret,
                               cuembed_stream_t stream);
/* Extension: with a compressed gradient (transpose_remapped_indices != NULL) num_grad_embedding_rows may
 * be negative = "num_unique is only known on the device" (it is transpose_remapped_indices[nnz-1] + 1):
 * grad_embedding / inverse_mapping must hold at least that many rows (nnz always suffices), rows past
 * the last id are left untouched, and no host read-back is needed between ComputeCompressedGradIndices
 * and EmbeddingBackward.  Applies to the typed entry points as well. */
void cuembed_embedding_backward(const void* grad_y, int elem_type, int embed_width,
                                int num_grad_embedding_rows, int nnz,
                                const void* transpose_indices, const void* transpose_sample_ids,
                                const void* transpose_remapped_indices, int index_type,
                                const void* transpose_weights, int skip_grad_init,
                                void* grad_embedding, void* inverse_mapping,
                                cuembed_stream_t stream);
/* Extension (cuembed::EmbeddingBackwardReferenceSums; opt-in, for verification): cuembed_embedding_backward in the
 * REFERENCE's arithmetic -- product and running sum rounded to the gradient type at every lookup, in nz order, as the
 * CPU reference's loop does (embedding_lookup_cpu.hpp:131-143) -- and therefore bit-identical to it for ANY data
 * (fp16 / bf16 gradients that are not exactly representable, runs of any length), where the default entry points
 * keep fp32 partial sums (ARITHMETIC note above).  WHAT EXACTNESS COSTS: a rounding chain cannot be cut into partial
 * sums, so a table row's run is one chain of dependent additions (short runs: one lane group each; runs of 257 lookups
 * and more: a whole workgroup stages the rows in LDS and one wavefront chains them from there).  At BASELINE config 4
 * (10M x 256, 65,536 x 64 lookups, alpha 1.15: the hottest row is a chain of 65,528) 1.2 ms in fp16 and 1.8 ms in fp32
 * against 0.26 / 0.54 ms for the default entry point on the same data -- 4.5 x and 3.4 x (bench.py: roofline.other_kernels,
 * "cost_of_exactness", with bit_identical_to_oracle checked on non-representable data).
 * num_grad_embedding_rows >= 0; skip_grad_init != 0 adds to what grad_embedding holds. */
void cuembed_embedding_backward_reference_sums(const void* grad_y, int elem_type, int embed_width,
                                               int num_grad_embedding_rows, int nnz,
                                               const void* transpose_indices, const void* transpose_sample_ids,
                                               const void* transpose_remapped_indices, int index_type,
                                               const void* transpose_weights, int skip_grad_init,
                                               void* grad_embedding, void* inverse_mapping,
                                               cuembed_stream_t stream);
void cuembed_transpose(const void* rows, const void* cols, const void* weights, int nnz,
                       int index_type, int weight_type, void* transpose_rows,
                       void* transpose_cols, void* transpose_weights, char* work, size_t* lwork,
                       cuembed_stream_t stream);
/* Extension: as cuembed_transpose, for callers that know all lookup indices are
 * < 2^index_bits (e.g. ceil(log2(num_categories))): the radix sort then skips the
 * always-zero high digits.  index_bits <= 0 means "all bits" (= cuembed_transpose). */
void cuembed_transpose_bounded(const void* rows, const void* cols, const void* weights, int nnz,
                               int index_type, int weight_type, void* transpose_rows,
                               void* transpose_cols, void* transpose_weights, char* work,
                               size_t* lwork, int index_bits, cuembed_stream_t stream);
/* Extension: as cuembed_transpose_bounded, plus a bound on the values in `rows`: int64 rows
 * known to lie in [0, 2^row_bits), row_bits <= 32 (sample ids always do), are moved as 32 bits
 * between the radix passes without the library reading them once more to find out.
 * row_bits <= 0 means "unknown" (= cuembed_transpose_bounded). */
void cuembed_transpose_hinted(const void* rows, const void* cols, const void* weights, int nnz,
                              int index_type, int weight_type, void* transpose_rows,
                              void* transpose_cols, void* transpose_weights, char* work,
                              size_t* lwork, int index_bits, int row_bits, cuembed_stream_t stream);
/* Extension (cuembed::TransposeFixedHotness): cuembed_extract_row_ids_from_fixed +
 * cuembed_transpose_bounded in one call, without materialising the sample ids -- the first radix
 * pass derives the sample id of lookup i as i / num_hots.  Same outputs.  num_hots = 1 is the
 * concat layout (row id = position).  index_bits <= 0: all bits. */
void cuembed_transpose_fixed_hotness(const void* indices, const void* weights, int batch_size,
                                     int num_hots, int index_type, int weight_type,
                                     void* transpose_indices, void* transpose_sample_ids,
                                     void* transpose_weights, char* work, size_t* lwork, int index_bits,
                                     cuembed_stream_t stream);
/* Extension (cuembed::Transpose / TransposeFixedHotness, `sample_blocks`): sample_blocks > 1 CHANGES the
 * result -- the sample-major input is cut into that many consecutive blocks of equal length (whole 4096-element
 * tiles; at most 64) and each block is transposed on its own; the output is the concatenation of the sorted
 * blocks.  For the COMPRESSED gradient only: cuembed_compute_compressed_grad_indices and
 * cuembed_embedding_backward then produce one gradient row per (block, table row) -- a table row looked up from
 * several blocks appears once per block in inverse_mapping (an uncoalesced compressed gradient) -- and while a
 * block is scattered every L2 gathers from 1 / sample_blocks of grad_y (C4: backward 0.258 -> 0.191 ms with 2
 * blocks; 572 k -> 679 k gradient rows).  cuembed_recommended_sample_blocks picks the count (1 = no gain).
 * Never combine with a dense gradient.  Otherwise as cuembed_transpose_hinted / cuembed_transpose_fixed_hotness. */
void cuembed_transpose_sample_blocks(const void* rows, const void* cols, const void* weights, int nnz,
                                     int index_type, int weight_type, void* transpose_rows,
                                     void* transpose_cols, void* transpose_weights, char* work, size_t* lwork,
                                     int index_bits, int row_bits, int sample_blocks, cuembed_stream_t stream);
void cuembed_transpose_fixed_hotness_sample_blocks(const void* indices, const void* weights, int batch_size,
                                                   int num_hots, int index_type, int weight_type,
                                                   void* transpose_indices, void* transpose_sample_ids,
                                                   void* transpose_weights, char* work, size_t* lwork,
                                                   int index_bits, int sample_blocks, cuembed_stream_t stream);
/* Extension (cuembed::Transpose / TransposeFixedHotness, `transpose_remapped_indices`): as the two calls above, and
 * transpose_remapped_indices (nnz entries of the index type; NULL: not wanted) also receives what
 * cuembed_compute_compressed_grad_indices would compute from transpose_rows / transpose_indices -- the same values
 * from the same call.  Up to 4,096 lookups the WHOLE index work (row ids of a fixed-hotness batch, stable sort, remap)
 * is ONE launch of one 1024-thread workgroup (a dependent launch costs 3.5-5 us at these sizes and the
 * reference's sequence is about ten of them, index_transforms.cuh:95-137, :278-323); beyond that the run-head scan's
 * launches follow the sort's on the stream and share `work`. */
void cuembed_transpose_remapped(const void* rows, const void* cols, const void* weights, int nnz,
                                int index_type, int weight_type, void* transpose_rows,
                                void* transpose_cols, void* transpose_weights, void* transpose_remapped_indices,
                                char* work, size_t* lwork, int index_bits, int row_bits, int sample_blocks,
                                cuembed_stream_t stream);
void cuembed_transpose_fixed_hotness_remapped(const void* indices, const void* weights, int batch_size,
                                              int num_hots, int index_type, int weight_type,
                                              void* transpose_indices, void* transpose_sample_ids,
                                              void* transpose_weights, void* transpose_remapped_indices, char* work,
                                              size_t* lwork, int index_bits, int sample_blocks,
                                              cuembed_stream_t stream);
int cuembed_recommended_sample_blocks(int elem_type, int embed_width, int batch_size, int64_t nnz);
/* Lookups per block that the two calls above use: block k = lookups [k * L, (k + 1) * L), L a multiple of 4096
 * (inputs of up to 131,072 lookups are always ONE block). */
int64_t cuembed_transpose_sample_block_length(int64_t nnz, int sample_blocks);
void cuembed_compute_compressed_grad_indices(const void* indices, int nnz, int index_type,
                                             void* remapped_indices, char* work, size_t* lwork,
                                             cuembed_stream_t stream);
/* Extension (cuembed::ComputeCompressedGradIndicesBlocked + cuembed::EmbeddingBackward(..., sample_blocks,
 * block_row_ids)): the REFERENCE's compressed gradient -- num_unique ascending rows, the inverse_mapping of the
 * fully sorted order (embedding_lookup.cuh:423-483, index_transforms.cuh:278-323) -- computed from a
 * sample-blocked order, so that the backward gathers grad_y block by block (see cuembed_transpose_sample_blocks).
 *   cuembed_compute_compressed_grad_indices_blocked: `indices` = transpose_rows of a transpose with the SAME nnz
 *     and sample_blocks.  remapped_indices[i] = number of the (block, table row) pair of lookup i (ids count up
 *     through the array; a new one where the index changes or a block begins).  block_row_ids[pair] (room for nnz
 *     uint32 always suffices) = rank of that table row among all distinct rows of the array (= the id the fully
 *     sorted order assigns), with bit 30 set when the row also occurs in an earlier block.  *num_unique (device
 *     word, may be NULL) = number of distinct rows.  At most 8 blocks, nnz < 2^30.  With one block (sample_blocks
 *     <= 1 or nnz <= 131072) remapped_indices is cuembed_compute_compressed_grad_indices' and block_row_ids is
 *     left alone.  Two-phase workspace query.
 *   cuembed_embedding_backward_blocked: as cuembed_embedding_backward with a compressed gradient, for that COO,
 *     those remapped indices and that table: one stream-ordered launch per block; a run whose row an earlier block
 *     already stored is added to it (read-modify-write; float atomic when the run crosses workgroups).
 *     num_grad_embedding_rows = num_unique, or negative when it is only known on the device (buffers of
 *     min(nnz, table rows) rows then suffice).  fp32: the sum of a table row is taken block by block; fp16 /
 *     bf16: one rounding per block (ARITHMETIC note above applies per block). */
void cuembed_compute_compressed_grad_indices_blocked(const void* indices, int nnz, int index_type,
                                                     int sample_blocks, void* remapped_indices,
                                                     uint32_t* block_row_ids, uint32_t* num_unique,
                                                     char* work, size_t* lwork, cuembed_stream_t stream);
void cuembed_embedding_backward_blocked(const void* grad_y, int elem_type, int embed_width,
                                        int num_grad_embedding_rows, int nnz,
                                        const void* transpose_indices, const void* transpose_sample_ids,
                                        const void* transpose_remapped_indices, int index_type,
                                        const void* transpose_weights, int skip_grad_init,
                                        void* grad_embedding, void* inverse_mapping, int sample_blocks,
                                        const uint32_t* block_row_ids, cuembed_stream_t stream);
/* Extension: cuembed_embedding_backward_blocked (sample_blocks <= 1, block_row_ids NULL: cuembed_embedding_backward)
 * with a CAPACITY for the device-side row count.  With num_grad_embedding_rows < 0 only the device knows how many rows
 * the compressed gradient has; capacity_rows > 0 states how many rows grad_embedding and inverse_mapping really hold.
 * If the count exceeds it, nothing is written (per launch: a sample-blocked call may have written its earlier blocks)
 * and *capacity_overflow -- a device word the caller zeroed once; may be NULL -- is OR-ed with 1: a sticky flag to read
 * back whenever convenient instead of a silent overrun.  capacity_rows = 0: unchecked (the other entry points).
 * pad_to_capacity != 0 (needs capacity_rows > 0, num_grad_embedding_rows < 0, skip_grad_init == 0, one block): the
 * rows from the device-side count up to capacity_rows are zeroed and their inverse_mapping entries set to rows of
 * the batch, different ones in turn (entry i names the row of entry (i - count) mod count) -- (inverse_mapping, grad_embedding) over all capacity_rows entries is then a valid uncoalesced
 * COO gradient (coalescing it gives the reference's) that needs no read-back of the count at all. */
void cuembed_embedding_backward_bounded(const void* grad_y, int elem_type, int embed_width,
                                        int num_grad_embedding_rows, int nnz,
                                        const void* transpose_indices, const void* transpose_sample_ids,
                                        const void* transpose_remapped_indices, int index_type,
                                        const void* transpose_weights, int skip_grad_init,
                                        void* grad_embedding, void* inverse_mapping, int sample_blocks,
                                        const uint32_t* block_row_ids, int capacity_rows,
                                        uint32_t* capacity_overflow, int pad_to_capacity, cuembed_stream_t stream);
void cuembed_extract_row_ids_from_fixed(int batch_size, int num_hots, int index_type,
                                        void* row_ids, cuembed_stream_t stream);
void cuembed_extract_row_ids_from_csr(const void* offsets, int offset_type, int batch_size,
                                      int index_type, void* row_ids, cuembed_stream_t stream);
void cuembed_extract_row_ids_for_concat(int nnz, int index_type, void* row_ids,
                                        cuembed_stream_t stream);

/* ---- extension: table-row caching hook (cuembed::TranslateIndicesForRowCache) ------------ */
/* For tables that live outside this GPU's HBM (pinned host memory, a peer) with hot rows copied
 * to a device buffer `cache_rows`: translated[i] = slot_of_row[indices[i]] >= 0 ?
 * cache_row_offset + slot : indices[i], with cache_row_offset = (cache_rows - params) / embed_width
 * in elements (the buffers must differ by a whole number of rows).  cuembed_embedding_forward with
 * index_type = CUEMBED_I64 on `translated` and the table's own `params` pointer then reads cached
 * rows from HBM and the rest from the table -- same kernel, same bits.  slot_of_row: one int32 per
 * table row (num_rows entries), -1 = not cached; indices outside [0, num_rows) pass through unchanged. */
void cuembed_translate_indices_for_row_cache(const void* indices, int index_type, int64_t nnz,
                                             const int32_t* slot_of_row, int64_t num_rows,
                                             int64_t cache_row_offset, int64_t* translated,
                                             cuembed_stream_t stream);
/* The same translation for up to three planes of one cache in ONE launch (cuembed::TranslateIndicesForRowCachePlanes):
 * a table behind the device-managed row cache whose optimizer state rides on the cache slots has a cached plane per
 * tensor, each a whole number of its own rows away from its home tensor.  slot_of_row is read once per index and
 * translatedP[i] = slot >= 0 ? cache_row_offsetP + slot : indices[i] for P = 0, 1, 2; a NULL output is skipped.  Per
 * output exactly the call above: indices outside [0, num_rows) pass through unchanged. */
void cuembed_translate_indices_for_row_cache_planes(const void* indices, int index_type, int64_t nnz,
                                                    const int32_t* slot_of_row, int64_t num_rows,
                                                    int64_t cache_row_offset0, int64_t* translated0,
                                                    int64_t cache_row_offset1, int64_t* translated1,
                                                    int64_t cache_row_offset2, int64_t* translated2,
                                                    cuembed_stream_t stream);

/* ---- extension: device-managed row cache (cuembed::RowCachePrefetch / RowCacheFlush, row_cache.hpp) ----
 * A set-associative LRU write-back cache behind the hook above: num_sets sets of 64 ways in the device buffer
 * cache_rows ([num_sets * 64] rows of row_bytes bytes, a whole number of rows away from `table`), filled and evicted on
 * the device from a batch's own indices.  Device state, owned by the caller: tags int64 [num_sets * 64] (-1 = empty),
 * stamps uint32 [num_sets * 64] (0 = never used), dirty uint8 [num_sets * 64], slot_of_row int32 [num_rows] (-1 = not
 * cached; what cuembed_translate_indices_for_row_cache reads), words uint64 [16]: [0] clock (set it to 1 first),
 * [1] hits, [2] misses, [3] evictions, [4] write-backs, [5] unplaced rows, [6] moves of the running prefetch,
 * [7] valid lookups of the last prefetch, [8] overflow flag.
 * cuembed_row_cache_prefetch, with t the clock and D the distinct rows of the valid lookups inside [0, num_rows):
 * hits first (every resident row of D gets stamp t, and its dirty byte when for_update), then the misses of each set
 * in ascending row id, each taking the way with the smallest (stamp, way) among ways with stamp < t -- none: the row
 * stays uncached, words[5] += 1 --; a valid dirty victim is stored to the table before the new row is loaded; then
 * clock += 1.  Valid lookups: the first num_valid (>= 0, host-known; else pass -1), or *count (one device word, int32,
 * or int64 with count_is_int64 != 0), or *last_id + 1 (one device word of index_type); a count outside [0, nnz] counts
 * as 0.  work == NULL: *lwork receives the bytes needed (cuembed_row_cache_workspace_bytes), nothing runs.
 * cuembed_row_cache_flush stores every dirty row to the table and clears the dirty bytes.  cuembed_cache_set_of is
 * the set of a row (host arithmetic).  Stream-ordered, no read-back. */
size_t cuembed_row_cache_workspace_bytes(int64_t nnz, int64_t num_rows, int num_sets);
void cuembed_row_cache_prefetch(void* table, void* cache_rows, int64_t row_bytes, int64_t num_rows, int num_sets,
                                int64_t* tags, uint32_t* stamps, void* dirty, int32_t* slot_of_row, uint64_t* words,
                                const void* indices, int index_type, int64_t nnz, int64_t num_valid, const void* count,
                                int count_is_int64, const void* last_id, int for_update, char* work, size_t* lwork,
                                cuembed_stream_t stream);
void cuembed_row_cache_flush(void* table, void* cache_rows, int64_t row_bytes, int64_t num_rows, int num_sets,
                             int64_t* tags, uint32_t* stamps, void* dirty, int32_t* slot_of_row, uint64_t* words,
                             cuembed_stream_t stream);
int cuembed_cache_set_of(int64_t row, int num_sets);
/* The same two calls for a cache with a STATE PLANE: fp32 optimizer state that rides on the cache slots.  state: the
 * host side (pinned), [num_rows] rows of state_row_bytes bytes -- 4 * width for Adagrad's accumulator, 4 for row-wise
 * Adagrad's word --; state_cache: [num_sets * 64] such rows in HBM, a whole number of state rows away from `state`.
 * A state row moves with its table row: host -> cache on every fill (for_update or not), cache -> host when a dirty
 * row is evicted or flushed.  One dirty byte covers both planes and the counters count rows, not planes.
 * cuembed_translate_indices_for_row_cache with cache_row_offset = (state_cache - state) / state_row_bytes gives the
 * state_ids of cuembed_sparse_row_update_placed.  state_row_bytes == 0: no state plane, the calls above. */
void cuembed_row_cache_prefetch_with_state(void* table, void* cache_rows, int64_t row_bytes, int64_t num_rows,
                                           int num_sets, int64_t* tags, uint32_t* stamps, void* dirty,
                                           int32_t* slot_of_row, uint64_t* words, const void* indices, int index_type,
                                           int64_t nnz, int64_t num_valid, const void* count, int count_is_int64,
                                           const void* last_id, int for_update, char* work, size_t* lwork,
                                           cuembed_stream_t stream, float* state, float* state_cache,
                                           int64_t state_row_bytes);
void cuembed_row_cache_flush_with_state(void* table, void* cache_rows, int64_t row_bytes, int64_t num_rows, int num_sets,
                                        int64_t* tags, uint32_t* stamps, void* dirty, int32_t* slot_of_row,
                                        uint64_t* words, cuembed_stream_t stream, float* state, float* state_cache,
                                        int64_t state_row_bytes);
/* The same two calls for a cache with TWO state planes (the Adam family: state = exp_avg, state2 = exp_avg_sq, 4 * width
 * bytes a row, or 4 for row-wise Adam's word).  state2 / state2_cache are laid out and moved exactly like state /
 * state_cache: with its table row on every fill, every dirty eviction and every flush, the second plane first, then the
 * first, then the table's rows; the table's move alone clears the dirty bytes and counts the write-backs.  One dirty
 * byte covers all planes, the counters count rows.  cuembed_translate_indices_for_row_cache_planes gives the three id
 * arrays of cuembed_sparse_row_adam_placed.  state2_row_bytes == 0: one plane, the calls above; a second plane without
 * a first (state_row_bytes == 0) aborts. */
void cuembed_row_cache_prefetch_with_states(void* table, void* cache_rows, int64_t row_bytes, int64_t num_rows,
                                            int num_sets, int64_t* tags, uint32_t* stamps, void* dirty,
                                            int32_t* slot_of_row, uint64_t* words, const void* indices, int index_type,
                                            int64_t nnz, int64_t num_valid, const void* count, int count_is_int64,
                                            const void* last_id, int for_update, char* work, size_t* lwork,
                                            cuembed_stream_t stream, float* state, float* state_cache,
                                            int64_t state_row_bytes, float* state2, float* state2_cache,
                                            int64_t state2_row_bytes);
void cuembed_row_cache_flush_with_states(void* table, void* cache_rows, int64_t row_bytes, int64_t num_rows,
                                         int num_sets, int64_t* tags, uint32_t* stamps, void* dirty,
                                         int32_t* slot_of_row, uint64_t* words, cuembed_stream_t stream, float* state,
                                         float* state_cache, int64_t state_row_bytes, float* state2,
                                         float* state2_cache, int64_t state2_row_bytes);

/* ---- extension: gradient w.r.t. the per-lookup weights ---------------------- */
/* grad_weights[s, j] = dot(params[indices[s, j], :], grad_y[s, :]); one entry per lookup;
 * index layouts as in cuembed_embedding_forward (cuembed::EmbeddingWeightGrad). */
void cuembed_embedding_weight_grad(const void* params, int elem_type, int embed_width,
                                   const void* indices, int index_type, const void* offsets,
                                   int offset_type, const void* grad_y, int batch_size, int num_hots,
                                   void* grad_weights, cuembed_stream_t stream);

/* ---- options ------------------------------------------------------------- */
/* cuembed::SetForwardReductionOrder / GetForwardReductionOrder (this library's addition):
 * 0 = sequential (default; bit-identical to the reference for every batch size),
 * 1 = small batches may split a sample's hotness loop over several wavefronts and combine
 *     partial rows through LDS (same result up to fp rounding, much faster for small batches). */
void cuembed_set_forward_reduction_order(int order);
int cuembed_get_forward_reduction_order(void);
/* cuembed::SetForwardRowLoadPolicy / GetForwardRowLoadPolicy (extension; the reference has no such knob,
 * embedding_lookup_kernels.cuh:34-77).  Never changes a result.
 * 0 = default: ordinary table-row loads (rows stay in L2 / Infinity Cache; right whenever rows are re-used),
 * 1 = streaming: non-temporal row loads for batches in which (nearly) every lookup hits a different row of a table
 *     far larger than the caches -- the HBM-bound case (C2 shape with uniform indices: 0.379 -> 0.355 ms); with
 *     re-use it is much slower (alpha = 1.15: 0.136 -> 0.222 ms).  sum / mean only.
 * Both setters change PROCESS-WIDE defaults used by the reference-shaped entry points (initial values:
 * CUEMBED_FORWARD_ORDER=split, CUEMBED_FORWARD_ROW_LOADS=streaming).  A caller that shares its process with
 * other users of the library passes the options per call instead: */
void cuembed_set_forward_row_load_policy(int policy);
int cuembed_get_forward_row_load_policy(void);
/* cuembed::SetForwardWideLoad (tuning / tests; never changes a result).  Small batches of sum / mean lookups take a
 * kernel with one sample per workgroup that requests a whole bag's rows at once and pools them in lookup order out of LDS
 * (bit-identical to the sequential kernel; the reference has one mapping for every batch size,
 * embedding_lookup.cuh:186-208).  0 = the launcher decides (default), 1 = never, 2 = whenever the row shape allows it,
 * 3 / 4 / 5 / ... = likewise with 2 / 4 / 8 / ... samples sharing a workgroup (narrow rows; as far as the row allows). */
void cuembed_set_forward_wide_load(int mode);
/* cuembed_embedding_forward with per-call options (cuembed::ForwardOptions): reduction_order 0 / 1,
 * row_load_policy 0 / 1, or -1 = the process-wide default.  No state is read or written when both are >= 0. */
void cuembed_embedding_forward_with_options(const void* params, int elem_type, int embed_width,
                                            const void* indices, int index_type, const void* offsets,
                                            int offset_type, const void* weights, int batch_size,
                                            int num_hots, int mode, int fp16_math, void* ret,
                                            int reduction_order, int row_load_policy,
                                            cuembed_stream_t stream);
/* ... and with cuembed::ForwardOptions::sample_order (extension, CSR only; NULL = none): `sample_order` is a device
 * array holding a permutation of [0, batch_size) -- the order in which the samples are handed to the wavefronts.
 * A scheduling hint: every sample is still pooled in lookup order into its own output row, so results do not
 * depend on it.  With ragged bags in descending order of length (the two bags of a wavefront run in lockstep;
 * wavefronts with unequal bags end at different times) BASELINE config 3 takes 0.148 instead of 0.170 ms.
 * Aborts when given with fixed hotness (nothing to balance there). */
void cuembed_embedding_forward_ordered(const void* params, int elem_type, int embed_width,
                                       const void* indices, int index_type, const void* offsets,
                                       int offset_type, const void* weights, int batch_size,
                                       int num_hots, int mode, int fp16_math, void* ret,
                                       int reduction_order, int row_load_policy,
                                       const int32_t* sample_order, cuembed_stream_t stream);
/* ... and with cuembed::ForwardOptions::row_loads_device (extension; NULL = none): the row-load decision that
 * cuembed_decide_row_loads left in device memory is read by the kernels instead of row_load_policy. */
void cuembed_embedding_forward_device_hints(const void* params, int elem_type, int embed_width,
                                            const void* indices, int index_type, const void* offsets,
                                            int offset_type, const void* weights, int batch_size,
                                            int num_hots, int mode, int fp16_math, void* ret,
                                            int reduction_order, int row_load_policy,
                                            const int32_t* sample_order, const uint32_t* row_loads_device,
                                            cuembed_stream_t stream);
/* cuembed::DecideRowLoads (extension; the reference has one launch rule for every index distribution,
 * embedding_lookup.cuh:186-208): the row-load policy decided ON THE DEVICE from the batch's own indices, no read-back,
 * one launch, capturable.  decision[0] = 1 (non-temporal row loads) when at least distinct_per_65536 / 65536 of an
 * evenly strided sample of up to 65,536 lookups names distinct rows (counted exactly, in groups of 4,096), the table
 * has table_bytes >= 1 GiB and the batch nnz >= 2^18 lookups; else 0.  distinct_per_65536 = 0: the built-in 0.998
 * (8 repeats per group of 4,096: the measured crossover -- streaming costs 20 % as soon as 3 % of a group repeats).
 * `decision` = FOUR 32-bit device words zeroed once by the caller (words 1..3 are the kernel's own and stay zero);
 * calls sharing them must be stream-ordered.  Never changes a result. */
void cuembed_decide_row_loads(const void* indices, int index_type, int64_t nnz, int64_t table_bytes,
                              uint32_t* decision, unsigned distinct_per_65536, cuembed_stream_t stream);
/* cuembed::BagOrderByLength (extension): sample_order[batch_size] = the samples of a CSR batch by descending bag
 * length, ties in input order.  max_length > 0: a bound on the bag length (longer bags rank as max_length), 0 =
 * unknown, < 0 = bags of 255 lookups and more rank alike.  With a bound <= 255 and batch_size <= 131,072 it is two small
 * launches (a stable counting sort in chunks of 1,024 samples; 7 us for 65,536 bags -- cheap enough for every fresh offsets
 * array); otherwise a key kernel + the library's stable sort.  Two-phase workspace query: work == NULL writes the bytes needed to *lwork. */
void cuembed_bag_order_by_length(const void* offsets, int offset_type, int batch_size, int max_length,
                                 int32_t* sample_order, char* work, size_t* lwork, cuembed_stream_t stream);
/* cuembed::SetBackwardTuning / GetBackwardTuning (tuning and tests; 0 = built-in heuristic):
 * lookups per nz-segment (rounded down to a multiple of 8), XCD column slices of the gather
 * (1, 2, 4, 8).  Process-wide; initial values from CUEMBED_BWD_SEGMENT_LEN / CUEMBED_BWD_SLICES,
 * read once.  Results never depend on these. */
void cuembed_set_backward_tuning(int segment_len, int column_slices);
void cuembed_get_backward_tuning(int* out2);

/* ---- multi-GPU: the device-side halves of the sparse gradient exchange (extensions) ------
 * The reference is single-GPU (README.md:108-119: multi-device is future work).  A data-parallel step sums the ranks'
 * compressed gradients with an owner-partitioned exchange of FIXED-size buffers (cuembed_amd/distributed.py:
 * SparseGradExchange; the collectives are the caller's); these two calls are the index work around the collectives,
 * without any read-back (cuembed::PackRowsByOwner / FinishOwnerPiece, exchange_transforms.hpp).
 *
 * cuembed_exchange_pack_rows: ids[num_rows] (index_type) ascending in their first *count entries (count: one device
 * word of index_type; NULL = all), rows[num_rows, embed_width]; cuts[world + 1] device words (cuts[r] = first row id
 * of owner r, cuts[world] = num_categories).  Slot r of send_ids[world * slot_capacity] /
 * send_rows[world * slot_capacity, embed_width] gets the ids / rows of owner r's range, then the padding id
 * num_categories.  range_starts[world + 1]: device scratch.  *flag |= 1 (a 64-bit device word the caller zeroes) when
 * a range exceeds its slot or, with input_capacity > 0, *count exceeds input_capacity.  Two launches. */
void cuembed_exchange_pack_rows(const void* ids, int index_type, const void* rows, int elem_type, int64_t num_rows,
                                int embed_width, const void* count, const int64_t* cuts, int world,
                                int64_t slot_capacity, int64_t input_capacity, int64_t num_categories,
                                int64_t* send_ids, void* send_rows, int64_t* range_starts, int64_t* flag,
                                cuembed_stream_t stream);
/* cuembed_exchange_finish_piece: after the owner merged what it received -- cuembed_transpose_fixed_hotness_remapped
 * (the received int64 ids as nnz samples of hotness 1, index bits of num_categories + 1) and
 * cuembed_embedding_backward_bounded (capacity_rows = capacity + 1, pad_to_capacity) into ids[capacity + 1] /
 * rows[capacity + 1, embed_width] -- this finishes the piece on the device: *count (may be NULL) = distinct real ids;
 * the padding ids' run (or the spare last row) zeroed; ids behind the count = pad_lo + i % pad_len; and, when `tail`
 * (capacity + 2 words) is given, the id buffer of the all-gather: the ids, min(count, capacity), *flag.
 * *flag |= 1 when count > capacity (the merge then wrote nothing).  One launch. */
void cuembed_exchange_finish_piece(const int64_t* sorted_ids, const int64_t* remapped_ids, int64_t nnz, int64_t capacity,
                                   int64_t num_categories, int64_t pad_lo, int64_t pad_len, int64_t* ids, void* rows,
                                   int elem_type, int embed_width, int64_t* tail, int64_t* flag, int64_t* count,
                                   cuembed_stream_t stream);

/* ---- introspection ------------------------------------------------------- */
/* Launch shape the forward would use (no launch): out[0] = elements per lane,
 * out[1] = lanes per row, out[2] = samples per workgroup, out[3] = grid size,
 * out[4] = dynamic LDS bytes, out[5] = 1 if indices are staged in LDS, 2 if the batch is small enough for the
 * wide-load kernel (out[2] = 1, or a few samples of narrow rows, per workgroup; the bags' rows parked in LDS). */
void cuembed_forward_launch_shape(int elem_type, int index_type, int embed_width, int batch_size,
                                  int num_hots, int is_csr, int is_weighted, int mode,
                                  int* out);
/* What the launch heuristics know about the current device (read once per device id, cuembed::detail::DeviceShape;
 * the reference queries the runtime per call, embedding_lookup.cuh:355-363): out[0] = compute units, out[1] = XCDs,
 * out[2] = resident lanes per compute unit, out[3] = L2 bytes per XCD. */
void cuembed_device_shape(int* out);
/* Launch shape EmbeddingBackward would use (no launch): out[0] = XCD column slices, out[1] = lanes per slice,
 * out[2] = nz-segments per workgroup, out[3] = lookups per segment, out[4] = workgroup ranges, out[5] = grid size,
 * out[6] = dynamic LDS bytes, out[7] = XCDs assumed.  compute_units <= 0: the current device; > 0: a device of that
 * many compute units in `xcds` XCDs (host arithmetic only: e.g. 32 CUs in 1 XCD = a CPX partition). */
void cuembed_backward_launch_shape(int elem_type, int index_type, int embed_width, int64_t nnz, int is_weighted,
                                   int compute_units, int xcds, int* out);
/* cuembed_recommended_sample_blocks for a described device (compute_units <= 0: the current one). */
int cuembed_recommended_sample_blocks_on(int elem_type, int embed_width, int batch_size, int64_t nnz,
                                         int compute_units, int xcds, int64_t l2_bytes_per_xcd);
/* ---- sparse optimizer step (extension: the reference ends at the gradient) ---------------
 * cuembed_sparse_row_update (cuembed::SparseRowUpdate, sparse_update.hpp): for every valid entry k,
 * table[ids[k], :] (elem_type, [num_categories, embed_width]) and the state of row ids[k] are updated in place from
 * rows[k, :] (elem_type).  fp32 arithmetic, one rounding to the table's type at the store.
 *   CUEMBED_UPDATE_SGD              w <- w - lr * g                                            state = NULL
 *   CUEMBED_UPDATE_ADAGRAD          s <- s + g^2;  w <- w - lr * g / (sqrt(s) + eps)           state fp32 [num_categories, embed_width]
 *   CUEMBED_UPDATE_ROWWISE_ADAGRAD  s_r <- s_r + mean_j(g_j^2);  w_j <- w_j - lr * g_j / (sqrt(s_r) + eps)   state fp32 [num_categories]
 * The entries are `pieces` blocks of piece_rows entries (ids[pieces * piece_rows], rows[pieces * piece_rows,
 * embed_width]); entry j of piece p is valid iff j < count(p), from exactly one of: num_rows >= 0 (host-known, one
 * piece; else pass -1); counts[pieces] on the device (int32, or int64 with counts_are_int64 != 0); last_id, one
 * index_type word on the device with count = *last_id + 1 (one piece; transpose_remapped_indices + nnz - 1 of
 * cuembed_embedding_backward with num_grad_embedding_rows < 0).  Entries at or past the count are ignored whatever
 * they hold; a count above piece_rows or below zero changes nothing.  The valid entries must name DISTINCT rows (a
 * coalesced gradient; the uncoalesced gradient of a sample-blocked transpose is not accepted).  lr_device != NULL:
 * the learning rate is read from that fp32 device word instead of lr.  One launch, no read-back. */
enum { CUEMBED_UPDATE_SGD = 0, CUEMBED_UPDATE_ADAGRAD = 1, CUEMBED_UPDATE_ROWWISE_ADAGRAD = 2 };
void cuembed_sparse_row_update(void* table, int elem_type, int embed_width, float* state, int rule, const void* ids,
                               int index_type, const void* rows, int64_t piece_rows, int pieces, int64_t num_rows,
                               const void* counts, int counts_are_int64, const void* last_id, float lr,
                               const float* lr_device, float eps, cuembed_stream_t stream);
/* The same step with the state in a place of its own: entry k updates table[ids[k], :] but reads and writes its state
 * at row state_ids[k] of `state` (the accumulator row for CUEMBED_UPDATE_ADAGRAD, the row word for
 * CUEMBED_UPDATE_ROWWISE_ADAGRAD).  For a table behind the row cache with a state plane: ids and state_ids are the
 * batch's ids translated with the two planes' row offsets.  Same walk, same bits.  state_ids == NULL: the call above;
 * otherwise the rule must have a state. */
void cuembed_sparse_row_update_placed(void* table, int elem_type, int embed_width, float* state, int rule,
                                      const void* ids, int index_type, const void* rows, int64_t piece_rows, int pieces,
                                      int64_t num_rows, const void* counts, int counts_are_int64, const void* last_id,
                                      float lr, const float* lr_device, float eps, cuembed_stream_t stream,
                                      const int64_t* state_ids);
/* Launch shape of cuembed_sparse_row_update for aligned buffers (no launch): out[0] = bytes per lane, out[1] = lanes
 * per row, out[2] = lanes per entry (a power of two <= 64), out[3] = row slices a lane holds at once (0 = run-time
 * loop), out[4] = grid size.  compute_units <= 0: the current device. */
void cuembed_sparse_row_update_launch_shape(int elem_type, int embed_width, int64_t total_entries, int compute_units,
                                            int* out);
/* cuembed_sparse_row_update with STOCHASTIC ROUNDING of the one rounding to the table's type (elem_type CUEMBED_F16 or
 * CUEMBED_BF16; the fp32 arithmetic and the fp32 state are those of cuembed_sparse_row_update).  An update smaller than
 * half a unit in the last place of a 16-bit table is otherwise rounded away at every step.  The fp32 value x is rounded
 * away from zero with the probability of its position between its two neighbours, decided by a 16-bit random field r:
 *   fp16: q = the spacing of fp16 at |x| (2^(e-10) for |x| >= 2^-14, else 2^-24), m = |x| / q, i = floor(m),
 *         t = floor((m - i) * 2^13); away from zero iff t + (r & 0x1FFF) >= 2^13; the result is +-(i + up) * q;
 *   bf16: r is added to the low 16 bits of x's pattern, which are then dropped.
 * A representable x is unchanged for every r, a result past the largest finite value is +-inf, inf and NaN convert as
 * usual, the sign of zero is kept.  The fields come from Philox4x32-10: one call serves columns [8 * G, 8 * G + 8) of
 * table row R, with counter (R low 32, R high 32, G, step low 32) and key (seed low 32, seed high 32 ^ step high 32);
 * column c takes half (c % 8) % 2 (low half first) of output word (c % 8) / 2.  The bits therefore depend on (seed, step,
 * table row, column) only -- not on alignment, the launch shape, the entry's position or the count source: give every
 * call of a run the same seed and its own step.  step_device != NULL: the step is read from that int64 device word
 * instead of `step` (advance it on the device and a replayed graph draws fresh bits).  One launch, no read-back. */
void cuembed_sparse_row_update_stochastic(void* table, int elem_type, int embed_width, float* state, int rule,
                                          const void* ids, int index_type, const void* rows, int64_t piece_rows,
                                          int pieces, int64_t num_rows, const void* counts, int counts_are_int64,
                                          const void* last_id, float lr, const float* lr_device, float eps,
                                          uint64_t seed, uint64_t step, const int64_t* step_device,
                                          cuembed_stream_t stream);
/* cuembed_sparse_row_update_stochastic BEHIND THE ROW CACHE: entry k updates table[ids[k], :] and, for a rule with a
 * state, the state at row state_ids[k] of `state` (as cuembed_sparse_row_update_placed), and the one rounding to the
 * table's type draws the bits of (seed, step, row_names[k], column): `ids` / `state_ids` are the batch's ids translated
 * with the planes' row offsets and name cache slots, `row_names` ([pieces * piece_rows] int64) are the batch's own ids,
 * the table rows, so that a row rounds with the same bits wherever the cache has put it.  Lane bytes, launch shape and
 * walk are those of cuembed_sparse_row_update_stochastic, and so are the bits on tensors that hold the same values.
 * row_names must not be NULL (without names the call is cuembed_sparse_row_update_stochastic).  CUEMBED_UPDATE_SGD takes
 * state == NULL and state_ids == NULL (the table plane only); the other rules require both.  elem_type CUEMBED_F16 or
 * CUEMBED_BF16.  The valid entries must name distinct rows in every id array.  Misuse aborts with the failed condition.
 * One launch, no read-back. */
void cuembed_sparse_row_update_placed_stochastic(void* table, int elem_type, int embed_width, float* state, int rule,
                                                 const void* ids, int index_type, const void* rows, int64_t piece_rows,
                                                 int pieces, int64_t num_rows, const void* counts, int counts_are_int64,
                                                 const void* last_id, float lr, const float* lr_device, float eps,
                                                 uint64_t seed, uint64_t step, const int64_t* step_device,
                                                 cuembed_stream_t stream, const int64_t* state_ids,
                                                 const int64_t* row_names);
/* The specification above as host code (no launch, no device): out[0..3] = the four Philox output words of the call
 * for (seed, step, row, column_group) ... */
void cuembed_stochastic_rounding_words(uint64_t seed, uint64_t step, int64_t row, uint32_t column_group, uint32_t* out);
/* ... and the 16-bit pattern that x is rounded to with the field r16 (elem_type CUEMBED_F16 or CUEMBED_BF16). */
uint16_t cuembed_stochastic_round(int elem_type, float x, uint32_t r16);
/* The same for n values on the host: out[i] = cuembed_stochastic_round(elem_type, x[i], r16[i]). */
void cuembed_stochastic_round_array(int elem_type, const float* x, const uint32_t* r16, int64_t n, uint16_t* out);
/* ---- sparse optimizer step, the Adam family (extension) --------------------------------------
 * cuembed_sparse_row_adam (cuembed::SparseRowAdam, sparse_adam.hpp): for every valid entry k, table[ids[k], :]
 * (elem_type, [num_categories, embed_width]) and the moments of row ids[k] are updated in place from rows[k, :]
 * (elem_type).  Rows that no valid entry names are neither read nor written: their moments do not decay (the "lazy"
 * behaviour of torch.optim.SparseAdam).  With g the gradient element, w the weight, m = exp_avg, v = exp_avg_sq:
 *   both rules                w <- w - (lr * weight_decay) * w           only if weight_decay != 0 (decoupled, AdamW)
 *                             m <- beta1 * m + one_minus_beta1 * g       exp_avg fp32 [num_categories, embed_width]
 *   CUEMBED_ADAM              v <- beta2 * v + one_minus_beta2 * (g * g) exp_avg_sq fp32 [num_categories, embed_width]
 *                             w <- w - ((lr * c) * m) / (sqrt(v) + eps)
 *   CUEMBED_ROWWISE_ADAM      v_r <- beta2 * v_r + one_minus_beta2 * (sum_j(g_j^2) / embed_width)
 *                                                                        exp_avg_sq fp32 [num_categories]
 *                             w_j <- w_j - ((lr * c) / (sqrt(v_r) + eps)) * m_j
 * Every operation written above is one fp32 operation, rounded once and never fused; the result is rounded once to the
 * table's type at the store.  sum_j adds the squares of a lane's elements in column order and then the lanes' sums in a
 * butterfly.  c = bias_factor is sqrt(1 - beta2^t) / (1 - beta1^t) of step t >= 1 (torch.optim.SparseAdam's formula: the
 * correction goes into the step size, eps is added to sqrt(v)), or 1 for no bias correction.  The kernel multiplies with
 * the fp32 values it is given: pass one_minus_beta = (float)(1.0 - (double)beta), formed in double and rounded once.
 * lr_device / bias_factor_device != NULL: the value is read from that fp32 device word instead (cuembed_adam_clock_advance
 * writes the latter).  Betas must lie in [0, 1), eps and weight_decay must not be negative.  The entries, the three count
 * sources (num_rows / counts / last_id), the pieces and the DISTINCT-rows contract are those of
 * cuembed_sparse_row_update.  One launch, no read-back. */
enum { CUEMBED_ADAM = 0, CUEMBED_ROWWISE_ADAM = 1 };
void cuembed_sparse_row_adam(void* table, int elem_type, int embed_width, float* exp_avg, float* exp_avg_sq, int rule,
                             const void* ids, int index_type, const void* rows, int64_t piece_rows, int pieces,
                             int64_t num_rows, const void* counts, int counts_are_int64, const void* last_id, float lr,
                             const float* lr_device, float bias_factor, const float* bias_factor_device, float beta1,
                             float one_minus_beta1, float beta2, float one_minus_beta2, float eps, float weight_decay,
                             cuembed_stream_t stream);
/* The same step with the moments in places of their own: entry k updates table[ids[k], :] but reads and writes its
 * first moment at row exp_avg_ids[k] of exp_avg and its second at row exp_avg_sq_ids[k] of exp_avg_sq (CUEMBED_ADAM: a
 * row of embed_width elements; CUEMBED_ROWWISE_ADAM: the row's word).  For a table behind the row cache with two state
 * planes: the three id arrays are the batch's ids translated with the three planes' row offsets.  Round to nearest;
 * same lane bytes, launch shape and walk as the call above, hence the same bits.  Both id arrays NULL: the call above;
 * exactly one of them NULL aborts. */
void cuembed_sparse_row_adam_placed(void* table, int elem_type, int embed_width, float* exp_avg, float* exp_avg_sq,
                                    int rule, const void* ids, int index_type, const void* rows, int64_t piece_rows,
                                    int pieces, int64_t num_rows, const void* counts, int counts_are_int64,
                                    const void* last_id, float lr, const float* lr_device, float bias_factor,
                                    const float* bias_factor_device, float beta1, float one_minus_beta1, float beta2,
                                    float one_minus_beta2, float eps, float weight_decay, cuembed_stream_t stream,
                                    const int64_t* exp_avg_ids, const int64_t* exp_avg_sq_ids);
/* cuembed_sparse_row_adam with STOCHASTIC ROUNDING of the one rounding to the table's type (elem_type CUEMBED_F16 or
 * CUEMBED_BF16): the rule and the random bits of (seed, step, table row, column) are those of
 * cuembed_sparse_row_update_stochastic; the fp32 arithmetic and the fp32 moments are those of cuembed_sparse_row_adam. */
void cuembed_sparse_row_adam_stochastic(void* table, int elem_type, int embed_width, float* exp_avg, float* exp_avg_sq,
                                        int rule, const void* ids, int index_type, const void* rows, int64_t piece_rows,
                                        int pieces, int64_t num_rows, const void* counts, int counts_are_int64,
                                        const void* last_id, float lr, const float* lr_device, float bias_factor,
                                        const float* bias_factor_device, float beta1, float one_minus_beta1, float beta2,
                                        float one_minus_beta2, float eps, float weight_decay, uint64_t seed,
                                        uint64_t step, const int64_t* step_device, cuembed_stream_t stream);
/* cuembed_sparse_row_adam_stochastic BEHIND THE ROW CACHE: the moments of entry k at rows exp_avg_ids[k] /
 * exp_avg_sq_ids[k] (as cuembed_sparse_row_adam_placed), and the rounding bits those of (seed, step, row_names[k], column)
 * -- row_names ([pieces * piece_rows] int64) are the batch's own ids, the table rows, next to the three translated id
 * arrays.  Lane bytes, launch shape and walk are those of cuembed_sparse_row_adam_stochastic, and so are the bits on
 * tensors that hold the same values.  exp_avg_ids, exp_avg_sq_ids and row_names must not be NULL; elem_type CUEMBED_F16
 * or CUEMBED_BF16.  Misuse aborts with the failed condition.  One launch, no read-back. */
void cuembed_sparse_row_adam_placed_stochastic(void* table, int elem_type, int embed_width, float* exp_avg,
                                               float* exp_avg_sq, int rule, const void* ids, int index_type,
                                               const void* rows, int64_t piece_rows, int pieces, int64_t num_rows,
                                               const void* counts, int counts_are_int64, const void* last_id, float lr,
                                               const float* lr_device, float bias_factor,
                                               const float* bias_factor_device, float beta1, float one_minus_beta1,
                                               float beta2, float one_minus_beta2, float eps, float weight_decay,
                                               uint64_t seed, uint64_t step, const int64_t* step_device,
                                               cuembed_stream_t stream, const int64_t* exp_avg_ids,
                                               const int64_t* exp_avg_sq_ids, const int64_t* row_names);
/* The bias-factor clock, advanced on the device (one single-thread launch, no read-back): powers, fp64[3] on the device
 * holding (t, beta1^t, beta2^t) and starting at (0, 1, 1), becomes (t + 1, beta1^t * beta1, beta2^t * beta2) in fp64, and
 * *bias_factor (fp32, on the device) = sqrt(1 - beta2^t) / (1 - beta1^t) of the new t, computed in fp64 and rounded once.
 * Enqueued in front of cuembed_sparse_row_adam(bias_factor_device = bias_factor), a captured graph counts its replays. */
void cuembed_adam_clock_advance(double* powers, float* bias_factor, double beta1, double beta2, cuembed_stream_t stream);
/* ---- 8-bit row-wise quantized tables (extension; inference only) ---------------------------
 * The format is PyTorch's fused 8-bit row-wise layout (quantized::embedding_bag_byte_prepack): a row of embed_width
 * values is embed_width + 8 bytes -- embed_width uint8 codes, the row's fp32 scale, its fp32 bias, little endian --
 * and a value is code * scale + bias.  embed_width must be a multiple of 4; tables are contiguous
 * [num_categories, embed_width + 8] bytes, at least 4-byte aligned (8-byte aligned tables of embed_width % 8 == 0 take
 * the 8-byte lanes); outputs are 16-byte aligned. */
int64_t cuembed_quantized_row_bytes(int embed_width);
/* cuembed::QuantizeRows: in [rows, embed_width] of elem_type (fp32 / fp16 / bf16, 16-byte aligned) -> out, fused rows.
 * scale = (max - min) / 255, bias = min, code = rint((x - min) * (255 / (max - min + 1e-8))), every step one fp32
 * operation: the bytes torch's CPU prepack writes. */
void cuembed_quantize_rows(const void* in, int elem_type, int embed_width, int64_t rows, void* out,
                           cuembed_stream_t stream);
/* cuembed::DequantizeRows: out[i, :] (out_type: CUEMBED_F32 or CUEMBED_F16) = the values of row ids[i] (ids == NULL:
 * row i): float(code) * scale + bias in two rounded fp32 operations, then one rounding to out_type. */
void cuembed_dequantize_rows(const void* qtable, int embed_width, const void* ids, int index_type, int64_t n, void* out,
                             int out_type, cuembed_stream_t stream);
/* cuembed::EmbeddingForwardQuantized: cuembed_embedding_forward on a fused table.  ret and weights are of out_type
 * (CUEMBED_F32 or CUEMBED_F16); fp32 accumulation in lookup order; row_load_policy (-1 = the process-wide default, 0
 * default, 1 streaming), sample_order (CSR only) and row_loads_device are the scheduling hints of
 * cuembed_embedding_forward_device_hints and change no bit. */
void cuembed_embedding_forward_quantized(const void* qtable, int embed_width, const void* indices, int index_type,
                                         const void* offsets, int offset_type, const void* weights, int batch_size,
                                         int num_hots, int mode, void* ret, int out_type, int row_load_policy,
                                         const int32_t* sample_order, const uint32_t* row_loads_device,
                                         cuembed_stream_t stream);
/* Launch shape of the quantized sum / mean forward for aligned buffers (no launch): out[0] = codes per lane, out[1] =
 * lanes per row, out[2] = samples per workgroup, out[3] = grid size, out[4] = dynamic LDS bytes, out[5] = 1 when the
 * indices are staged in LDS.  compute_units > 0 describes the device (with xcds); <= 0: the current device. */
void cuembed_quantized_forward_launch_shape(int index_type, int out_type, int embed_width, int batch_size, int num_hots,
                                            int is_csr, int is_weighted, int compute_units, int xcds, int* out);
/* ---- a GROUP of tables pooled in one launch (extension; forward only, sum / mean only) -----
 * num_tables >= 1 tables on one device, of one element type (or all fused 8-bit) and one embed_width; their row counts
 * may differ.  Bag g = t * batch_per_table + b belongs to table t and sample b (table-major).  CSR: one indices[nnz],
 * one offsets[num_tables * batch_per_table + 1], optional weights[nnz]; fixed hotness (offsets == NULL): indices
 * [num_tables, batch_per_table, num_hots].  ret is [batch_per_table, num_tables, embed_width], contiguous: bag (t, b)
 * at ret + (b * num_tables + t) * embed_width -- the per-table results stacked on dimension 1, with the bits of
 * num_tables single-table calls.  num_tables * batch_per_table <= INT_MAX.
 * The caller builds the table base pointers twice, once: tables_host (host memory; read by the library for the access
 * width -- the least aligned table decides for the group) and tables_device (device memory; read by the kernel).  The
 * library never reads device memory on the host, copies nothing per call and allocates nothing.
 * row_load_policy (-1 = the process-wide default, 0 default, 1 streaming; one value for the group) and sample_order (CSR
 * only: a permutation of the num_tables * batch_per_table bags, e.g. cuembed_bag_order_by_length on the combined
 * offsets) are scheduling hints and change no bit.  Misuse aborts like everywhere else. */
/* cuembed::EmbeddingForwardGrouped: tables, weights and ret of elem_type; fp32 accumulation in lookup order. */
void cuembed_embedding_forward_grouped(const void* const* tables_host, const void* const* tables_device, int num_tables,
                                       int elem_type, int embed_width, const void* indices, int index_type,
                                       const void* offsets, int offset_type, const void* weights, int batch_per_table,
                                       int num_hots, int mode, void* ret, int row_load_policy,
                                       const int32_t* sample_order, cuembed_stream_t stream);
/* cuembed::EmbeddingForwardQuantizedGrouped: fused 8-bit tables (at least 4-byte aligned); weights and ret of out_type
 * (CUEMBED_F32 or CUEMBED_F16), ret 16-byte aligned. */
void cuembed_embedding_forward_quantized_grouped(const void* const* tables_host, const void* const* tables_device,
                                                 int num_tables, int embed_width, const void* indices, int index_type,
                                                 const void* offsets, int offset_type, const void* weights,
                                                 int batch_per_table, int num_hots, int mode, void* ret, int out_type,
                                                 int row_load_policy, const int32_t* sample_order,
                                                 cuembed_stream_t stream);
/* Launch shape of a grouped forward for aligned buffers (no launch; host arithmetic only when compute_units > 0 or
 * quantized == 0): quantized != 0: fused tables, elem_type = the output's type.  out[0] = elements (codes) per lane,
 * out[1] = lanes per row, out[2] = bags per workgroup, out[3] = grid size = ceil(num_tables * batch_per_table / out[2]),
 * out[4] = dynamic LDS bytes, out[5] = 1 when the indices are staged in LDS, out[6] = where the lanes find their
 * indices: 0 = staged in LDS, 1 = cross-lane reads, 2 = global loads. */
void cuembed_grouped_forward_launch_shape(int quantized, int elem_type, int index_type, int embed_width, int num_tables,
                                          int batch_per_table, int num_hots, int is_csr, int is_weighted,
                                          int compute_units, int xcds, int* out);
/* ---- a group of tables of DIFFERENT widths pooled in one launch (extension; sum / mean only, its backward:
 * cuembed_embedding_backward_mixed_group below; plain
 * tables of one element type; cuembed::EmbeddingForwardMixedGroup, mixed_group_lookup.hpp) -----
 * The input is the group's above: bag g = t * batch_per_table + b; CSR indices[nnz] / offsets[num_tables *
 * batch_per_table + 1] / optional weights[nnz], or fixed hotness (offsets == NULL) indices[num_tables, batch_per_table,
 * num_hots].  Table t is [rows_t, widths_host[t]], every row a multiple of 4 bytes.  ret is [batch_per_table, D],
 * contiguous, D = the sum of the widths: bag (t, b) at ret + b * D + c_t, c_t the exclusive prefix sum of the widths --
 * the per-table results concatenated on dimension 1, with the bits of num_tables single-table calls.
 * The caller builds once: tables_host / tables_device as above, widths_host (host memory), and per (group,
 * batch_per_table, lane bytes) the descriptor: cuembed_mixed_group_descriptor_bytes(num_tables) bytes, filled on the
 * host by cuembed_fill_mixed_group_descriptor and copied to the device by the caller (4-byte aligned).  lane_bytes is
 * the widest of 16 / 8 / 4 that every table base, ret, D * sizeof, every c_t * sizeof and every width * sizeof are a
 * multiple of (cuembed_mixed_group_launch_shape computes it: out[0] * sizeof); block_threads is out[1] of the same
 * call.  A descriptor filled for another lane width, batch_per_table or block size is a contract violation the library
 * cannot see.  The library never reads device memory on the host, copies nothing per call and allocates nothing; the
 * call is one kernel launch.  row_load_policy as above; there is no sample_order.  num_tables * batch_per_table,
 * D and the grid must fit an int; there is no other limit on num_tables.  Misuse aborts like everywhere else. */
void cuembed_embedding_forward_mixed_group(const void* const* tables_host, const void* const* tables_device,
                                           const int* widths_host, const void* descriptor_device, int num_tables,
                                           int elem_type, const void* indices, int index_type, const void* offsets,
                                           int offset_type, const void* weights, int batch_per_table, int num_hots,
                                           int mode, void* ret, int row_load_policy, cuembed_stream_t stream);
size_t cuembed_mixed_group_descriptor_bytes(int num_tables);
/* Host arithmetic only.  Entry t < num_tables of host_blob: int32 {width, c_t, L_t, first workgroup}, L_t = min(width *
 * elem_bytes / lane_bytes, block_threads) lanes per bag, block_threads / L_t bags per workgroup; entry num_tables: {0,
 * D, 0, grid}.  Returns the grid = sum_t ceil(batch_per_table / (block_threads / L_t)). */
int cuembed_fill_mixed_group_descriptor(const int* widths_host, int num_tables, int elem_bytes, int lane_bytes,
                                        int batch_per_table, int block_threads, void* host_blob);
/* Launch shape of a mixed-width forward (no launch; host arithmetic only).  pointer_bits: the table bases and ret OR-ed
 * (0 = aligned buffers).  out[0] = elements per lane, out[1] = block threads, out[2] = grid, out[3] = D, out[4] =
 * dynamic LDS bytes, out[5] = 1 when the indices are staged in LDS, out[6] = the most bags a workgroup holds. */
void cuembed_mixed_group_launch_shape(const int* widths_host, int num_tables, int elem_type, int index_type,
                                      int batch_per_table, int num_hots, int is_weighted, size_t pointer_bits, int* out);
/* ---- the backward of a group (extension): one sort and one scatter-add for all its tables -----
 * The group above is trained through the single-table pipeline, fed the right keys.  row_base[num_tables + 1] is the
 * exclusive prefix sum of the tables' row counts: int64, DEVICE memory, built once by the caller; row_base[num_tables]
 * = total_rows.  Call sequence (all on one stream, nothing allocated, nothing read back):
 *   cuembed_grouped_backward_keys        keys + sample ids of all lookups
 *   cuembed_transpose[_remapped]         rows = sample_ids, cols = keys, index_bits = ceil(log2(total_rows))
 *   cuembed_compute_compressed_grad_indices   (compressed gradient only, unless the transpose gave the remap)
 *   cuembed_embedding_backward[_bounded] grad_y = the gradient of ret viewed as [batch_per_table * num_tables, width]
 *   cuembed_grouped_table_cuts           where each table's entries begin in the compressed gradient
 * The gradient is that of the tables laid end to end, sorted by table, then by row; for tables that are row slices of
 * ONE allocation it is directly a gradient of that allocation (cuembed_sparse_row_update applies unchanged). */
/* cuembed::GroupedBackwardKeys: for lookup p of bag t * batch_per_table + b, keys[p] = row_base[t] + indices[p] and
 * sample_ids[p] = b * num_tables + t, both of key_type (CUEMBED_I32 needs total_rows < 2^31; independent of index_type).
 * CSR: offsets[num_tables * batch_per_table + 1] of offset_type, num_hots = 0; fixed hotness: offsets = NULL, num_hots
 * > 0.  nnz = the number of lookups, <= INT_MAX.  Ids outside their table are a contract violation
 * (cuembed_check_indices finds and repairs them on the device). */
void cuembed_grouped_backward_keys(const void* indices, int index_type, const void* offsets, int offset_type,
                                   const int64_t* row_base, int num_tables, int batch_per_table, int num_hots,
                                   int64_t nnz, void* keys, void* sample_ids, int key_type, cuembed_stream_t stream);
/* cuembed::GroupedTableCuts: cuts[t] (int64, device, num_tables + 1 entries) = the number of valid entries of the
 * ascending global ids inverse_mapping (index_type) that are < row_base[t]; cuts[num_tables] = the count.  The count:
 * count_word (device; one int32 word, or int64 with count_word_is_64), else last_id (device; one word of index_type,
 * count = last_id + 1: transpose_remapped_indices + nnz - 1), else the host value count.  capacity = the entries
 * inverse_mapping has room for; a count outside [0, capacity] gives all-zero cuts. */
void cuembed_grouped_table_cuts(const void* inverse_mapping, int index_type, int64_t capacity, int64_t count,
                                const void* count_word, int count_word_is_64, const void* last_id,
                                const int64_t* row_base, int num_tables, int64_t* cuts, cuembed_stream_t stream);
/* cuembed::EmbeddingWeightGradGrouped: the gradient of a weighted SUM-forward of a group with respect to the per-lookup
 * weights, in one launch: for lookup p of bag t * batch_per_table + b, grad_weights[p] = dot(tables[t][indices[p], :],
 * grad_y[b, t, :]) in fp32, rounded once -- the bits of num_tables calls of cuembed_embedding_weight_grad.  tables_host /
 * tables_device, indices and offsets as in cuembed_embedding_forward_grouped; grad_y [batch_per_table, num_tables,
 * embed_width] contiguous and grad_weights (the layout of indices) of elem_type. */
void cuembed_embedding_weight_grad_grouped(const void* const* tables_host, const void* const* tables_device,
                                           int num_tables, int elem_type, int embed_width, const void* indices,
                                           int index_type, const void* offsets, int offset_type, const void* grad_y,
                                           int batch_per_table, int num_hots, void* grad_weights,
                                           cuembed_stream_t stream);
/* cuembed::GroupedMeanScale: grad_y of a MEAN-pooled group -> grad_y of the equivalent sum-pooled one, in one launch:
 * out[b, t, :] = grad_y[b, t, :] * f (one fp32 multiply, one rounding), f = 1 / the length of bag t * batch_per_table +
 * b, or with weights (elem_type, the layout of the indices) 1 / the fp32 sum of the bag's weights; 0 when that is 0.
 * CSR: offsets[num_tables * batch_per_table + 1] of offset_type, num_hots = 0; fixed hotness: offsets = NULL, num_hots
 * > 0.  grad_y and out: [batch_per_table, num_tables, embed_width] of elem_type, contiguous; out may be grad_y.  The
 * sequence above, run on out, is then the backward of the mean. */
void cuembed_grouped_mean_scale(const void* grad_y, int elem_type, int embed_width, const void* offsets,
                                int offset_type, const void* weights, int num_tables, int batch_per_table, int num_hots,
                                void* out, cuembed_stream_t stream);
/* ---- the backward of a group of tables of DIFFERENT widths (extension): one sort and one scatter-add for all widths -----
 * The mixed-width group above (cuembed_embedding_forward_mixed_group: grad_y is the gradient of ret, [batch_per_table, D])
 * is trained through the sequence above with ONE call replaced:
 *   cuembed_grouped_backward_keys, cuembed_transpose_remapped           unchanged (sample ids b * num_tables + t)
 *   cuembed_embedding_backward_mixed_group                              for cuembed_embedding_backward
 *   cuembed_grouped_table_cuts                                          unchanged
 * The result is a compressed gradient PADDED to the widest table: inverse_mapping[k] = ascending global row ids,
 * grad_embedding [capacity, W_max], the gradient of entry k in grad_embedding[k * W_max, k * W_max + W_t) for the table t
 * its id falls in.  Columns >= W_t of an entry are UNSPECIFIED (untouched or zero); nothing in the library reads them.
 * The count is device-side only: transpose_remapped_indices[nnz - 1] + 1.  capacity_rows > 0: the rows the two outputs
 * hold; if the count exceeds it nothing is written and *capacity_overflow (device word, may be NULL) is OR-ed with 1;
 * 0 = unchecked.  widths_host: host memory.  table_columns_device: int32 [num_tables][2] = (c_t, W_t) in elements,
 * DEVICE memory, 8-byte aligned, built once by the caller -- it MUST agree with widths_host (c_t the exclusive prefix sum):
 * the kernel addresses grad_y and picks its lanes from it, and the library, which never reads device memory on the host,
 * cannot check that.  Arithmetic: cuembed_embedding_backward's default.  One lane
 * width for the launch: the widest of 16 / 8 / 4 bytes that grad_y, grad_embedding, D * sizeof, every c_t * sizeof and
 * every W_t * sizeof are a multiple of.  Limits: num_tables * batch_per_table and nnz <= INT_MAX, W_max at most 1024
 * lanes, batch_per_table * D * sizeof / lane bytes < 2^31; no other limit on num_tables.  Allocates nothing, reads
 * nothing back, capturable.  Not available for a mixed group: the dense gradient, reference sums, the sample-blocked
 * order, pad_to_capacity, the weight gradient and a one-launch optimizer step. */
void cuembed_embedding_backward_mixed_group(const void* grad_y, int elem_type, const int* widths_host,
                                            const void* table_columns_device, int num_tables, int batch_per_table,
                                            int64_t nnz, const void* transpose_indices, const void* transpose_sample_ids,
                                            const void* transpose_remapped_indices, int index_type,
                                            const void* transpose_weights, void* grad_embedding, void* inverse_mapping,
                                            int64_t capacity_rows, uint32_t* capacity_overflow, cuembed_stream_t stream);
/* cuembed::MixedGroupMeanScale: cuembed_grouped_mean_scale on the [batch_per_table, D] layout, in one launch:
 * out[b, c_t + j] = grad_y[b, c_t + j] * f, f the mean factor of bag t * batch_per_table + b.  The bits of num_tables
 * cuembed_grouped_mean_scale calls on one-table groups (aligned buffers).  out may be grad_y. */
void cuembed_mixed_group_mean_scale(const void* grad_y, int elem_type, const int* widths_host,
                                    const void* table_columns_device, const void* offsets, int offset_type,
                                    const void* weights, int num_tables, int batch_per_table, int num_hots, void* out,
                                    cuembed_stream_t stream);
/* Launch shape of cuembed_embedding_backward_mixed_group (no launch; host arithmetic only when compute_units > 0): the
 * plan of cuembed_backward_launch_shape at W_max.  pointer_bits: grad_y and grad_embedding OR-ed (0 = aligned buffers).
 * out[0] = elements per lane, out[1] = lanes of a workgroup's column slice, out[2] = segments per workgroup, out[3] =
 * segment length, out[4] = column slices, out[5] = grid, out[6] = dynamic LDS bytes, out[7] = lookups per workgroup,
 * out[8] = W_max, out[9] = D. */
void cuembed_mixed_group_backward_launch_shape(const int* widths_host, int num_tables, int elem_type, int64_t nnz,
                                               int is_weighted, size_t pointer_bits, int compute_units, int xcds,
                                               int* out);
/* ---- extension: the sparse optimizer step on a group of SEPARATE table tensors, in one launch ---------------------------
 * cuembed::SparseRowUpdateGrouped: cuembed_sparse_row_update on num_tables tables of elem_type and embed_width that are
 * separate allocations.  ids (index_type) are GLOBAL rows of the tables laid end to end -- the compressed gradient of
 * the sequence above --, rows their gradient rows; the kernel finds the table t of an entry itself (row_base[t] <= id <
 * row_base[t + 1]; row_base: int64, DEVICE memory, num_tables + 1 entries) and updates row id - row_base[t] of tables[t]
 * and of that table's state tensor.  tables_host / tables_device as in cuembed_embedding_forward_grouped (the host copy
 * is read for the access width: the least aligned table decides for the group); state_host / state_device likewise hold
 * the bases of the fp32 state tensors: both NULL for CUEMBED_UPDATE_SGD, [rows_t, embed_width] each for
 * CUEMBED_UPDATE_ADAGRAD (host copy required), [rows_t] each for CUEMBED_UPDATE_ROWWISE_ADAGRAD (host copy not read).
 * total_entries = the room of ids / rows.  The count, exactly one source: num_rows >= 0 on the host, else count_word
 * (device; one int32 word, or int64 with count_word_is_64), else last_id (device; one word of index_type, count =
 * last_id + 1); a count outside [0, total_entries] applies nothing.  Round to nearest.  num_tables <= 1023.  Nothing
 * is allocated or read back. */
void cuembed_sparse_row_update_grouped(const void* const* tables_host, const void* const* tables_device,
                                       const void* const* state_host, const void* const* state_device, int num_tables,
                                       int elem_type, int embed_width, const int64_t* row_base, int rule, const void* ids,
                                       int index_type, const void* rows, int64_t total_entries, int64_t num_rows,
                                       const void* count_word, int count_word_is_64, const void* last_id, float lr,
                                       const float* lr_device, float eps, cuembed_stream_t stream);
/* cuembed::SparseRowAdamGrouped: cuembed_sparse_row_adam on such a group.  exp_avg_* hold the bases of the fp32 [rows_t,
 * embed_width] first moments, exp_avg_sq_* those of the second moments: [rows_t, embed_width] (CUEMBED_ADAM; host copy
 * required) or [rows_t] (CUEMBED_ROWWISE_ADAM; host copy not read).  bias_factor_device serves the whole group.  The
 * other parameters as above and as in cuembed_sparse_row_adam. */
void cuembed_sparse_row_adam_grouped(const void* const* tables_host, const void* const* tables_device,
                                     const void* const* exp_avg_host, const void* const* exp_avg_device,
                                     const void* const* exp_avg_sq_host, const void* const* exp_avg_sq_device,
                                     int num_tables, int elem_type, int embed_width, const int64_t* row_base, int rule,
                                     const void* ids, int index_type, const void* rows, int64_t total_entries,
                                     int64_t num_rows, const void* count_word, int count_word_is_64, const void* last_id,
                                     float lr, const float* lr_device, float bias_factor, const float* bias_factor_device,
                                     float beta1, float one_minus_beta1, float beta2, float one_minus_beta2, float eps,
                                     float weight_decay, cuembed_stream_t stream);
/* The two grouped steps with STOCHASTIC ROUNDING (CUEMBED_F16 / CUEMBED_BF16 tables; CUEMBED_F32 is a bad type): the
 * arguments of the functions above, then seeds_device -- num_tables uint64 seeds in DEVICE memory, ONE PER TABLE, required
 * -- and the step, one value for the group: `step`, or step_device (one int64 word on the device, read by the kernel;
 * advance it on the device and a replayed graph draws fresh bits).  The one rounding of entry k draws the bits of
 * (seeds[t], step, id - row_base[t], column), t the entry's table: those of cuembed_sparse_row_update_stochastic /
 * cuembed_sparse_row_adam_stochastic on table t alone with seed = seeds[t], so a table's bits depend neither on the group
 * it is in nor on its place there.  (Not the bits of the single-table step on the tables laid end to end in one
 * allocation: that one names them by the global row.)  Arithmetic and state as with round to nearest. */
void cuembed_sparse_row_update_grouped_stochastic(const void* const* tables_host, const void* const* tables_device,
                                                  const void* const* state_host, const void* const* state_device,
                                                  int num_tables, int elem_type, int embed_width, const int64_t* row_base,
                                                  int rule, const void* ids, int index_type, const void* rows,
                                                  int64_t total_entries, int64_t num_rows, const void* count_word,
                                                  int count_word_is_64, const void* last_id, float lr,
                                                  const float* lr_device, float eps, const uint64_t* seeds_device,
                                                  uint64_t step, const int64_t* step_device, cuembed_stream_t stream);
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
                                                cuembed_stream_t stream);
/* ---- extension: the device-side index check (cuembed::CheckIndices, index_check.hpp) ---------------------------------
 * Is this batch safe to hand to the row-addressing calls above, which all trust their indices and offsets?  Never reads
 * a table, reads nothing back, allocates nothing, capturable.  n = num_tables * batch_per_table bags, table-major.  Row
 * counts: row_base[num_tables + 1] (int64, device, as for cuembed_grouped_backward_keys), or row_base == NULL and ONE
 * table of num_rows rows; every table has at least one row.  num_tables <= 1023.
 *   CSR (num_hots == 0, offsets[n + 1] of offset_type): position i is bad iff o[i] < 0, o[i] > nnz, or i > 0 and o[i] <
 *     o[i - 1]; the repaired offsets r are the running maximum clamped into [0, nnz].  Checked indices: [r[0], r[n]);
 *     position p belongs to the table t with r[t * batch_per_table] <= p < r[(t + 1) * batch_per_table].
 *   Fixed hotness (num_hots > 0, offsets == NULL, nnz == n * num_hots): every position is checked, t = p /
 *     (batch_per_table * num_hots).
 *   p is bad iff indices[p] < 0 or indices[p] >= rows_t (64-bit comparison); the repaired index is 0 where bad.
 * report: int64[4] on the device, initialised by the call: [bad indices, first (smallest) bad index position or -1, bad
 * offsets, first bad offset position or -1].  indices_out / offsets_out: NULL (report only), the input (in place), or a
 * separate array of the same type; bit-identical copies on a clean batch; positions outside the checked range are
 * copied through.  Any garbage in either array is a defined input: nothing is addressed with an unchecked value.
 * Two-phase workspace query: work == NULL writes the bytes needed to *lwork (0 for fixed hotness, which still needs a
 * non-NULL work to run) and runs nothing.  Launches: 3 (CSR), 2 (fixed hotness); one fewer for nnz == 0. */
void cuembed_check_indices(const void* indices, int index_type, const void* offsets, int offset_type, int64_t nnz,
                           const int64_t* row_base, int64_t num_rows, int num_tables, int batch_per_table, int num_hots,
                           int64_t* report, void* indices_out, void* offsets_out, char* work, size_t* lwork,
                           cuembed_stream_t stream);
/* hipPeekAtLastError() as an int (0 = hipSuccess); launches themselves never
 * report errors, exactly like the reference. */
int cuembed_peek_last_error(void);
/* "cuembed_amd <version> gfx950" */
const char* cuembed_version(void);

#ifdef __cplusplus
}
#endif

#endif /* CUEMBED_AMD_H_ */
