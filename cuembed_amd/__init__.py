"""cuembed_amd -- MI355X-native (gfx950 / CDNA4) embedding lookup.

The gather-reduce hot path of NVIDIA/cuEmbed (EmbeddingForward, EmbeddingBackward,
Transpose and the index helpers) as hand-written HIP kernels behind
 * a header-only C++ host API   (cuembed_amd/csrc/cuembed/include/*.hpp),
 * a C ABI shared library       (include/cuembed_amd.h, cuembed_amd/lib/libcuembed_amd.so),
 * this Python host layer       (cuembed_amd.ops; the torch op surface of the reference's examples/pytorch is
                                 cuembed_amd.cuembed_pyt over cuembed_amd/lib/libcuembed_pyt.so).
"""
from . import _lib  # noqa: F401
from .ops import (CONCAT, MEAN, SUM, ComputeCompressedGradIndices, EmbeddingBackward,  # noqa: F401
                  EmbeddingForward, ExtractRowIdsForConcat, ExtractRowIdsFromCSR,
                  ExtractRowIdsFromFixed, Transpose, compressed_grad_workspace_bytes,
                  compute_compressed_grad_indices, compute_compressed_grad_indices_blocked,
                  compressed_grad_blocked_workspace_bytes, SHARED_ROW_BIT, embedding_backward, embedding_forward,
                  get_backward_tuning, set_backward_tuning, recommended_sample_blocks, transpose_sample_block_length,
                  embedding_weight_grad, bag_order_by_length, capacity_overflowed, decide_row_loads,
                  new_row_loads_decision,
                  extract_row_ids_for_concat, extract_row_ids_from_csr,
                  extract_row_ids_from_fixed, forward_launch_shape, backward_launch_shape, device_shape, get_forward_reduction_order,
                  set_forward_reduction_order, set_forward_row_load_policy, get_forward_row_load_policy, set_forward_wide_load, transpose,
                  transpose_fixed_hotness,
                  transpose_workspace_bytes, sparse_row_update, sparse_row_update_launch_shape, UPDATE_RULES,
                  stochastic_rounding_words, stochastic_round, stochastic_round_array, sparse_row_adam,
                  adam_bias_factor, new_adam_clock, adam_clock_advance, ADAM_RULES)
from .quantized import (QuantizedEmbeddingBag, dequantize_rows, embedding_forward_quantized,  # noqa: F401
                        quantize_rows, quantized_forward_launch_shape, quantized_row_bytes)
from .grouped import (EmbeddingBagGroup, QuantizedEmbeddingBagGroup, TableGroup,  # noqa: F401
                      embedding_forward_grouped, embedding_forward_quantized_grouped, grouped_forward_launch_shape)
from .mixed_group import (MixedEmbeddingBagGroup, MixedTableGroup, embedding_forward_mixed_group,  # noqa: F401
                          mixed_group_launch_shape)
from .grouped_backward import (GroupedGrad, embedding_backward_grouped, embedding_weight_grad_grouped,  # noqa: F401
                               grouped_backward_keys, grouped_mean_scale, grouped_table_cuts,
                               sparse_row_adam_grouped, sparse_row_update_grouped)
from .mixed_group_backward import (MixedGroupedGrad, embedding_backward_mixed_group,  # noqa: F401
                                   mixed_group_backward_launch_shape, mixed_group_mean_scale)
from .index_check import (IndexCheck, check_indices, check_indices_workspace_bytes,  # noqa: F401
                          new_index_report)

__version__ = "0.1.0"
