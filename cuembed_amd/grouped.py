"""The forward on a GROUP of embedding tables in one launch (an extension: forward only, sum / mean only).

A model with T tables calls embedding_forward T times and stacks the results; here the bags of T tables of one width
and dtype lie one table after the other and one kernel pools them all:

    bag g = t * B + b        table t, sample b (B samples per table; the table-major order of FBGEMM's table-batched op)
    CSR                      one indices[nnz], one offsets[T * B + 1], optional weights[nnz]
    fixed hotness            indices [T, B, H] (offsets=None, num_hots=H), the same H for every table
    out                      [B, T, W], contiguous -- torch.stack(per_table_results, dim=1), with the same bits

    TableGroup(tables)                          the tables + their base pointers on the host and (built once) on the device
    embedding_forward_grouped(group, ...)       embedding_forward on a group of fp32 / fp16 / bf16 tables
    embedding_forward_quantized_grouped(...)    embedding_forward_quantized on a group of fused 8-bit tables
    grouped_forward_launch_shape(...)           the launch shape (host arithmetic)
    EmbeddingBagGroup, QuantizedEmbeddingBagGroup   a group with a mode: bag(idx, offsets, weights)

Every function validates its arguments and raises before any launch; the kernels run on torch's current stream
(cuembed::EmbeddingForwardGrouped / EmbeddingForwardQuantizedGrouped through the C ABI).  No host read-back, no copy per
call, no allocation inside the library: with `out=` given a call can be captured into a HIP graph.  Nothing here is
differentiable: a table that requires grad while grad mode is on is an error.  A group is trained through
cuembed_amd.grouped_backward (embedding_backward_grouped: one sort and one scatter-add for all tables) and, with
autograd, cuembed_amd.cuembed_pyt.cuemb_embedding_grouped_trainable; TableGroup.allocate / from_flat put a group into
one storage so that the sparse optimizers apply to it as they are.
"""
import ctypes

import torch

from . import _lib
from .group_layout import INT_MAX, BagGroupModule, GroupTables, check_weights, group_batch_layout
from .ops import _ELEM, _INDEX, _MODES, _ROW_LOADS, MEAN, SUM, _check_alignment, _check_dev, _ptr, _stream
from .quantized import TRAILER_BYTES, _check_qtable, _out_code, quantize_rows

_SOURCES = ("lds_staged", "wave_shuffle", "global")


class TableGroup(GroupTables):
    """T >= 1 tables of one device, dtype and width (their row counts may differ): all 2-D float32 / float16 / bfloat16
    [rows_t, W], or all fused 8-bit tables, uint8 [rows_t, W + 8].  Holds the tensors (so that the pointers stay
    valid), their base pointers on the host, and `table_ptrs`, ONE int64 device tensor of the same pointers that the
    kernel reads -- built here, once: no host-to-device copy per call.  A tensor whose storage is replaced later
    (`table.data = ...`) needs a new TableGroup; updating rows in place does not."""

    def __init__(self, tables, table_ptrs=None):
        super().__init__(tables, table_ptrs)
        self.flat = None                 # the one storage of allocate() / from_flat(); None for separate tensors
        self._state_ptr_arrays = {}      # the pointer arrays of per-table optimizer state (grouped_backward._state_ptrs)
        self._seed_arrays = {}           # the per-table rounding seeds on the device (grouped_backward._seeds_tensor)

    def _first_table(self, first):
        self.quantized = first.dtype == torch.uint8
        if self.quantized:
            self.width = _check_qtable(first)
        else:
            if first.dtype not in _ELEM:
                raise TypeError("tables must be float32, float16 or bfloat16 (or fused uint8 rows), got %s" % first.dtype)
            if first.dim() != 2:
                raise ValueError("every table must be [rows, width]")
            self.width = first.shape[1]

    def _check_table(self, k, t, first):
        if t.dim() != 2 or t.shape[1] != first.shape[1]:
            raise ValueError("table %d is %s, table 0 has rows of %d: one width per group"
                             % (k, tuple(t.shape), first.shape[1]))

    @classmethod
    def from_flat(cls, flat, row_counts):
        """A group whose tables are row slices of ONE [total_rows, width] tensor the caller owns: table t is
        flat[row_base[t]:row_base[t + 1]], so a global row id of the grouped backward is directly a row of `flat` and a
        sparse optimizer step on `flat` (cuembed_amd.sparse_row_update, sparse_row_adam, cuembed_amd.optim) trains the
        whole group.  `flat` may be an nn.Parameter: the views (and the pointer table) are taken from flat.detach(),
        `flat` itself is kept as group.flat -- what cuemb_embedding_grouped_trainable differentiates with respect to.
        Float tables only.  A slice's base is only row-aligned (rows_t * width * itemsize bytes past the previous one):
        lane_bytes() already narrows the whole group to the least aligned pointer, so nothing else is needed."""
        if not isinstance(flat, torch.Tensor):
            raise TypeError("flat must be a torch.Tensor")
        if flat.dtype not in _ELEM:
            raise TypeError("a one-storage group holds float32, float16 or bfloat16 tables (a quantized group is a list "
                            "of fused tables), got %s" % flat.dtype)
        if flat.dim() != 2 or not flat.is_contiguous():
            raise ValueError("flat must be a contiguous [total_rows, width] tensor")
        counts = [int(n) for n in row_counts]
        if not counts or any(n < 0 for n in counts) or sum(counts) != flat.shape[0]:
            raise ValueError("row_counts must be non-negative and sum to flat.shape[0] = %d" % flat.shape[0])
        base, data, views = 0, flat.detach(), []
        for n in counts:
            views.append(data[base:base + n])
            base += n
        group = cls(views)
        group.flat = flat
        return group

    @classmethod
    def allocate(cls, row_counts, width, dtype=torch.float32, device="cuda"):
        """from_flat on ONE new zero-filled [sum(row_counts), width] tensor (group.flat)."""
        if dtype not in _ELEM:
            raise TypeError("a one-storage group holds float32, float16 or bfloat16 tables, got %s" % dtype)
        counts = [int(n) for n in row_counts]
        if not counts or any(n < 0 for n in counts) or width <= 0:
            raise ValueError("row_counts must be non-negative and width positive")
        return cls.from_flat(torch.zeros((sum(counts), int(width)), dtype=dtype, device=device), counts)

    def lane_bytes(self, out_ptr=0):
        """Bytes of a row one lane moves (16, 8 or 4; codes per lane for fused tables before the 16-code widening): the
        least aligned table -- and `out_ptr` -- decide for the whole group.  ValueError where the library would abort."""
        ptr = 0
        for p in self.host_ptrs:
            ptr |= p
        if self.quantized:
            return _check_alignment("tables", ptr, 1, self.width, codes=True)
        return _check_alignment("tables", ptr, self.tables[0].element_size(), self.width, others=(("out", out_ptr),))


def _as_group(group):
    return group if isinstance(group, TableGroup) else TableGroup(group)


def _check_no_grad(group, weights):
    if torch.is_grad_enabled():
        for k, t in enumerate(group.tables):
            if t.requires_grad:
                raise RuntimeError("table %d requires grad: the grouped forward is forward only (call it under "
                                   "torch.no_grad() or detach the tables)" % k)
        if weights is not None and weights.requires_grad:
            raise RuntimeError("weights require grad: the grouped forward is forward only")


def _grouped_args(group, indices, offsets, weights, batch_size, num_hots, mode, row_loads, sample_order, row_loads_device,
                  weight_dtype):
    """Validates the arguments of one grouped forward that do not need the GPU and returns (B, mode code, index code,
    offset code)."""
    if mode not in ("sum", "mean", SUM, MEAN):
        raise ValueError("mode must be 'sum' or 'mean': the grouped forward has no concat and no max")
    if row_loads not in _ROW_LOADS:
        raise ValueError("row_loads: None, 'default' or 'streaming'")
    if row_loads_device is not None:
        raise ValueError("row_loads_device is not taken by the grouped forward: the decision is per table and nothing "
                         "carries one per table yet; pass row_loads= for the whole group")
    _check_no_grad(group, weights)
    batch_size, nnz, it, ot = group_batch_layout(group.num_tables, indices, offsets, batch_size, num_hots)
    if weights is not None:
        check_weights(weight_dtype, weights, nnz)
    if sample_order is not None and offsets is None:
        raise ValueError("sample_order is a hint for CSR batches (bags of different lengths)")
    return batch_size, _MODES[mode], it, ot


def _grouped_devices(group, indices, offsets, weights):
    """The call is in order: now the devices."""
    dev = group.device
    _check_dev("tables[0]", group.tables[0])
    _check_dev("indices", indices, dev)
    if offsets is not None:
        _check_dev("offsets", offsets, dev)
    if weights is not None:
        _check_dev("weights", weights, dev)
    return dev


def _grouped_call(group, indices, offsets, weights, batch_size, num_hots, mode, row_loads, sample_order, out,
                  row_loads_device, weight_dtype, out_dtype):
    """Validates one same-width grouped call (everything that does not need the GPU first) and returns
    (B, mode code, index code, offset code, out)."""
    batch_size, m, it, ot = _grouped_args(group, indices, offsets, weights, batch_size, num_hots, mode, row_loads,
                                          sample_order, row_loads_device, weight_dtype)
    T = group.num_tables
    dev = _grouped_devices(group, indices, offsets, weights)
    if sample_order is not None:
        _check_dev("sample_order", sample_order, dev)
        if sample_order.dtype != torch.int32 or sample_order.numel() != T * batch_size:
            raise ValueError("sample_order must be a contiguous int32 permutation of range(num_tables * batch_size)")
    if out is None:
        out = torch.empty((batch_size, T, group.width), dtype=out_dtype, device=dev)
    else:
        _check_dev("out", out, dev)
        if out.dtype != out_dtype or out.numel() != batch_size * T * group.width:
            raise ValueError("out must be a contiguous %s tensor [batch_size, num_tables, width]" % out_dtype)
    return batch_size, m, it, ot, out


def embedding_forward_grouped(group, indices, offsets=None, weights=None, batch_size=None, num_hots=0, mode="sum",
                              row_loads=None, sample_order=None, out=None, row_loads_device=None):
    """out[b, t] = combine_j weights[.] * group.tables[t][indices[.]] over the lookups of bag t * batch_size + b, for all
    tables of a TableGroup (or a list of tables: a TableGroup is then built, with its one host-to-device copy) in ONE
    launch.  Returns [batch_size, num_tables, width] of the tables' dtype -- torch.stack([embedding_forward(table_t,
    ...)], dim=1), bit for bit.

    CSR: offsets[num_tables * batch_size + 1] over one indices[nnz]; fixed hotness: offsets=None, num_hots=H, indices
    [num_tables, batch_size, H].  The ids of table t's bags are rows of table t.  mode "sum" | "mean"; weights (optional)
    in the tables' dtype; fp32 accumulation in lookup order; empty bags give zeros.  row_loads ("default" | "streaming" |
    None, one value for the group) and sample_order (CSR only: an int32 permutation of the num_tables * batch_size bags,
    bag_order_by_length(offsets)) are scheduling hints that change no bit.  row_loads_device must stay None."""
    group = _as_group(group)
    if group.quantized:
        raise TypeError("a group of fused 8-bit tables is looked up with embedding_forward_quantized_grouped")
    B, m, it, ot, out = _grouped_call(group, indices, offsets, weights, batch_size, num_hots, mode, row_loads,
                                      sample_order, out, row_loads_device, group.dtype, group.dtype)
    group.lane_bytes(out.data_ptr())
    if B > 0:
        with torch.cuda.device(group.device):   # the launch must happen on the tensors' device
            _lib.lib().cuembed_embedding_forward_grouped(
                group._host_array, _ptr(group.table_ptrs), group.num_tables, _ELEM[group.dtype], group.width,
                _ptr(indices), it, _ptr(offsets), ot, _ptr(weights), B, num_hots, m, _ptr(out), _ROW_LOADS[row_loads],
                _ptr(sample_order), _stream(out))
    return out


def embedding_forward_quantized_grouped(group, indices, offsets=None, weights=None, batch_size=None, num_hots=0,
                                        mode="sum", out_dtype=torch.float16, row_loads=None, sample_order=None, out=None,
                                        row_loads_device=None):
    """embedding_forward_grouped on a TableGroup of fused 8-bit tables (uint8 [rows_t, W + 8], torch's
    embedding_bag_byte_prepack layout): returns [batch_size, num_tables, W] of out_dtype (float16 or float32) --
    torch.stack([embedding_forward_quantized(qtable_t, ...)], dim=1), bit for bit.  `weights` have the output's dtype."""
    group = _as_group(group)
    if not group.quantized:
        raise TypeError("embedding_forward_quantized_grouped takes fused uint8 tables [rows, width + 8]")
    oc = _out_code("out_dtype", out_dtype)
    B, m, it, ot, out = _grouped_call(group, indices, offsets, weights, batch_size, num_hots, mode, row_loads,
                                      sample_order, out, row_loads_device, out_dtype, out_dtype)
    if out.data_ptr() % 16 != 0:
        raise ValueError("out must be 16-byte aligned")
    group.lane_bytes()
    if B > 0:
        with torch.cuda.device(group.device):
            _lib.lib().cuembed_embedding_forward_quantized_grouped(
                group._host_array, _ptr(group.table_ptrs), group.num_tables, group.width, _ptr(indices), it,
                _ptr(offsets), ot, _ptr(weights), B, num_hots, m, _ptr(out), oc, _ROW_LOADS[row_loads],
                _ptr(sample_order), _stream(out))
    return out


def grouped_forward_launch_shape(elem_dtype, index_dtype, embed_width, num_tables, batch_size, num_hots, is_csr=False,
                                 is_weighted=False, quantized=False, compute_units=256, xcds=8):
    """Launch shape of a grouped forward for aligned buffers (pure host arithmetic; compute_units / xcds describe the
    device for quantized groups, whose plan depends on it: 0 = ask the current device).  elem_dtype: the tables' dtype,
    or with quantized=True the output's.  grid = ceil(num_tables * batch_size / samples_per_block); index_source is
    "lds_staged", "wave_shuffle" or "global"."""
    if index_dtype not in _INDEX:
        raise TypeError("index dtype must be int32 or int64, got %s" % index_dtype)
    if quantized:
        ec = _out_code("elem_dtype", elem_dtype)
    else:
        if elem_dtype not in _ELEM:
            raise TypeError("elem_dtype must be float32, float16 or bfloat16, got %s" % elem_dtype)
        ec = _ELEM[elem_dtype]
    if num_tables < 1 or batch_size < 0 or num_tables * batch_size > INT_MAX:
        raise ValueError("num_tables >= 1, batch_size >= 0 and num_tables * batch_size must fit a 32-bit int")
    if embed_width <= 0 or (embed_width * (1 if quantized else elem_dtype.itemsize)) % 4:
        raise ValueError("the row size must be a multiple of 4 bytes")
    out = (ctypes.c_int * 7)()
    _lib.lib().cuembed_grouped_forward_launch_shape(int(bool(quantized)), ec, _INDEX[index_dtype], int(embed_width),
                                                    int(num_tables), int(batch_size), int(num_hots), int(is_csr),
                                                    int(is_weighted), int(compute_units), int(xcds), out)
    return dict(elems_per_lane=out[0], lanes_per_row=out[1], samples_per_block=out[2], grid=out[3], lds_bytes=out[4],
                staged=out[5] == 1, index_source=_SOURCES[out[6]])


class EmbeddingBagGroup(BagGroupModule):
    """A TableGroup with a mode and the call shape of nn.EmbeddingBag: bags(idx, offsets, weights) with CSR offsets
    (num_tables * batch + 1 entries), or bags(idx) with idx [num_tables, batch, hotness].  Returns [batch, num_tables,
    width].  Forward only.  bounds_check: None (the batch is trusted), "raise" or "repair" (_checked_batch); the last
    check is kept as .last_check."""

    def __init__(self, tables, mode="sum", bounds_check=None):
        super().__init__(mode, bounds_check)
        self.group = _as_group(tables)
        if self.group.quantized:
            raise TypeError("fused 8-bit tables go into a QuantizedEmbeddingBagGroup")

    @property
    def embedding_dim(self):
        return self.group.width

    def __call__(self, idx, offsets=None, weights=None, sample_order=None, out=None):
        idx, offsets, hot = self._batch(idx, offsets)
        return embedding_forward_grouped(self.group, idx, offsets, weights, num_hots=hot, mode=self.mode,
                                         sample_order=sample_order, out=out)


class QuantizedEmbeddingBagGroup(BagGroupModule):
    """EmbeddingBagGroup on fused 8-bit tables; from_float quantizes fp32 / fp16 / bf16 tables on the device."""

    def __init__(self, qtables, mode="sum", out_dtype=torch.float16, bounds_check=None):
        super().__init__(mode, bounds_check)
        _out_code("out_dtype", out_dtype)
        self.group = _as_group(qtables)
        if not self.group.quantized:
            raise TypeError("QuantizedEmbeddingBagGroup takes fused uint8 tables; see from_float")
        self.out_dtype = out_dtype

    @classmethod
    def from_float(cls, tables, mode="sum", out_dtype=torch.float16, bounds_check=None):
        return cls([quantize_rows(t.detach()) for t in tables], mode=mode, out_dtype=out_dtype, bounds_check=bounds_check)

    @property
    def embedding_dim(self):
        return self.group.width

    def __call__(self, idx, offsets=None, weights=None, sample_order=None, out=None):
        idx, offsets, hot = self._batch(idx, offsets)
        return embedding_forward_quantized_grouped(self.group, idx, offsets, weights, num_hots=hot, mode=self.mode,
                                                   out_dtype=self.out_dtype, sample_order=sample_order, out=out)
