"""The forward on a group of embedding tables of DIFFERENT widths in one launch (an extension: sum / mean only, plain
fp32 / fp16 / bf16 tables of one dtype).

cuembed_amd.grouped pools T tables of ONE width; a model whose widths follow the tables' cardinality would need one such
group per width and a torch.cat over the results.  Here the widths may all differ and the kernel writes the
concatenated layout itself:

    bag g = t * B + b        table t, sample b (exactly the same-width group's input layout)
    CSR                      one indices[nnz], one offsets[T * B + 1], optional weights[nnz]
    fixed hotness            indices [T, B, H] (offsets=None, num_hots=H), the same H for every table
    out                      [B, D], D = sum of the widths; bag (t, b) at out[b, c_t : c_t + W_t], c_t the exclusive
                             prefix sum of the widths -- torch.cat(per_table_results, dim=1), with the same bits

    MixedTableGroup(tables)                     the tables, their pointers (host and device) and widths
    embedding_forward_mixed_group(group, ...)   embedding_forward on the group, one launch
    mixed_group_launch_shape(...)               the launch shape (host arithmetic)
    MixedEmbeddingBagGroup                      a group with a mode: bags(idx, offsets, weights)

Every function validates its arguments and raises before any launch; the kernel runs on torch's current stream
(cuembed::EmbeddingForwardMixedGroup through the C ABI).  The kernel reads a small per-table descriptor from device
memory; MixedTableGroup builds it once per (batch size, lane width) -- one host-to-device copy at the FIRST call of a
shape (or at group.descriptor(B, lane_bytes)), none afterwards -- so with `out=` given every later call copies nothing,
allocates nothing and can be captured into a HIP graph.  The functions here are forward only and refuse tensors that
require grad; the backward is cuembed_amd.mixed_group_backward (autograd:
cuembed_pyt.cuemb_embedding_mixed_group_trainable).  There is no sample_order, no per-table row-load decision, no
quantized and no mixed-dtype group.
"""
import ctypes

import torch

from . import _lib
from .group_layout import INT_MAX, BagGroupModule, GroupTables, mixed_lane_bytes
from .grouped import _grouped_args, _grouped_devices
from .ops import _ELEM, _INDEX, _ROW_LOADS, _check_dev, _ptr, _stream

BLOCK_THREADS = 256        # cuembed::kMixedGroupBlockThreads


class MixedTableGroup(GroupTables):
    """T >= 1 contiguous 2-D tables [rows_t, W_t] of one device and one dtype (float32 / float16 / bfloat16); the widths
    and row counts may all differ, every row is a multiple of 4 bytes.  Holds the tensors (so that the pointers stay
    valid), their base pointers and widths on the host, `table_ptrs` (ONE int64 device tensor of the pointers, which the
    kernel reads) and the device descriptors, one per (batch size, lane width), each built at its first use.  A group of
    CPU tensors can be built and inspected; calls need the GPU."""

    quantized = False

    def __init__(self, tables, table_ptrs=None):
        super().__init__(tables, table_ptrs)
        self.widths = tuple(int(t.shape[1]) for t in self.tables)
        base = [0]
        for w in self.widths:
            base.append(base[-1] + w)
        if base[-1] > INT_MAX:
            raise ValueError("the widths sum to %d, which does not fit a 32-bit int" % base[-1])
        self.column_base = tuple(base)
        self._widths_array = (ctypes.c_int * len(self.tables))(*self.widths)
        self._named_ptrs = None          # (name, pointer) of every table, for lane_bytes(): built at its first call
        self._table_columns_device = None
        self._descriptors = {}

    def _first_table(self, first):
        if first.dtype not in _ELEM:
            raise TypeError("tables must be float32, float16 or bfloat16, got %s" % first.dtype)

    def _check_table(self, k, t, first):
        if t.dim() != 2:
            raise ValueError("table %d is %s: every table must be [rows, width]" % (k, tuple(t.shape)))
        if t.shape[1] <= 0 or (t.shape[1] * t.element_size()) % 4:
            raise ValueError("table %d: the row size must be a multiple of 4 bytes, got %d elements of %d"
                             % (k, t.shape[1], t.element_size()))

    @property
    def embedding_dim(self):
        """D: the columns of a result row, the sum of the widths."""
        return self.column_base[-1]

    @property
    def table_columns_device(self):
        """int32 [num_tables, 2] on the device: (column base c_t, width W_t) of every table in elements -- what the
        backward's kernels read per lookup (cuembed_amd.mixed_group_backward).  Built at the first use, once."""
        if self._table_columns_device is None:
            self._table_columns_device = torch.tensor(list(zip(self.column_base[:-1], self.widths)), dtype=torch.int32,
                                                      device=self.device)
        return self._table_columns_device

    def lane_bytes(self, out_ptr=0):
        """Bytes of a row one lane moves (16, 8 or 4), ONE value for the launch: the widest that every table base,
        `out_ptr`, D * itemsize, every column base * itemsize and every width * itemsize are a multiple of (the least
        aligned one decides).  ValueError where the library would abort."""
        if self._named_ptrs is None:
            self._named_ptrs = tuple(("tables[%d]" % k, p) for k, p in enumerate(self.host_ptrs))
        return mixed_lane_bytes(self.widths, self.tables[0].element_size(), self._named_ptrs + (("out", out_ptr),))

    def descriptor_words(self, batch_size, lane_bytes):
        """The descriptor of (batch_size, lane_bytes) on the host (cuembed_fill_mixed_group_descriptor: host arithmetic):
        (grid, list of (num_tables + 1) * 4 ints -- per table width, column base, lanes per bag, first workgroup)."""
        T = self.num_tables
        if batch_size < 0 or T * batch_size > INT_MAX:
            raise ValueError("num_tables * batch_size = %d does not fit a 32-bit int" % (T * batch_size))
        if lane_bytes not in (16, 8, 4) or lane_bytes > self.lane_bytes():
            raise ValueError("lane_bytes must be 16, 8 or 4 and at most what the group allows (%d)" % self.lane_bytes())
        L = _lib.lib()
        nbytes = L.cuembed_mixed_group_descriptor_bytes(T)
        blob = (ctypes.c_int32 * (nbytes // 4))()
        grid = L.cuembed_fill_mixed_group_descriptor(self._widths_array, T, self.tables[0].element_size(), lane_bytes,
                                                     int(batch_size), BLOCK_THREADS, blob)
        return grid, list(blob)

    def descriptor(self, batch_size, lane_bytes):
        """The device descriptor of (batch_size, lane_bytes): an int32 tensor, built and copied to the device at the
        first use of the pair and kept.  Call it ahead of a graph capture (or run the call once)."""
        key = (int(batch_size), int(lane_bytes))
        if key not in self._descriptors:
            _, words = self.descriptor_words(*key)
            self._descriptors[key] = torch.tensor(words, dtype=torch.int32, device=self.device)
        return self._descriptors[key]


def _as_mixed_group(group):
    return group if isinstance(group, MixedTableGroup) else MixedTableGroup(group)


def embedding_forward_mixed_group(group, indices, offsets=None, weights=None, batch_size=None, num_hots=0, mode="sum",
                                  row_loads=None, out=None, sample_order=None, row_loads_device=None):
    """out[b, c_t : c_t + W_t] = combine_j weights[.] * group.tables[t][indices[.]] over the lookups of bag
    t * batch_size + b, for all tables of a MixedTableGroup (or a list of tables: a group is then built, with its
    host-to-device copies) in ONE launch.  Returns [batch_size, D] of the tables' dtype -- torch.cat([embedding_forward(
    table_t, ...)], dim=1), bit for bit.

    CSR: offsets[num_tables * batch_size + 1] over one indices[nnz]; fixed hotness: offsets=None, num_hots=H, indices
    [num_tables, batch_size, H].  The ids of table t's bags are rows of table t.  mode "sum" | "mean"; weights (optional)
    in the tables' dtype; fp32 accumulation in lookup order; empty bags give zeros.  row_loads ("default" | "streaming" |
    None, one value for the group) changes no bit.  sample_order and row_loads_device must stay None."""
    group = _as_mixed_group(group)
    if sample_order is not None:
        raise ValueError("sample_order is not taken by the mixed-width forward in this version")
    batch_size, m, it, ot = _grouped_args(group, indices, offsets, weights, batch_size, num_hots, mode, row_loads, None,
                                          row_loads_device, group.dtype)
    T, D = group.num_tables, group.embedding_dim
    if out is not None:
        if not isinstance(out, torch.Tensor):
            raise TypeError("out must be a torch.Tensor")
        if out.dtype != group.dtype or out.numel() != batch_size * D:
            raise ValueError("out must be a contiguous %s tensor [batch_size, embedding_dim] = [%d, %d]"
                             % (group.dtype, batch_size, D))
    dev = _grouped_devices(group, indices, offsets, weights)
    if out is None:
        out = torch.empty((batch_size, D), dtype=group.dtype, device=dev)
    else:
        _check_dev("out", out, dev)
    lane = group.lane_bytes(out.data_ptr())
    if batch_size > 0:
        descriptor = group.descriptor(batch_size, lane)
        with torch.cuda.device(dev):   # the launch must happen on the tensors' device
            _lib.lib().cuembed_embedding_forward_mixed_group(
                group._host_array, _ptr(group.table_ptrs), group._widths_array, _ptr(descriptor), T, _ELEM[group.dtype],
                _ptr(indices), it, _ptr(offsets), ot, _ptr(weights), batch_size, num_hots, m, _ptr(out),
                _ROW_LOADS[row_loads], _stream(out))
    return out


def mixed_group_launch_shape(elem_dtype, index_dtype, widths, batch_size, num_hots=0, is_weighted=False, pointer_bits=0):
    """Launch shape of a mixed-width forward (pure host arithmetic).  pointer_bits: the table bases and out OR-ed (0 =
    aligned buffers).  A workgroup of block_threads serves bags of ONE table: table t takes L_t = min(W_t /
    elems_per_lane, block_threads) lanes per bag and block_threads // L_t bags per workgroup; grid = sum_t ceil(
    batch_size / bags per workgroup of t).  num_hots == 0: CSR."""
    if elem_dtype not in _ELEM:
        raise TypeError("elem_dtype must be float32, float16 or bfloat16, got %s" % elem_dtype)
    if index_dtype not in _INDEX:
        raise TypeError("index dtype must be int32 or int64, got %s" % index_dtype)
    widths = [int(w) for w in widths]
    T = len(widths)
    if T < 1 or batch_size < 0 or T * batch_size > INT_MAX or num_hots < 0:
        raise ValueError("num_tables >= 1, batch_size >= 0, num_hots >= 0 and num_tables * batch_size must fit a 32-bit int")
    if any(w <= 0 or (w * elem_dtype.itemsize) % 4 for w in widths) or sum(widths) > INT_MAX:
        raise ValueError("every row size must be a multiple of 4 bytes and the widths must sum to at most 2^31 - 1")
    if pointer_bits % 4:
        raise ValueError("every pointer must be 4-byte aligned")
    out = (ctypes.c_int * 7)()
    _lib.lib().cuembed_mixed_group_launch_shape((ctypes.c_int * T)(*widths), T, _ELEM[elem_dtype], _INDEX[index_dtype],
                                                int(batch_size), int(num_hots), int(bool(is_weighted)),
                                                int(pointer_bits), out)
    return dict(elems_per_lane=out[0], block_threads=out[1], grid=out[2], embedding_dim=out[3], lds_bytes=out[4],
                staged=out[5] == 1, max_bags_per_block=out[6])


class MixedEmbeddingBagGroup(BagGroupModule):
    """A MixedTableGroup with a mode and the call shape of nn.EmbeddingBag: bags(idx, offsets, weights) with CSR offsets
    (num_tables * batch + 1 entries), or bags(idx) with idx [num_tables, batch, hotness].  Returns [batch, embedding_dim].
    Forward only.  bounds_check: None (the batch is trusted), "raise" or "repair" (cuembed_amd.check_indices in front of
    the forward, as in EmbeddingBagGroup); the last check is kept as .last_check."""

    def __init__(self, tables, mode="sum", bounds_check=None):
        super().__init__(mode, bounds_check)
        self.group = _as_mixed_group(tables)

    @property
    def embedding_dim(self):
        return self.group.embedding_dim

    def __call__(self, idx, offsets=None, weights=None, out=None):
        idx, offsets, hot = self._batch(idx, offsets)
        return embedding_forward_mixed_group(self.group, idx, offsets, weights, num_hots=hot, mode=self.mode, out=out)
