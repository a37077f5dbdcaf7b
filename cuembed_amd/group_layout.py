"""What every entry point on a GROUP of tables shares on the host, in one place each (pure Python: a group of CPU tensors
can be built and inspected without the library):

    GroupTables          base of TableGroup and MixedTableGroup: the tensor list, its pointers, the row prefix sums
    BagGroupModule       base of the *EmbeddingBagGroup modules: mode, bounds_check, the call shape
    group_batch_layout   THE bag-layout check of a grouped call: CSR xor fixed hotness, the counts, the batch size
    bag_offsets_layout   ... its part for a call whose batch size is known (the mean scales)
    check_weights        the per-lookup weights of a grouped call
    mixed_lane_bytes     THE lane rule of a mixed-width group (detail::PlanMixedGroupColumns on the C++ side)
"""
import ctypes

import torch

from .ops import _CSR_XOR_FIXED, _index_code

INT_MAX = 2 ** 31 - 1
_BOUNDS_CHECKS = (None, "raise", "repair")


def mixed_lane_bytes(widths, itemsize, pointers=()):
    """Bytes of a row one lane moves in a launch on a mixed-width group (16, 8 or 4), ONE value for the launch: the widest
    that every pointer of `pointers` -- (name, address) pairs --, D * itemsize, every column base * itemsize and every
    width * itemsize are a multiple of (the least aligned one decides).  ValueError for a pointer that is not 4-byte
    aligned, where the library would abort."""
    bits = column = 0
    for name, p in pointers:
        p = int(p)
        if p % 4:
            raise ValueError("%s must be 4-byte aligned: its data pointer is %d bytes past a 4-byte boundary" % (name, p % 4))
        bits |= p
    for w in widths:
        row = w * itemsize
        column += row
        bits |= row | column
    return 16 if bits % 16 == 0 else (8 if bits % 8 == 0 else 4)


def _check_bag_count(num_tables, batch_size):
    if num_tables * batch_size > INT_MAX:
        raise ValueError("num_tables * batch_size = %d does not fit a 32-bit int" % (num_tables * batch_size))


def csr_batch_size(num_tables, offsets_count):
    """batch_size of CSR offsets of num_tables * batch_size + 1 entries, or None where the count is no such number."""
    if offsets_count < 1 or (offsets_count - 1) % num_tables:
        return None
    return (offsets_count - 1) // num_tables


def bag_offsets_layout(num_tables, offsets, batch_size, num_hots):
    """CSR (offsets given, num_hots == 0) xor fixed hotness (offsets None, num_hots > 0), and for CSR the offsets:
    num_tables * batch_size + 1 int32 / int64 entries, batch_size inferred from their count when None.  Returns
    (batch_size, offset code); a fixed-hotness batch_size comes back as it was given."""
    if not ((offsets is not None and num_hots == 0) or (offsets is None and num_hots > 0)):
        raise ValueError(_CSR_XOR_FIXED)
    if offsets is None:
        return batch_size, 0
    if not isinstance(offsets, torch.Tensor):
        raise TypeError("offsets must be a torch.Tensor")
    ot = _index_code("offsets", offsets)
    if batch_size is None:
        batch_size = csr_batch_size(num_tables, offsets.numel())
        if batch_size is None:
            raise ValueError("offsets must hold num_tables * batch_size + 1 entries: %d - 1 is not a multiple of %d "
                             "tables" % (offsets.numel(), num_tables))
    if batch_size < 0 or offsets.numel() != num_tables * batch_size + 1:
        raise ValueError("offsets must hold num_tables * batch_size + 1 = %d entries, got %d"
                         % (num_tables * batch_size + 1, offsets.numel()))
    return batch_size, ot


def group_batch_layout(num_tables, indices, offsets, batch_size, num_hots, *, max_nnz=None):
    """The bag layout of one grouped call, validated without the GPU: (batch_size, nnz, index code, offset code).  The
    only place that decides CSR against fixed hotness and infers batch_size (None) from the counts.  max_nnz: the most
    lookups the caller's pipeline takes."""
    if not isinstance(indices, torch.Tensor):
        raise TypeError("indices must be a torch.Tensor")
    it = _index_code("indices", indices)
    batch_size, ot = bag_offsets_layout(num_tables, offsets, batch_size, num_hots)
    nnz = indices.numel()
    if offsets is None:
        if batch_size is None:
            if nnz % (num_tables * num_hots):
                raise ValueError("indices.numel() is not a multiple of num_tables * num_hots")
            batch_size = nnz // (num_tables * num_hots)
        if batch_size < 0 or nnz != num_tables * batch_size * num_hots:
            raise ValueError("indices must hold num_tables * batch_size * num_hots entries")
    _check_bag_count(num_tables, batch_size)
    if max_nnz is not None and nnz > max_nnz:
        raise ValueError("%d lookups: the backward pipeline takes at most 2^31 - 1" % nnz)
    return batch_size, nnz, it, ot


def mean_scale_layout(num_tables, offsets, batch_size, num_hots):
    """bag_offsets_layout for a mean scale, whose batch_size is grad_y's."""
    bag_offsets_layout(num_tables, offsets, batch_size, num_hots)
    _check_bag_count(num_tables, batch_size)


def check_weights(dtype, weights, nnz):
    if not isinstance(weights, torch.Tensor):
        raise TypeError("weights must be a torch.Tensor")
    if weights.dtype != dtype:
        raise TypeError("weights must be %s, got %s" % (dtype, weights.dtype))
    if weights.numel() < nnz:
        raise ValueError("weights must have one entry per index")


class GroupTables:
    """T >= 1 contiguous 2-D tables of one device and dtype, kept alive, with their base pointers on the host
    (`host_ptrs`) and in `table_ptrs`, ONE int64 device tensor that the kernels read -- built here, once -- and the
    prefix sums of their row counts.  A subclass says what a table may be: _first_table(first) validates table 0 and
    takes what the class derives from it, _check_table(k, t, first) validates every table against it."""

    def __init__(self, tables, table_ptrs=None):
        tables = list(tables)
        if not tables:
            raise ValueError("a %s needs at least one table" % type(self).__name__)
        for t in tables:
            if not isinstance(t, torch.Tensor):
                raise TypeError("every table must be a torch.Tensor")
        first = tables[0]
        self._first_table(first)
        for k, t in enumerate(tables):
            if t.dtype != first.dtype:
                raise TypeError("table %d is %s, table 0 is %s: one dtype per group" % (k, t.dtype, first.dtype))
            self._check_table(k, t, first)
            if t.device != first.device:
                raise ValueError("table %d is on %s, table 0 on %s: one device per group" % (k, t.device, first.device))
            if not t.is_contiguous():
                raise ValueError("table %d must be contiguous" % k)
        self.tables = tuple(tables)
        self.device = first.device
        self.dtype = first.dtype
        self.host_ptrs = tuple(int(t.data_ptr()) for t in tables)
        self._host_array = (ctypes.c_void_p * len(tables))(*self.host_ptrs)
        if table_ptrs is None:   # (a CPU group can be built and inspected; calls need the GPU)
            table_ptrs = torch.tensor(self.host_ptrs, dtype=torch.int64, device=self.device)
        elif (not isinstance(table_ptrs, torch.Tensor) or table_ptrs.dtype != torch.int64 or
              table_ptrs.numel() != len(tables) or table_ptrs.device != self.device or not table_ptrs.is_contiguous()):
            # (an earlier group's tensor for the same tables; its values stay on the device, unread)
            raise ValueError("table_ptrs must be the contiguous int64 tensor of the tables' data pointers on their device")
        self.table_ptrs = table_ptrs
        self.row_counts = tuple(int(t.shape[0]) for t in tables)
        self._row_base_device = None

    @property
    def row_counts(self):
        return self._row_counts

    @row_counts.setter
    def row_counts(self, counts):
        """Sets row_counts and, once, row_base: the host tuple of num_tables + 1 ints, the exclusive prefix sum of
        row_counts.  Table t owns the global rows [row_base[t], row_base[t + 1]) of the tables laid end to end."""
        self._row_counts = tuple(counts)
        base = [0]
        for n in self._row_counts:
            base.append(base[-1] + n)
        self.row_base = tuple(base)

    @property
    def total_rows(self):
        return self.row_base[-1]

    @property
    def row_base_device(self):
        """row_base as ONE int64 device tensor of num_tables + 1 entries (what the grouped backward's kernels and
        check_indices read) -- built at the first use, once."""
        if self._row_base_device is None:
            self._row_base_device = torch.tensor(self.row_base, dtype=torch.int64, device=self.device)
        return self._row_base_device

    def __len__(self):
        return len(self.tables)

    @property
    def num_tables(self):
        return len(self.tables)


class BagGroupModule:
    """What the *EmbeddingBagGroup modules share -- a group of tables with a mode and the call shape of nn.EmbeddingBag:
    bags(idx, offsets, weights) with CSR offsets (num_tables * batch + 1 entries), or bags(idx) with idx [num_tables,
    batch, hotness].  Forward only.  bounds_check: None (the batch is trusted), "raise" or "repair" (_checked_batch); the
    last check is kept as .last_check.  A subclass sets .group and gives __call__, which begins with _batch()."""

    def __init__(self, mode, bounds_check):
        if mode not in ("sum", "mean"):
            raise ValueError("mode must be 'sum' or 'mean'")
        if bounds_check not in _BOUNDS_CHECKS:
            raise ValueError("bounds_check must be None, 'raise' or 'repair'")
        self.mode = mode
        self.bounds_check = bounds_check
        self.last_check = None

    @property
    def num_tables(self):
        return self.group.num_tables

    def _batch(self, idx, offsets):
        """(idx, offsets, hotness) as the forward takes them: the hotness from idx's shape, the batch checked."""
        hot = 0
        if offsets is None:
            if idx.dim() != 3:
                raise ValueError("without offsets, idx must be [num_tables, batch, hotness]")
            hot = idx.shape[2]
        idx, offsets = _checked_batch(self, idx, offsets, hot)
        return idx, offsets, hot


def _checked_batch(bags, idx, offsets, hot):
    """The batch a group module hands to its forward.  bounds_check None: the caller's, untouched (ids outside their table
    are then a contract violation).  "repair": cuembed_amd.check_indices with repair runs on the stream in front of the
    forward, which gets the repaired arrays; the report stays on the device as bags.last_check -- no synchronisation.
    "raise": the check, then IndexCheck.raise_if_bad() (one synchronisation) before the forward is launched."""
    if bags.bounds_check is None:
        return idx, offsets
    from .index_check import check_indices
    check = check_indices(idx, offsets, group=bags.group, num_hots=hot, repair=bags.bounds_check == "repair")
    bags.last_check = check
    if bags.bounds_check == "raise":
        check.raise_if_bad()
    return check.indices, check.offsets
