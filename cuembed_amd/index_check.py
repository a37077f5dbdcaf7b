"""The device-side index check: is a batch safe to hand to the kernels that address table rows?

Every row-addressing kernel of the library trusts its indices and offsets completely; one id at or beyond the row count,
one negative id from a hashing bug upstream or one decreasing offset is an illegal memory access (or, in a one-storage
group, a silent read of a neighbouring table's rows).  check_indices looks at the values ON THE DEVICE
(cuembed::CheckIndices through the C ABI): it never reads a table, reads nothing back, and leaves a four-word report in
device memory; with repair=True it also writes a copy of the batch that is safe by construction.

    check_indices(indices, offsets, num_rows= | group=, ...)    -> IndexCheck(report, indices, offsets)
    IndexCheck.raise_if_bad()                                    the only thing that synchronises: IndexError

Definitions (tests/index_check_reference.py is exactly this in numpy; n = num_tables * batch_size bags, table-major):
    offsets      position i in 0 .. n is bad iff o[i] < 0, o[i] > nnz, or i > 0 and o[i] < o[i - 1]; the repaired offsets
                 are the running maximum clamped into [0, nnz] (o[0] != 0 and o[n] != nnz are no errors);
    indices      checked range [r[0], r[n]) (CSR) or everything (fixed hotness); position p belongs to the table t with
                 r[t * B] <= p < r[(t + 1) * B], or t = p // (B * num_hots); bad iff indices[p] < 0 or >= rows_t; the
                 repaired index is 0 where bad; positions outside the checked range are copied through;
    report       int64[4]: [bad indices, first bad index position or -1, bad offsets, first bad offset position or -1].

Host checks, in this order, all before any launch: indices (a tensor of int32 / int64); exactly one of num_rows / group;
the row counts (every table at least one row, at most MAX_CHECK_TABLES tables); CSR or fixed hotness; offsets (tensor,
dtype, num_tables * batch_size + 1 entries); the lookup count; the outputs (only with repair=True; dtype, size, the input
itself or disjoint from it); then the devices (a CPU tensor: "no CPU fallback"), the report and the workspace.
"""
import ctypes

import torch

from . import _lib
from .group_layout import INT_MAX, group_batch_layout
from .grouped import _as_group
from .mixed_group import MixedTableGroup
from .ops import _check_dev, _index_code, _ptr, _stream

MAX_CHECK_TABLES = 1023    # detail::kCheckMaxTables: the cuts and row counts of a group are staged in 16 KiB of LDS
MAX_CHECK_NNZ = 1 << 38    # detail::kCheckMaxLookups: the index pass is ONE launch, 2^30 workgroups at one id per lane
SCAN_CHUNK = 1024          # detail::kCheckScanChunk: offsets per workgroup and trip of the offsets scan
MAX_SCAN_TILES = 1024      # detail::kCheckMaxTiles


class IndexCheck:
    """What check_indices returns.  `report`: the four int64 words on the device.  `indices` / `offsets`: what to hand to
    the forward -- the repaired arrays with repair=True, the inputs themselves otherwise (offsets is None for fixed
    hotness).  Nothing here synchronises except words() and raise_if_bad(), which read the report."""

    def __init__(self, report, indices, offsets, repaired, given_indices, given_offsets, row_counts, batch_size, num_hots,
                 nnz):
        self.report = report
        self.indices = indices
        self.offsets = offsets
        self.repaired = repaired
        # the values as they came in, where the call left them alone (None: repaired in place, or no offsets)
        self._given_indices = given_indices
        self._given_offsets = given_offsets
        self._row_counts = row_counts
        self._batch_size = batch_size
        self._num_hots = num_hots
        self._nnz = nnz

    def words(self):
        """The report on the host (synchronises): (bad_indices, first_bad_index, bad_offsets, first_bad_offset)."""
        return tuple(int(w) for w in self.report[:4].tolist())

    def _table_of_position(self, p):
        T, B = len(self._row_counts), self._batch_size
        if self._num_hots > 0:
            return int(p // (B * self._num_hots))
        if self.repaired:
            r = self.offsets.long()
        else:   # report only: the repaired offsets are the clamped running maximum of the given ones
            r = torch.cummax(self.offsets.long(), 0).values.clamp(0, self._nnz)
        cuts = (r[::B] if B > 0 else r[:1].expand(T + 1)).tolist()
        t = 0
        while t + 1 < T and cuts[t + 1] <= p:
            t += 1
        return t

    def raise_if_bad(self):
        """Reads the report (the one synchronisation) and raises IndexError when the batch has a bad index or offset: the
        counts, the first positions, the table and -- unless the input was repaired in place -- the offending values.
        Returns self otherwise."""
        bad_idx, first_idx, bad_off, first_off = self.words()
        if bad_idx == 0 and bad_off == 0:
            return self
        parts = []
        if bad_off:
            B, T = self._batch_size, len(self._row_counts)
            text = "%d bad offsets, first at position %d" % (bad_off, first_off)
            if B > 0:
                text += " (table %d)" % min(first_off // B, T - 1)
            if self._given_offsets is not None:
                text += ": offsets[%d] = %d" % (first_off, int(self._given_offsets[first_off]))
                if first_off > 0:
                    text += " after %d" % int(self._given_offsets[first_off - 1])
                text += ", nnz = %d" % self._nnz
            parts.append(text)
        if bad_idx:
            t = self._table_of_position(first_idx)
            text = "%d bad indices, first at position %d (table %d of %d rows)" % (bad_idx, first_idx, t,
                                                                                  self._row_counts[t])
            if self._given_indices is not None:
                text += ": indices[%d] = %d" % (first_idx, int(self._given_indices.reshape(-1)[first_idx]))
            parts.append(text)
        raise IndexError("cuembed_amd: the batch is not safe to look up: " + "; ".join(parts))


def new_index_report(device="cuda"):
    """The four int64 device words of a report (check_indices initialises them itself on every call)."""
    return torch.empty((4,), dtype=torch.int64, device=device)


def _same_or_apart(name, given, out):
    if out.data_ptr() == given.data_ptr():
        return
    a, b = given.data_ptr(), out.data_ptr()
    size = given.numel() * given.element_size()
    if not (a + size <= b or b + size <= a):
        raise ValueError("%s must be its input (in place) or not overlap it at all" % name)


def check_indices_workspace_bytes(num_tables, batch_size, num_hots=0, nnz=0):
    """Bytes of workspace one check_indices call of this shape needs (0 for fixed hotness): host arithmetic on the number
    of offsets; the lookup count `nnz` does not enter."""
    if not 1 <= num_tables <= MAX_CHECK_TABLES or batch_size < 0 or num_tables * batch_size > INT_MAX or num_hots < 0:
        raise ValueError("1 <= num_tables <= %d, batch_size >= 0, num_tables * batch_size must fit a 32-bit int and "
                         "num_hots >= 0" % MAX_CHECK_TABLES)
    if num_hots > 0:
        return 0
    # detail::PlanIndexCheck: tiles of whole 1,024-offset chunks, at most 1,024 of them; one word per tile for the maxima,
    # one for the tile ends, num_tables + 1 cuts; every region a multiple of 256 bytes (check_indices itself asks the
    # library, and tests/test_index_check_host.py pins these numbers against it)
    positions = num_tables * batch_size + 1
    chunks = -(-positions // SCAN_CHUNK)
    tile_len = -(-chunks // MAX_SCAN_TILES) * SCAN_CHUNK
    tiles = -(-positions // tile_len)

    def align(v):
        return -(-v // 256) * 256
    return 2 * align(tiles * 8) + align((num_tables + 1) * 8)


def check_indices(indices, offsets=None, *, num_rows=None, group=None, batch_size=None, num_hots=0, repair=False,
                  out_indices=None, out_offsets=None, report=None, workspace=None):
    """Checks one batch on the device, without a read-back (cuembed::CheckIndices; 3 launches for CSR, 2 for fixed
    hotness, capturable when report, workspace and -- with repair -- the outputs are given).

    indices: int32 / int64; CSR: offsets[num_tables * batch_size + 1] (int32 / int64); fixed hotness: offsets=None,
    num_hots=H, indices [num_tables, batch_size, H].  The rows: num_rows= (one table) or group= (a TableGroup, a
    MixedTableGroup or a list of same-width tables: group.row_base_device is what the kernel reads).  repair=True writes
    the repaired batch: into new tensors, or into out_indices / out_offsets, each of which may be its input (in place).  report: a 4-word int64
    device tensor to re-use (new_index_report()); workspace: a uint8 device tensor of at least
    check_indices_workspace_bytes(...) bytes, holding anything.  Returns an IndexCheck."""
    if not isinstance(indices, torch.Tensor):
        raise TypeError("indices must be a torch.Tensor")
    it = _index_code("indices", indices)
    if (num_rows is None) == (group is None):
        raise ValueError("exactly one of num_rows= (one table) and group= (a TableGroup) must be given")
    if group is not None:
        if not isinstance(group, MixedTableGroup):   # (a mixed-width group: only its row counts enter)
            group = _as_group(group)
        row_counts = group.row_counts
    else:
        if isinstance(num_rows, bool) or not isinstance(num_rows, int):
            raise TypeError("num_rows must be an int")
        row_counts = (num_rows,)
    T = len(row_counts)
    if T > MAX_CHECK_TABLES:
        raise ValueError("check_indices takes at most %d tables, got %d" % (MAX_CHECK_TABLES, T))
    for t, rows in enumerate(row_counts):
        if rows < 1:
            raise ValueError("table %d has %d rows: every checked table needs at least one row (the repaired id is 0)"
                             % (t, rows))
    batch_size, nnz, it, ot = group_batch_layout(T, indices, offsets, batch_size, num_hots)
    if offsets is not None and offsets.dtype == torch.int32 and nnz > INT_MAX:
        raise ValueError("int32 offsets cannot address %d lookups" % nnz)
    if nnz > MAX_CHECK_NNZ:
        raise ValueError("at most 2^38 lookups per call, got %d" % nnz)
    if not repair and (out_indices is not None or out_offsets is not None):
        raise ValueError("out_indices / out_offsets are written by repair=True only")
    if out_offsets is not None and offsets is None:
        raise ValueError("out_offsets: a fixed-hotness batch has no offsets")
    for name, out, given in (("out_indices", out_indices, indices), ("out_offsets", out_offsets, offsets)):
        if out is None:
            continue
        if not isinstance(out, torch.Tensor):
            raise TypeError("%s must be a torch.Tensor" % name)
        if out.dtype != given.dtype:
            raise TypeError("%s must have its input's dtype %s, got %s" % (name, given.dtype, out.dtype))
        if out.numel() != given.numel():
            raise ValueError("%s must have its input's %d entries, got %d" % (name, given.numel(), out.numel()))
        _same_or_apart(name, given, out)
    if report is not None:
        if not isinstance(report, torch.Tensor):
            raise TypeError("report must be a torch.Tensor")
        if report.dtype != torch.int64 or report.numel() < 4:
            raise ValueError("report must be an int64 tensor of 4 words (new_index_report())")
    # ---- the call is in order: now the devices
    _check_dev("indices", indices)
    dev = indices.device
    if group is not None and group.device != dev:
        raise RuntimeError("cuembed_amd: the group's tables are on %s, indices on %s" % (group.device, dev))
    if offsets is not None:
        _check_dev("offsets", offsets, dev)
    if out_indices is not None:
        _check_dev("out_indices", out_indices, dev)
    if out_offsets is not None:
        _check_dev("out_offsets", out_offsets, dev)
    if report is not None:
        _check_dev("report", report, dev)
    need = ctypes.c_size_t(0)
    L = _lib.lib()
    row_base = group.row_base_device if group is not None else None
    rows_arg = 0 if group is not None else int(num_rows)
    L.cuembed_check_indices(None, it, None, ot, nnz, _ptr(row_base), rows_arg, T, batch_size, num_hots, None, None, None,
                            None, ctypes.byref(need), None)
    if workspace is None:
        workspace = torch.empty((max(need.value, 8),), dtype=torch.uint8, device=dev)
    else:
        _check_dev("workspace", workspace, dev)
        if workspace.numel() * workspace.element_size() < need.value:
            raise ValueError("workspace too small: need %d bytes" % need.value)
        if workspace.numel() == 0:
            raise ValueError("workspace must hold at least one byte (the library runs only with a workspace pointer)")
        if workspace.data_ptr() % 8:
            raise ValueError("workspace must be 8-byte aligned")
    if report is None:
        report = new_index_report(dev)
    new_indices, new_offsets = indices, offsets
    if repair:
        new_indices = out_indices if out_indices is not None else torch.empty_like(indices)
        if offsets is not None:
            new_offsets = out_offsets if out_offsets is not None else torch.empty_like(offsets)
    lwork = ctypes.c_size_t(workspace.numel() * workspace.element_size())
    with torch.cuda.device(dev):
        L.cuembed_check_indices(_ptr(indices), it, _ptr(offsets), ot, nnz, _ptr(row_base), rows_arg, T, batch_size,
                                num_hots, _ptr(report), _ptr(new_indices) if repair else None,
                                _ptr(new_offsets) if repair and offsets is not None else None, _ptr(workspace),
                                ctypes.byref(lwork), _stream(indices))
    in_place_i = repair and new_indices.data_ptr() == indices.data_ptr()
    in_place_o = repair and offsets is not None and new_offsets.data_ptr() == offsets.data_ptr()
    return IndexCheck(report, new_indices, new_offsets, bool(repair), None if in_place_i else indices,
                      None if (in_place_o or offsets is None) else offsets, tuple(row_counts), batch_size, num_hots, nnz)
