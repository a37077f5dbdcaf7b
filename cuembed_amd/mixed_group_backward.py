"""The backward on a group of embedding tables of DIFFERENT widths: one sort and one scatter-add for all widths (an
extension).

The group of cuembed_amd.mixed_group -- T tables of any widths and one dtype, bag g = t * B + b, out [B, D], table t at
columns [c_t, c_t + W_t) -- is trained through the same-width group's pipeline (cuembed_amd.grouped_backward); only the
scatter-add is its own kernel, which finds the source slice and the active lanes per lookup:

    keys, sample ids        cuembed::GroupedBackwardKeys with group.row_base_device          (unchanged)
    transpose(..., num_categories=total_rows, remapped=True)                                 (unchanged)
    embedding_backward_mixed_group(group, grad_y, ...)   the three above and ONE mixed scatter-add
    MixedGroupedGrad        the compressed gradient: global ids, PADDED rows, the device-side count
    mixed_group_mean_scale  grad_y of a mean-pooled group -> grad_y of the sum-pooled one, ONE launch
    mixed_group_backward_launch_shape                    the scatter-add's launch shape (host arithmetic)

The gradient is padded to the widest table: rows is [capacity, W_max], entry k holds its row's gradient in
rows[k, :W_t] for the table t that ids[k] falls in.  COLUMNS >= W_t ARE UNSPECIFIED (untouched or zero): read an entry
through per_table(), which slices them off.  A ragged layout, the one-launch optimizer step, the weight gradient, dense
gradients, reference_sums, the sample-blocked order and pad_to_capacity do not exist for a mixed group (DESIGN.md
section 7).

Everything validates before any launch and runs on torch's current stream; nothing is read back, so after one warm call
(which builds the group's small device arrays) a call can be captured into a HIP graph.
"""
import ctypes

import torch

from . import _lib
from .group_layout import INT_MAX, check_weights, mean_scale_layout, mixed_lane_bytes
from .grouped_backward import GroupedGrad, _key_dtype, _layout
from .mixed_group import MixedTableGroup, _as_mixed_group
from .ops import MAX_LANES_PER_ROW, _ELEM, _INDEX, _check_dev, _overflow_word, _ptr, _stream, transpose


def _lane_bytes(group, *pointers):
    """The launch's lane (mixed_lane_bytes) for the (name, address) pairs given.  W_max is one of the widths."""
    return mixed_lane_bytes(group.widths, group.tables[0].element_size(), pointers)


def _check_limits(group, batch_size, lane):
    """The limits EmbeddingBackwardMixedGroup asserts, as ValueErrors."""
    size = group.tables[0].element_size()
    if max(group.widths) * size // lane > MAX_LANES_PER_ROW:
        raise ValueError("the widest table (%d elements) is more than %d lanes of %d bytes"
                         % (max(group.widths), MAX_LANES_PER_ROW, lane))
    if batch_size * (group.embedding_dim * size // lane) >= 2 ** 31:
        raise ValueError("batch_size * embedding_dim * itemsize / %d = %d: a staged lookup carries its source offset in "
                         "lanes of %d bytes in 31 bits" % (lane, batch_size * (group.embedding_dim * size // lane), lane))


def _check_grad_y(group, grad_y, batch_size, name="grad_y"):
    if not isinstance(grad_y, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor" % name)
    if grad_y.dtype != group.dtype:
        raise TypeError("%s must have the tables' dtype (%s), got %s" % (name, group.dtype, grad_y.dtype))
    want = (batch_size, group.embedding_dim)
    if tuple(grad_y.shape) != want:
        raise ValueError("%s must be [batch_size, embedding_dim] = %r, got %r" % (name, want, tuple(grad_y.shape)))
    if not grad_y.is_contiguous():
        raise ValueError("%s must be contiguous" % name)


def _group(group):
    group = _as_mixed_group(group)
    if not isinstance(group, MixedTableGroup):
        raise TypeError("group must be a MixedTableGroup or a list of tables")
    return group


class MixedGroupedGrad(GroupedGrad):
    """The compressed gradient of a mixed-width group, nothing read back:

        ids        ascending GLOBAL row ids (group.row_base[t] + the row of table t), `capacity` entries of room
        rows       [capacity, W_max]: rows[k, :W_t] is the gradient of ids[k], t the table the id falls in.  The columns
                   from W_t on are UNSPECIFIED (untouched or zero) and nothing in the library reads them
        last_id    one device word of ids' dtype: the entry count is last_id + 1
        row_base   group.row_base (host tuple);  widths  group.widths
        capacity   min(nnz, total_rows) unless the caller passed less

    Entries at and past the count hold nothing.  If the device-side count exceeded the capacity, nothing was written
    and capacity_overflowed() says so."""

    def __init__(self, ids, rows, last_id, row_base, row_base_device, widths):
        super().__init__(ids, rows, last_id, row_base, row_base_device)
        self.widths = tuple(widths)

    def per_table(self):
        """[(local_ids_t, rows_t)] for every table, with ONE read-back (the num_tables + 1 cuts): local_ids_t =
        ids[c0:c1] - row_base[t], the ascending rows of table t that were looked up; rows_t = rows[c0:c1, :W_t], a view
        (not contiguous where W_t < W_max)."""
        return [(ids, rows[:, :w]) for (ids, rows), w in zip(super().per_table(), self.widths)]

    def capacity_overflowed(self, reset=False):
        """True if a compressed backward on this gradient's device found more rows than its buffers hold since the last
        reset (cuembed_amd.capacity_overflowed: the device's sticky word; one 4-byte read-back)."""
        from .ops import capacity_overflowed
        return capacity_overflowed(self.ids.device, reset=reset)


def _mean_scale(group, grad_y, offsets, weights, batch_size, num_hots, out):
    """The launch of mixed_group_mean_scale, everything validated and on the device."""
    with torch.cuda.device(grad_y.device):
        _lib.lib().cuembed_mixed_group_mean_scale(
            _ptr(grad_y), _ELEM[grad_y.dtype], group._widths_array, _ptr(group.table_columns_device), _ptr(offsets),
            0 if offsets is None else _INDEX[offsets.dtype], _ptr(weights), group.num_tables, int(batch_size),
            int(num_hots), _ptr(out), _stream(grad_y))
    return out


def mixed_group_mean_scale(group, grad_y, offsets=None, weights=None, num_hots=0, out=None):
    """grad_y [batch_size, D] of a MEAN-pooled mixed group times each bag's mean factor -- the grad_y of the equivalent
    sum-pooled group -- in ONE launch (cuembed::MixedGroupMeanScale): out[b, c_t + j] = grad_y[b, c_t + j] * f with one
    fp32 multiply and one rounding per element, f the forward's own factor of bag t * batch_size + b: 1 / its length,
    or with `weights` (one per lookup, the tables' dtype) 1 / the fp32 sum of its weights; 0 when that is 0.  The bits
    of num_tables grouped_mean_scale calls on one-table groups, concatenated on dim 1.  CSR (offsets[num_tables *
    batch_size + 1]) or fixed hotness (offsets=None, num_hots=H).  out: a contiguous tensor of grad_y's shape and dtype,
    which may be grad_y itself (in place); None allocates one."""
    group = _group(group)
    if not isinstance(grad_y, torch.Tensor) or grad_y.dim() != 2:
        raise ValueError("grad_y must be a [batch_size, embedding_dim] torch.Tensor")
    batch_size = grad_y.shape[0]
    _check_grad_y(group, grad_y, batch_size)
    T = group.num_tables
    mean_scale_layout(T, offsets, batch_size, num_hots)
    if weights is not None:
        check_weights(group.dtype, weights, 0 if offsets is not None else T * batch_size * num_hots)
    if out is not None:
        _check_grad_y(group, out, batch_size, name="out")
    # ---- the call is in order: now the devices
    _check_dev("grad_y", grad_y)
    dev = grad_y.device
    if offsets is not None:
        _check_dev("offsets", offsets, dev)
    if weights is not None:
        _check_dev("weights", weights, dev)
    if out is None:
        out = torch.empty_like(grad_y)
    else:
        _check_dev("out", out, dev)
    if grad_y.numel() == 0:
        return out
    _lane_bytes(group, ("grad_y", grad_y.data_ptr()), ("out", out.data_ptr()))
    return _mean_scale(group, grad_y, offsets, weights, batch_size, num_hots, out)


def embedding_backward_mixed_group(group, grad_y, indices, offsets=None, weights=None, batch_size=None, num_hots=0,
                                   mode="sum", capacity=None):
    """The gradient of ALL tables of a MixedTableGroup from grad_y [batch_size, D] (contiguous, the tables' dtype), the
    gradient of embedding_forward_mixed_group(mode=mode)'s result: one key launch (cuembed::GroupedBackwardKeys), ONE
    transpose bounded by total_rows with the remap, ONE scatter-add for all widths (cuembed::EmbeddingBackwardMixedGroup).
    indices / offsets / weights / num_hots as in the forward.  mode="mean": one launch in front (mixed_group_mean_scale)
    multiplies grad_y, into a new buffer, by each bag's mean factor.

    Returns a MixedGroupedGrad: ascending global ids, rows PADDED to the widest table and the device-side count, in
    buffers of `capacity` entries -- min(nnz, total_rows) by default, always enough; a caller who knows better may pass
    less, and if the device-side count exceeds it nothing is written and the overflow word is raised
    (capacity_overflowed()).  Arithmetic: embedding_backward's default (fp32 partial sums, one rounding per flush); on
    exactly representable data the bits of num_tables single-table compressed backwards.  set_backward_tuning applies.
    No read-back."""
    group = _group(group)
    batch_size, nnz = _layout(group, indices, offsets, batch_size, num_hots)
    _check_grad_y(group, grad_y, batch_size)
    if mode not in ("sum", "mean"):
        raise ValueError("mode must be 'sum' or 'mean', got %r: the grouped backward has no other pooling" % (mode,))
    if weights is not None:
        check_weights(group.dtype, weights, nnz)
    total = group.total_rows
    if capacity is None:
        capacity = min(nnz, total)
    elif isinstance(capacity, bool) or not isinstance(capacity, int) or capacity < 0:
        raise ValueError("capacity must be a non-negative int or None, got %r" % (capacity,))
    _check_limits(group, batch_size, _lane_bytes(group))
    # ---- the call is in order: now the devices
    dev = group.device
    _check_dev("tables[0]", group.tables[0])
    _check_dev("grad_y", grad_y, dev)
    _check_dev("indices", indices, dev)
    if offsets is not None:
        _check_dev("offsets", offsets, dev)
    if weights is not None:
        _check_dev("weights", weights, dev)
        weights = weights.reshape(-1)[:nnz]
    kd = _key_dtype(group)
    w_max = max(group.widths)
    rows = torch.empty((capacity, w_max), dtype=group.dtype, device=dev)
    ids = torch.empty((capacity,), dtype=kd, device=dev)
    if nnz == 0:
        return MixedGroupedGrad(ids, rows, torch.full((1,), -1, dtype=kd, device=dev), group.row_base,
                                group.row_base_device, group.widths)
    if mode == "mean":
        scaled = torch.empty_like(grad_y)
        _lane_bytes(group, ("grad_y", grad_y.data_ptr()), ("grad_y", scaled.data_ptr()))
        grad_y = _mean_scale(group, grad_y, offsets, weights, batch_size, num_hots, scaled)
    lane = _lane_bytes(group, ("grad_y", grad_y.data_ptr()), ("rows", rows.data_ptr()))
    _check_limits(group, batch_size, lane)
    keys = torch.empty((nnz,), dtype=kd, device=dev)
    sample_ids = torch.empty((nnz,), dtype=kd, device=dev)
    L = _lib.lib()
    with torch.cuda.device(dev):   # the launches must happen on the tensors' device
        L.cuembed_grouped_backward_keys(
            _ptr(indices), _INDEX[indices.dtype], _ptr(offsets), 0 if offsets is None else _INDEX[offsets.dtype],
            _ptr(group.row_base_device), group.num_tables, int(batch_size), int(num_hots), nnz, _ptr(keys),
            _ptr(sample_ids), _INDEX[kd], _stream(indices))
    t_keys, t_sids, t_w, remap = transpose(sample_ids, keys, weights, num_categories=total, remapped=True)
    if capacity > 0:
        with torch.cuda.device(dev):
            L.cuembed_embedding_backward_mixed_group(
                _ptr(grad_y), _ELEM[group.dtype], group._widths_array, _ptr(group.table_columns_device), group.num_tables,
                int(batch_size), nnz, _ptr(t_keys), _ptr(t_sids), _ptr(remap), _INDEX[kd], _ptr(t_w), _ptr(rows),
                _ptr(ids), int(capacity), _ptr(_overflow_word(dev)), _stream(grad_y))
    else:   # no room at all and lookups to scatter: the overflow, without a launch that could not even be told so
        _overflow_word(dev).fill_(1)
    return MixedGroupedGrad(ids, rows, remap[-1:], group.row_base, group.row_base_device, group.widths)


def mixed_group_backward_launch_shape(elem_dtype, widths, nnz, is_weighted=False, pointer_bits=0, compute_units=0,
                                      xcds=0):
    """Launch shape of the mixed-width scatter-add (pure host arithmetic when compute_units > 0 describes the device; 0 =
    ask the current device): backward_launch_shape's plan at W_max = max(widths), so set_backward_tuning applies, with
    the lane width of the whole group.  pointer_bits: grad_y and the gradient rows OR-ed (0 = aligned buffers)."""
    if elem_dtype not in _ELEM:
        raise TypeError("elem_dtype must be float32, float16 or bfloat16, got %s" % elem_dtype)
    widths = [int(w) for w in widths]
    T = len(widths)
    if T < 1 or any(w <= 0 or (w * elem_dtype.itemsize) % 4 for w in widths) or sum(widths) > INT_MAX:
        raise ValueError("at least one table, every row size a multiple of 4 bytes, the widths summing to at most 2^31 - 1")
    if nnz < 0 or nnz > INT_MAX:
        raise ValueError("nnz must be in [0, 2^31 - 1]")
    if pointer_bits % 4:
        raise ValueError("every pointer must be 4-byte aligned")
    lane = mixed_lane_bytes(widths, elem_dtype.itemsize, (("pointer_bits", pointer_bits),))
    if max(widths) * elem_dtype.itemsize // lane > MAX_LANES_PER_ROW:
        raise ValueError("the widest table is more than %d lanes of %d bytes" % (MAX_LANES_PER_ROW, lane))
    out = (ctypes.c_int * 10)()
    _lib.lib().cuembed_mixed_group_backward_launch_shape((ctypes.c_int * T)(*widths), T, _ELEM[elem_dtype], int(nnz),
                                                         int(bool(is_weighted)), int(pointer_bits), int(compute_units),
                                                         int(xcds), out)
    return dict(elems_per_lane=out[0], lanes=out[1], segments_per_block=out[2], segment_len=out[3], column_slices=out[4],
                grid=out[5], lds_bytes=out[6], lookups_per_block=out[7], max_width=out[8], embedding_dim=out[9])
