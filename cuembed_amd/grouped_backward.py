"""The backward on a GROUP of embedding tables: one sort and one scatter-add for all tables (an extension).

The group of cuembed_amd.grouped -- T tables of one width and dtype, bag g = t * B + b, out [B, T, W] -- is trained
through the single-table pipeline, fed the right keys:

    keys[p]       = row_base[t] + indices[p]     a row of the tables laid end to end (row_base: group.row_base)
    sample_ids[p] = b * T + t                    the lookup's row in out[B, T, W] viewed as [B * T, W]

    grouped_backward_keys(group, ...)            both arrays in ONE launch (cuembed::GroupedBackwardKeys)
    embedding_backward_grouped(group, grad_y, ...)   keys -> transpose -> remap -> embedding_backward: the gradient of
                                                 all tables, dense ([total_rows, W] + per-table views) or compressed
    GroupedGrad                                  the compressed gradient: global ids, rows, the device-side count
    grouped_table_cuts(ids, row_base, ...)       where each table's entries begin (cuembed::GroupedTableCuts)

The gradient comes out sorted by table, then by row.  For a ONE-STORAGE group (TableGroup.allocate / from_flat) the
global ids are directly rows of group.flat, so the sparse optimizers apply as they are, with no read-back:

    g = embedding_backward_grouped(group, grad_y, idx, offsets)
    sparse_row_update(group.flat, g.ids, g.rows, rule="sgd", lr=lr, last_id=g.last_id)      # or sparse_row_adam, or a
                                                                                            # cuembed_amd.optim updater
For a group of SEPARATE tensors (one parameter per table, as most models hold them) the same gradient is applied in ONE
launch by the grouped step, which finds each entry's table on the device -- no cuts, no read-back, capturable:

    sparse_row_update_grouped(group, g.ids, g.rows, rule="sgd", lr=lr, last_id=g.last_id)   # or sparse_row_adam_grouped, or
                                                                                            # cuembed_amd.optim.GroupSparseUpdater
(fp16 / bf16 tables: stochastic_rounding=True, seeds=[one per table], step=...)
The sort is stable, so inside one table row the lookups keep the order of the single-table pipeline: on exactly
representable data, and with reference_sums=True on any data, the result has the bits of T single-table calls.  With
the default arithmetic the segment cuts of the scatter-add move with the position in the combined stream: the same
sums, associated differently.

Everything validates before any launch and runs on torch's current stream.  The fixed-hotness path materialises the
sample ids, which transpose_fixed_hotness avoids for one table.
"""
import ctypes

import torch

from . import _lib
from .group_layout import INT_MAX, check_weights, group_batch_layout, mean_scale_layout
from .grouped import _as_group
from .ops import (ADAM_RULES, UPDATE_RULES, _ELEM, _INDEX, _check_alignment, _check_betas, _check_dev, _entry_counts,
                  _index_code, _ptr, _stream, embedding_backward, transpose)


def _layout(group, indices, offsets, batch_size, num_hots):
    """The bag layout of one grouped call, validated without the GPU: (batch_size, nnz)."""
    return group_batch_layout(group.num_tables, indices, offsets, batch_size, num_hots, max_nnz=INT_MAX)[:2]


def _float_group(group):
    group = _as_group(group)
    if group.quantized:
        raise TypeError("a group of fused 8-bit tables has no backward: quantized tables are inference only")
    return group


def _key_dtype(group, key_dtype=None):
    total = group.total_rows
    if key_dtype is None:
        return torch.int32 if total < 2 ** 31 else torch.int64
    if key_dtype not in _INDEX:
        raise TypeError("key_dtype must be int32 or int64, got %s" % (key_dtype,))
    if key_dtype == torch.int32 and total >= 2 ** 31:
        raise ValueError("int32 keys need fewer than 2^31 rows in the group, it has %d" % total)
    return key_dtype


def grouped_backward_keys(group, indices, offsets=None, batch_size=None, num_hots=0, key_dtype=None, out=None):
    """(keys, sample_ids) of a group's lookups in ONE launch: for lookup p of bag t * batch_size + b,
    keys[p] = group.row_base[t] + indices[p] and sample_ids[p] = b * num_tables + t.  CSR (offsets[num_tables *
    batch_size + 1]) or fixed hotness (offsets=None, num_hots=H, indices [num_tables, batch_size, H]), int32 or int64
    indices and offsets in any combination.  key_dtype: the dtype of both results, the index type of the backward
    pipeline; None = int32 whenever the group has fewer than 2^31 rows (whatever the indices' dtype: the arrays are
    written fresh, so narrowing is free), else int64; int32 with 2^31 rows or more is a ValueError.  out: optional
    (keys, sample_ids) buffers of nnz entries.  Ids outside [0, rows_t) are a contract violation, as in the forward
    (cuembed_amd.check_indices finds and repairs them on the device)."""
    group = _float_group(group)
    batch_size, nnz = _layout(group, indices, offsets, batch_size, num_hots)
    kd = _key_dtype(group, key_dtype)
    if out is not None:
        if not (isinstance(out, (tuple, list)) and len(out) == 2 and all(isinstance(o, torch.Tensor) for o in out)):
            raise TypeError("out must be a (keys, sample_ids) pair of tensors")
        for name, o in zip(("out[0]", "out[1]"), out):
            if o.dtype != kd or o.numel() != nnz:
                raise ValueError("%s must hold %d entries of %s" % (name, nnz, kd))
    # ---- the call is in order: now the devices
    dev = group.device
    _check_dev("tables[0]", group.tables[0])
    _check_dev("indices", indices, dev)
    if offsets is not None:
        _check_dev("offsets", offsets, dev)
    if out is None:
        keys = torch.empty((nnz,), dtype=kd, device=dev)
        sample_ids = torch.empty((nnz,), dtype=kd, device=dev)
    else:
        keys, sample_ids = out
        _check_dev("out[0]", keys, dev)
        _check_dev("out[1]", sample_ids, dev)
    if nnz > 0:
        with torch.cuda.device(dev):   # the launch must happen on the tensors' device
            _lib.lib().cuembed_grouped_backward_keys(
                _ptr(indices), _INDEX[indices.dtype], _ptr(offsets), 0 if offsets is None else _INDEX[offsets.dtype],
                _ptr(group.row_base_device), group.num_tables, int(batch_size), int(num_hots), nnz, _ptr(keys),
                _ptr(sample_ids), _INDEX[kd], _stream(indices))
    return keys, sample_ids


def grouped_table_cuts(ids, row_base, count=None, last_id=None):
    """cuts[t] = the number of valid entries of the ascending global ids `ids` that are < row_base[t]: an int64 device
    tensor of num_tables + 1 entries, cuts[0] = 0, cuts[-1] = the count; table t owns the entries [cuts[t], cuts[t + 1]).
    row_base: the int64 device tensor group.row_base_device.  The count, as sparse_row_update takes it: count=int (None:
    all entries), count=tensor (one int32 / int64 device word) or last_id=tensor (one word of ids' dtype, count =
    last_id + 1).  A count below zero or above ids.numel() gives all-zero cuts.  No read-back."""
    if not isinstance(ids, torch.Tensor) or not isinstance(row_base, torch.Tensor):
        raise TypeError("ids and row_base must be torch.Tensors")
    it = _index_code("ids", ids)
    if row_base.dtype != torch.int64 or row_base.dim() != 1 or row_base.numel() < 2:
        raise TypeError("row_base must be the int64 tensor of num_tables + 1 entries (group.row_base_device)")
    if count is not None and last_id is not None:
        raise ValueError("give at most one of count= and last_id=")
    n = ids.numel()
    host_count, word, word64 = n, None, False
    if isinstance(count, torch.Tensor):
        if count.dtype not in _INDEX or count.numel() != 1:
            raise TypeError("count must be an int or a one-element int32 / int64 tensor")
        word, word64 = count, count.dtype == torch.int64
    elif count is not None:
        host_count = int(count)
        if host_count < 0 or host_count > n:
            raise ValueError("count must be in [0, ids.numel()]")
    if last_id is not None and (not isinstance(last_id, torch.Tensor) or last_id.dtype != ids.dtype or
                                last_id.numel() != 1):
        raise TypeError("last_id must be a one-element tensor of ids' dtype")
    _check_dev("ids", ids)
    dev = ids.device
    _check_dev("row_base", row_base, dev)
    for name, t in (("count", word), ("last_id", last_id)):
        if t is not None:
            _check_dev(name, t, dev)
    cuts = torch.empty((row_base.numel(),), dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        _lib.lib().cuembed_grouped_table_cuts(_ptr(ids), it, n, host_count, _ptr(word), int(word64), _ptr(last_id),
                                              _ptr(row_base), row_base.numel() - 1, _ptr(cuts), _stream(ids))
    return cuts


class GroupedGrad:
    """The compressed gradient of a group, nothing read back:

        ids        ascending GLOBAL row ids (group.row_base[t] + the row of table t), `capacity` entries of room
        rows       [capacity, width] gradient rows, rows[k] belongs to ids[k]
        last_id    one device word of ids' dtype: the entry count is last_id + 1 (sparse_row_update's last_id=)
        row_base   group.row_base (host tuple)
        capacity   min(nnz, total_rows): always enough for a fully sorted order

    Entries at and past the count hold nothing.  For a one-storage group (ids, rows, last_id) is a gradient of
    group.flat as the sparse optimizers take it."""

    def __init__(self, ids, rows, last_id, row_base, row_base_device):
        self.ids = ids
        self.rows = rows
        self.last_id = last_id
        self.row_base = tuple(row_base)
        self.row_base_device = row_base_device
        self.capacity = ids.numel()

    def table_cuts(self):
        """The int64 device tensor of num_tables + 1 cuts (grouped_table_cuts): table t owns [cuts[t], cuts[t + 1])."""
        return grouped_table_cuts(self.ids, self.row_base_device, last_id=self.last_id)

    def per_table(self):
        """[(local_ids_t, rows_t)] for every table, with ONE read-back (the num_tables + 1 cuts): local_ids_t =
        ids[cut_t:cut_t+1] - row_base[t], the ascending rows of table t that were looked up; rows_t is a view."""
        cuts = self.table_cuts().tolist()
        return [(self.ids[cuts[t]:cuts[t + 1]] - self.row_base[t], self.rows[cuts[t]:cuts[t + 1]])
                for t in range(len(self.row_base) - 1)]


def _check_grad_y(group, grad_y, batch_size):
    if not isinstance(grad_y, torch.Tensor):
        raise TypeError("grad_y must be a torch.Tensor")
    if grad_y.dtype != group.dtype:
        raise TypeError("grad_y must have the tables' dtype (%s), got %s" % (group.dtype, grad_y.dtype))
    want = (batch_size, group.num_tables, group.width)
    if tuple(grad_y.shape) != want:
        raise ValueError("grad_y must be [batch_size, num_tables, width] = %r, got %r" % (want, tuple(grad_y.shape)))
    if not grad_y.is_contiguous():
        raise ValueError("grad_y must be contiguous")


def _mean_scale(group, grad_y, offsets, weights, batch_size, num_hots, out):
    """The launch of grouped_mean_scale, everything validated and on the device."""
    with torch.cuda.device(grad_y.device):
        _lib.lib().cuembed_grouped_mean_scale(
            _ptr(grad_y), _ELEM[grad_y.dtype], group.width, _ptr(offsets),
            0 if offsets is None else _INDEX[offsets.dtype], _ptr(weights), group.num_tables, int(batch_size),
            int(num_hots), _ptr(out), _stream(grad_y))
    return out


def grouped_mean_scale(group, grad_y, offsets=None, weights=None, num_hots=0, out=None):
    """grad_y [batch_size, num_tables, width] of a MEAN-pooled group times each bag's mean factor -- the grad_y of the
    equivalent sum-pooled group -- in ONE launch (cuembed::GroupedMeanScale): out[b, t, :] = grad_y[b, t, :] * f with one
    fp32 multiply and one rounding per element, f the forward's own factor of bag t * batch_size + b: 1 / its length,
    or with `weights` (one per lookup, the tables' dtype) 1 / the fp32 sum of its weights; 0 when that is 0.  CSR
    (offsets[num_tables * batch_size + 1]) or fixed hotness (offsets=None, num_hots=H).  out: a contiguous tensor of
    grad_y's shape and dtype, which may be grad_y itself (in place); None allocates one."""
    group = _float_group(group)
    if not isinstance(grad_y, torch.Tensor) or grad_y.dim() != 3:
        raise ValueError("grad_y must be a [batch_size, num_tables, width] torch.Tensor")
    batch_size = grad_y.shape[0]
    _check_grad_y(group, grad_y, batch_size)
    T = group.num_tables
    mean_scale_layout(T, offsets, batch_size, num_hots)
    if weights is not None:
        check_weights(group.dtype, weights, 0 if offsets is not None else T * batch_size * num_hots)
    if out is not None:
        if not isinstance(out, torch.Tensor):
            raise TypeError("out must be a torch.Tensor")
        if out.dtype != grad_y.dtype or tuple(out.shape) != tuple(grad_y.shape) or not out.is_contiguous():
            raise ValueError("out must be a contiguous tensor of grad_y's shape and dtype")
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
    _check_alignment("grad_y", grad_y.data_ptr(), grad_y.element_size(), group.width, others=(("out", out.data_ptr()),))
    return _mean_scale(group, grad_y, offsets, weights, batch_size, num_hots, out)


def embedding_weight_grad_grouped(group, grad_y, indices, offsets=None, batch_size=None, num_hots=0, out=None):
    """The gradient of a weighted SUM-forward of a group with respect to the per-lookup weights, in ONE launch
    (cuembed::EmbeddingWeightGradGrouped): for lookup p of bag t * batch_size + b, grad_w[p] = <tables[t][indices[p], :],
    grad_y[b, t, :]> in fp32, rounded once to the tables' dtype -- the bits of num_tables calls of embedding_weight_grad
    on grad_y[:, t, :].contiguous().  grad_y [batch_size, num_tables, width], contiguous, the tables' dtype; indices /
    offsets / num_hots as in the forward.  Returns a tensor of indices' shape; out: an optional contiguous buffer of
    indices.numel() entries of the tables' dtype.  It reads every looked-up row once more."""
    group = _float_group(group)
    batch_size, nnz = _layout(group, indices, offsets, batch_size, num_hots)
    _check_grad_y(group, grad_y, batch_size)
    if out is not None:
        if not isinstance(out, torch.Tensor):
            raise TypeError("out must be a torch.Tensor")
        if out.dtype != group.dtype or out.numel() != nnz or not out.is_contiguous():
            raise ValueError("out must be a contiguous tensor of %d entries of %s" % (nnz, group.dtype))
    # ---- the call is in order: now the devices
    dev = group.device
    _check_dev("tables[0]", group.tables[0])
    _check_dev("grad_y", grad_y, dev)
    _check_dev("indices", indices, dev)
    if offsets is not None:
        _check_dev("offsets", offsets, dev)
    if out is None:
        out = torch.empty(indices.shape, dtype=group.dtype, device=dev)
    else:
        _check_dev("out", out, dev)
    group.lane_bytes(grad_y.data_ptr())
    if nnz > 0:
        with torch.cuda.device(dev):
            _lib.lib().cuembed_embedding_weight_grad_grouped(
                group._host_array, _ptr(group.table_ptrs), group.num_tables, _ELEM[group.dtype], group.width,
                _ptr(indices), _INDEX[indices.dtype], _ptr(offsets), 0 if offsets is None else _INDEX[offsets.dtype],
                _ptr(grad_y), int(batch_size), int(num_hots), _ptr(out), _stream(indices))
    return out


def embedding_backward_grouped(group, grad_y, indices, offsets=None, weights=None, batch_size=None, num_hots=0,
                               dense=False, reference_sums=False, mode="sum"):
    """The gradient of ALL tables of a group from grad_y [batch_size, num_tables, width] (contiguous, the tables' dtype),
    the gradient of embedding_forward_grouped(mode=mode)'s result: grouped_backward_keys, ONE transpose (bounded by
    total_rows, so the sort skips the zero digits) with the remap, ONE embedding_backward on grad_y viewed as
    [batch_size * num_tables, width].  indices / offsets / weights / num_hots as in the forward.  (The remap is the
    transpose's own fourth result, compute_compressed_grad_indices' values from the same call: up to 4,096 lookups the
    whole index work after the keys is then one launch.)

    mode="sum"    the pipeline above, as it is.
    mode="mean"   one launch in front of it (grouped_mean_scale) multiplies grad_y, into a new buffer, by each bag's mean
                  factor; the pipeline then runs unchanged on that.

    dense=True    returns (grad, views): ONE zero-initialised [total_rows, width] buffer and its per-table row slices
                  views[t] = grad[row_base[t]:row_base[t + 1]].  reference_sums=True (dense only: it needs a host-known
                  row count) sums in the gradient's own type in lookup order, like the CPU reference.
    dense=False   returns a GroupedGrad: global ids, rows and the device-side count in buffers of min(nnz, total_rows)
                  entries; the scatter-add runs with num_grad_embedding_rows=None, so its capacity check and the
                  overflow word (capacity_overflowed()) apply.  No read-back."""
    group = _float_group(group)
    batch_size, nnz = _layout(group, indices, offsets, batch_size, num_hots)
    _check_grad_y(group, grad_y, batch_size)
    if mode not in ("sum", "mean"):
        raise ValueError("mode must be 'sum' or 'mean', got %r: the grouped backward has no other pooling" % (mode,))
    if reference_sums and not dense:
        raise ValueError("reference_sums needs a host-known row count: dense=True only")
    if weights is not None:
        check_weights(group.dtype, weights, nnz)
    # ---- the call is in order: now the devices
    dev = group.device
    _check_dev("tables[0]", group.tables[0])
    _check_dev("grad_y", grad_y, dev)
    if weights is not None:
        _check_dev("weights", weights, dev)
        weights = weights.reshape(-1)[:nnz]
    total, width = group.total_rows, group.width
    if mode == "mean" and nnz > 0:
        if offsets is not None:
            _check_dev("offsets", offsets, dev)
        _check_alignment("grad_y", grad_y.data_ptr(), grad_y.element_size(), width)
        grad_y = _mean_scale(group, grad_y, offsets, weights, batch_size, num_hots, torch.empty_like(grad_y))
    grad_2d = grad_y.view(batch_size * group.num_tables, width)
    keys, sample_ids = grouped_backward_keys(group, indices, offsets, batch_size, num_hots)
    if dense:
        grad = torch.zeros((total, width), dtype=group.dtype, device=dev)
        if nnz > 0:
            t_keys, t_sids, t_w = transpose(sample_ids, keys, weights, num_categories=total)
            embedding_backward(grad_2d, total, t_keys, t_sids, None, t_w, skip_grad_init=True, grad_embedding=grad,
                               reference_sums=reference_sums)
        base = group.row_base
        return grad, tuple(grad[base[t]:base[t + 1]] for t in range(group.num_tables))
    capacity = min(nnz, total)
    rows = torch.empty((capacity, width), dtype=group.dtype, device=dev)
    ids = torch.empty((capacity,), dtype=keys.dtype, device=dev)
    if capacity == 0:
        last_id = torch.full((1,), -1, dtype=keys.dtype, device=dev)
    else:
        t_keys, t_sids, t_w, remap = transpose(sample_ids, keys, weights, num_categories=total, remapped=True)
        embedding_backward(grad_2d, None, t_keys, t_sids, remap, t_w, grad_embedding=rows, inverse_mapping=ids)
        last_id = remap[-1:]
    return GroupedGrad(ids, rows, last_id, group.row_base, group.row_base_device)


# ---- the optimizer step on a group of separate tensors (cuembed::SparseRowUpdateGrouped / SparseRowAdamGrouped) ------
MAX_GROUPED_STEP_TABLES = 1023   # detail::kGroupedMaxTables: row_base and the base pointers are staged in 32 KiB of LDS


def _check_seeds(group, stochastic_rounding, seeds):
    """The rounding of a grouped step, validated without the GPU: None (to nearest) or the tables' seeds, as a tuple of
    ints (or as the int64 device tensor [num_tables] of their bits, if that is what was passed).
    There are no default seeds: one seed for the group would give row r of every table the same bits."""
    if stochastic_rounding and seeds is None:
        raise ValueError("stochastic rounding on a grouped step takes one seed per table: pass seeds=[...]")
    if seeds is None:
        return None
    if not stochastic_rounding:
        raise ValueError("seeds go with stochastic_rounding=True: a step that rounds to nearest draws no bits")
    if isinstance(seeds, torch.Tensor):
        # the seeds as they live on the device (what the torch op is handed): int64 [num_tables] holding their bits
        if seeds.dtype != torch.int64 or seeds.dim() != 1 or not seeds.is_contiguous():
            raise TypeError("seeds as a tensor must be a contiguous int64 tensor [num_tables] that holds the seeds' bits")
        if seeds.numel() != group.num_tables:
            raise ValueError("seeds must hold one seed per table: the group has %d tables, got %d"
                             % (group.num_tables, seeds.numel()))
        if group.dtype == torch.float32:
            raise TypeError("stochastic_rounding is for float16 / bfloat16 tables: a float32 table is not rounded")
        return seeds
    if not isinstance(seeds, (list, tuple)):
        raise TypeError("seeds must be a sequence of %d ints, one per table" % group.num_tables)
    if len(seeds) != group.num_tables:
        raise ValueError("seeds must hold one seed per table: the group has %d tables, got %d"
                         % (group.num_tables, len(seeds)))
    for t, seed in enumerate(seeds):
        if isinstance(seed, bool) or not isinstance(seed, int):
            raise TypeError("seeds[%d] must be an int in [0, 2**64), got %r" % (t, seed))
        if not 0 <= seed < 2 ** 64:
            raise ValueError("seeds[%d] must be an int in [0, 2**64), got %r" % (t, seed))
    if group.dtype == torch.float32:
        raise TypeError("stochastic_rounding is for float16 / bfloat16 tables: a float32 table is not rounded")
    return tuple(seeds)


def _seeds_tensor(group, seeds):
    """The seeds on the device, as the int64 [num_tables] tensor that holds their bits.  Built ONCE per tuple of seeds and
    kept on the group, next to the state pointer arrays: a step copies nothing, so it can run under capture."""
    if isinstance(seeds, torch.Tensor):
        return seeds
    cache = group._seed_arrays
    hit = cache.get(seeds)
    if hit is None:
        if len(cache) >= 16:    # (seeds that came and went)
            cache.clear()
        hit = cache[seeds] = torch.tensor([s - 2 ** 64 if s >= 2 ** 63 else s for s in seeds], dtype=torch.int64,
                                        device=group.device)
    return hit


def _check_step(seeds, step):
    """The step of a stochastic grouped step, validated: (step, step word).  Not read without seeds."""
    if seeds is None:
        return 0, None
    if isinstance(step, torch.Tensor):
        if step.dtype != torch.int64 or step.numel() != 1:
            raise TypeError("a device-side step must be a one-element int64 tensor")
        return 0, step
    if isinstance(step, bool) or not isinstance(step, int) or not 0 <= step < 2 ** 64:
        raise ValueError("step must be an int in [0, 2**64) or a one-element int64 device tensor, got %r" % (step,))
    return step, None


def _step_group(group, ids, rows, stochastic_rounding, seeds=None):
    """What both grouped steps check first, without the GPU: the group, the rounding, ids and rows.  Returns (group, index
    code, n, seeds)."""
    group = _as_group(group)
    if group.quantized:
        raise TypeError("a group of fused 8-bit tables has no optimizer step: quantized tables are inference only")
    seeds = _check_seeds(group, stochastic_rounding, seeds)
    if group.num_tables > MAX_GROUPED_STEP_TABLES:
        raise ValueError("a grouped step takes at most %d tables, the group has %d"
                         % (MAX_GROUPED_STEP_TABLES, group.num_tables))
    for name, t in (("ids", ids), ("rows", rows)):
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s must be a torch.Tensor" % name)
    it = _index_code("ids", ids)
    if rows.dtype != group.dtype:
        raise TypeError("rows must have the tables' dtype (%s), got %s" % (group.dtype, rows.dtype))
    if rows.dim() != 2 or rows.shape[1] != group.width:
        raise ValueError("rows must be [entries, width = %d], got %r" % (group.width, tuple(rows.shape)))
    if (group.width * rows.element_size()) % 4 != 0:
        raise ValueError("the row size must be a multiple of 4 bytes")
    if ids.dim() != 1 or rows.shape[0] != ids.numel():
        raise ValueError("ids must hold one entry per row of rows: %d ids, %d rows" % (ids.numel(), rows.shape[0]))
    return group, it, ids.numel(), seeds


def _check_group_states(group, name, states, rowwise):
    """`states`: a sequence of num_tables float32 tensors, [rows_t, width] or (rowwise) [rows_t]."""
    if isinstance(states, torch.Tensor) or not isinstance(states, (list, tuple)):
        raise TypeError("%s must be a sequence of %d float32 tensors, one per table" % (name, group.num_tables))
    if len(states) != group.num_tables:
        raise ValueError("%s must hold one tensor per table: the group has %d tables, got %d"
                         % (name, group.num_tables, len(states)))
    for t, (s, n) in enumerate(zip(states, group.row_counts)):
        want = (n,) if rowwise else (n, group.width)
        if not isinstance(s, torch.Tensor):
            raise TypeError("%s[%d] must be a float32 tensor of shape %r" % (name, t, want))
        if s.dtype != torch.float32:
            raise TypeError("%s[%d] must be float32, got %s" % (name, t, s.dtype))
        if tuple(s.shape) != want:
            raise ValueError("%s[%d] must have shape %r, got %r" % (name, t, want, tuple(s.shape)))
    return tuple(states)


def _state_ptrs(group, states):
    """(host array, device tensor, OR of the pointers) of the base pointers of one state tensor per table.  The device
    tensor is built ONCE per set of tensors and kept on the group, next to table_ptrs: a step copies nothing."""
    ptrs = tuple(int(s.data_ptr()) for s in states)
    cache = group._state_ptr_arrays
    hit = cache.get(ptrs)
    if hit is None:
        if len(cache) >= 16:    # (state tensors that came and went)
            cache.clear()
        bits = 0
        for p in ptrs:
            bits |= p
        hit = cache[ptrs] = ((ctypes.c_void_p * len(ptrs))(*ptrs),
                             torch.tensor(ptrs, dtype=torch.int64, device=group.device), bits)
    return hit


def _word(name, value, dtype):
    """A hyper-parameter as (float, device word): one-element tensors are read by the kernel."""
    if isinstance(value, torch.Tensor):
        if value.dtype != dtype or value.numel() != 1:
            raise TypeError("a device-side %s must be a one-element %s tensor" % (name, dtype))
        return 0.0, value
    return float(value), None


def _step_devices(group, named):
    _check_dev("tables[0]", group.tables[0])
    for name, t in named:
        if t is not None:
            _check_dev(name, t, group.device)


def sparse_row_update_grouped(group, ids, rows, *, rule, lr, states=None, eps=1e-8, count=None, last_id=None,
                              stochastic_rounding=False, seeds=None, step=0):
    """sparse_row_update on a group of SEPARATE table tensors, in ONE launch (cuembed::SparseRowUpdateGrouped): (ids, rows)
    is the compressed gradient of the group -- GroupedGrad's ids, GLOBAL rows of the tables laid end to end, distinct and
    inside [0, group.total_rows) wherever valid -- and for every valid entry k the kernel finds the table t with
    row_base[t] <= ids[k] < row_base[t + 1] itself and updates row ids[k] - row_base[t] of group.tables[t] and of states[t]
    in place from rows[k].  Rows that no valid entry names keep their bits.  Returns None.

        rule="sgd"              states=None
        rule="adagrad"          states: num_tables float32 tensors [rows_t, width]
        rule="rowwise_adagrad"  states: num_tables float32 tensors [rows_t]

    The rules, lr (a float or a one-element fp32 device tensor), eps and the count sources count=int | count=tensor |
    last_id=tensor are sparse_row_update's; a count below zero or above ids.numel() applies nothing.  The least aligned
    table (and, for "adagrad", state tensor) decides the lane width for the whole group, and the result has the bits of
    num_tables sparse_row_update calls at that lane width.

    stochastic_rounding=True, seeds=[...] (float16 / bfloat16 tables): ONE SEED PER TABLE, ints in [0, 2**64), and one
    `step` for the group, an int in [0, 2**64) or a one-element int64 device tensor.  (seeds may also be the int64
    device tensor [num_tables] that holds the seeds' bits, as the torch op takes it.)  The bits of entry k are those of
    (seeds[t], step, ids[k] - row_base[t], column): the step equals num_tables sparse_row_update(stochastic_rounding=True,
    seed=seeds[t], step=step) calls, and a table's bits depend neither on the group it is in nor on its place there.  (The
    single-table step on a one-storage group's flat tensor names its bits by the global row: other bits.)  There are no
    default seeds -- one seed for the group would give row r of every table the same bits -- so stochastic_rounding=True
    without seeds is an error, and so are seeds without it.  The seeds' device tensor is built at the first call with
    these seeds and kept on the group.
    Everything is validated before the launch; nothing is read back, so the call can be captured into a HIP graph (the
    pointer arrays of `states` are built at the first call with these tensors and kept on the group)."""
    group, it, n, seeds = _step_group(group, ids, rows, stochastic_rounding, seeds)
    step, step_word = _check_step(seeds, step)
    if rule not in UPDATE_RULES:
        raise ValueError("rule must be one of %r, got %r" % (sorted(UPDATE_RULES), rule))
    if rule == "sgd":
        if states is not None:
            raise ValueError("rule='sgd' takes no states")
    else:
        states = _check_group_states(group, "states", states, rule == "rowwise_adagrad")
    num_rows, count_word, words64, _, _ = _entry_counts(ids, count, last_id, None, None)
    lr, lr_word = _word("lr", lr, torch.float32)
    # ---- the call is in order: now the devices
    _step_devices(group, (("ids", ids), ("rows", rows), ("count", count_word), ("last_id", last_id), ("lr", lr_word),
                          ("step", step_word), ("seeds", seeds if isinstance(seeds, torch.Tensor) else None)) +
                  tuple(("states[%d]" % t, s) for t, s in enumerate(states or ())))
    host = dev = None
    state_bits = ()
    if states is not None:
        host, dev, bits = _state_ptrs(group, states)
        state_bits = (("states", bits),) if rule == "adagrad" else ()
    _check_alignment("tables", _or(group.host_ptrs), rows.element_size(), group.width,
                     others=(("rows", rows.data_ptr()),), state=state_bits, max_lanes=None)
    if n == 0:
        return None
    with torch.cuda.device(group.device):
        if seeds is not None:
            _lib.lib().cuembed_sparse_row_update_grouped_stochastic(
                group._host_array, _ptr(group.table_ptrs), host, _ptr(dev), group.num_tables, _ELEM[group.dtype],
                group.width, _ptr(group.row_base_device), UPDATE_RULES[rule], _ptr(ids), it, _ptr(rows), n, int(num_rows),
                _ptr(count_word), int(words64), _ptr(last_id), lr, _ptr(lr_word), float(eps),
                _ptr(_seeds_tensor(group, seeds)), step, _ptr(step_word), _stream(rows))
            return None
        _lib.lib().cuembed_sparse_row_update_grouped(
            group._host_array, _ptr(group.table_ptrs), host, _ptr(dev), group.num_tables, _ELEM[group.dtype], group.width,
            _ptr(group.row_base_device), UPDATE_RULES[rule], _ptr(ids), it, _ptr(rows), n, int(num_rows), _ptr(count_word),
            int(words64), _ptr(last_id), lr, _ptr(lr_word), float(eps), _stream(rows))
    return None


def sparse_row_adam_grouped(group, ids, rows, *, exp_avg, exp_avg_sq, lr, bias_factor=1.0, betas=(0.9, 0.999), eps=1e-8,
                            weight_decay=0.0, rowwise=False, count=None, last_id=None, stochastic_rounding=False,
                            seeds=None, step=0):
    """sparse_row_adam on a group of SEPARATE table tensors, in ONE launch (cuembed::SparseRowAdamGrouped): as
    sparse_row_update_grouped, with exp_avg a sequence of num_tables float32 tensors [rows_t, width] and exp_avg_sq one of
    [rows_t, width] tensors, or with rowwise=True of [rows_t] tensors.  lr, bias_factor (a float or a one-element fp32
    device tensor: adam_clock_advance's word, one clock for the group), betas, eps, weight_decay (decoupled, named rows
    only) and the formulas are sparse_row_adam's; the result has the bits of num_tables sparse_row_adam calls at the
    group's lane width.  stochastic_rounding=True, seeds=[...], step: as in sparse_row_update_grouped -- one seed per table,
    the bits of num_tables sparse_row_adam(stochastic_rounding=True, seed=seeds[t], step=step) calls.  Nothing is read
    back."""
    group, it, n, seeds = _step_group(group, ids, rows, stochastic_rounding, seeds)
    step, step_word = _check_step(seeds, step)
    exp_avg = _check_group_states(group, "exp_avg", exp_avg, False)
    exp_avg_sq = _check_group_states(group, "exp_avg_sq", exp_avg_sq, bool(rowwise))
    beta1, beta2 = _check_betas(betas)
    if not float(eps) >= 0.0:
        raise ValueError("eps must not be negative, got %r" % (eps,))
    if not float(weight_decay) >= 0.0:
        raise ValueError("weight_decay must not be negative, got %r" % (weight_decay,))
    num_rows, count_word, words64, _, _ = _entry_counts(ids, count, last_id, None, None)
    lr, lr_word = _word("lr", lr, torch.float32)
    bias_factor, bias_word = _word("bias_factor", bias_factor, torch.float32)
    # ---- the call is in order: now the devices
    _step_devices(group, (("ids", ids), ("rows", rows), ("count", count_word), ("last_id", last_id), ("lr", lr_word),
                          ("bias_factor", bias_word), ("step", step_word),
                          ("seeds", seeds if isinstance(seeds, torch.Tensor) else None)) +
                  tuple(("exp_avg[%d]" % t, s) for t, s in enumerate(exp_avg)) +
                  tuple(("exp_avg_sq[%d]" % t, s) for t, s in enumerate(exp_avg_sq)))
    m_host, m_dev, m_bits = _state_ptrs(group, exp_avg)
    v_host, v_dev, v_bits = _state_ptrs(group, exp_avg_sq)
    _check_alignment("tables", _or(group.host_ptrs), rows.element_size(), group.width,
                     others=(("rows", rows.data_ptr()),),
                     state=(("exp_avg", m_bits),) + ((("exp_avg_sq", v_bits),) if not rowwise else ()), max_lanes=None)
    if n == 0:
        return None
    with torch.cuda.device(group.device):
        if seeds is not None:
            _lib.lib().cuembed_sparse_row_adam_grouped_stochastic(
                group._host_array, _ptr(group.table_ptrs), m_host, _ptr(m_dev), v_host, _ptr(v_dev), group.num_tables,
                _ELEM[group.dtype], group.width, _ptr(group.row_base_device),
                ADAM_RULES["rowwise_adam" if rowwise else "adam"], _ptr(ids), it, _ptr(rows), n, int(num_rows),
                _ptr(count_word), int(words64), _ptr(last_id), lr, _ptr(lr_word), bias_factor, _ptr(bias_word), beta1,
                1.0 - beta1, beta2, 1.0 - beta2, float(eps), float(weight_decay), _ptr(_seeds_tensor(group, seeds)), step,
                _ptr(step_word), _stream(rows))
            return None
        _lib.lib().cuembed_sparse_row_adam_grouped(
            group._host_array, _ptr(group.table_ptrs), m_host, _ptr(m_dev), v_host, _ptr(v_dev), group.num_tables,
            _ELEM[group.dtype], group.width, _ptr(group.row_base_device),
            ADAM_RULES["rowwise_adam" if rowwise else "adam"], _ptr(ids), it, _ptr(rows), n, int(num_rows),
            _ptr(count_word), int(words64), _ptr(last_id), lr, _ptr(lr_word), bias_factor, _ptr(bias_word), beta1,
            1.0 - beta1, beta2, 1.0 - beta2, float(eps), float(weight_decay), _stream(rows))
    return None


def _or(pointers):
    bits = 0
    for p in pointers:
        bits |= p
    return bits
