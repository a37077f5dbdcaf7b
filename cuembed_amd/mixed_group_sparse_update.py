"""The sparse optimizer step on a group of embedding tables of DIFFERENT widths, in one launch (an extension).

cuembed_amd.mixed_group_backward ends at a MixedGroupedGrad: ascending global ids, gradient rows PADDED to the widest
table, the entry count on the device.  The functions here consume exactly that, for all five rules:

    sparse_row_update_mixed_group(group, ids, rows, rule=..., lr=..., states=...)     sgd / adagrad / rowwise_adagrad
    sparse_row_adam_mixed_group(group, ids, rows, exp_avg=..., exp_avg_sq=..., ...)   adam / rowwise_adam
    mixed_group_update_launch_shape(...)                                              the launch shape (host arithmetic)

For every valid entry k, with t the last table whose row_base[t] <= ids[k] and r = ids[k] - row_base[t], tables[t][r, :W_t]
and the state of row r of table t are updated in place from rows[k, :W_t]; the columns from W_t on are never read.
Per-element state is float32 [rows_t, W_t], row-wise state float32 [rows_t].  One lane width serves the launch
(group_layout.mixed_lane_bytes over the widths, the table bases, rows and, for rules with per-element state, the state
bases), and tables and state have the bits of num_tables sparse_row_update / sparse_row_adam calls at width W_t and that
lane width.  Everything validates before any launch; nothing is allocated, copied or read back, so a call can be
captured into a HIP graph (the small device arrays -- the state pointers, the widths -- are built at the first call
with these tensors and kept on the group).  The updaters are cuembed_amd.optim.MixedGroupSparseUpdater /
MixedGroupSparseAdamUpdater.

Not taken, each with its own error: stochastic rounding, counts= (several pieces), tables behind the row cache, a ragged
gradient layout (rows must be [n, W_max]), quantized or mixed-dtype groups (a MixedTableGroup holds neither).
"""
import ctypes

import torch

from . import _lib
from .group_layout import INT_MAX, mixed_lane_bytes
from .grouped_backward import MAX_GROUPED_STEP_TABLES, _state_ptrs, _step_devices, _word
from .mixed_group import MixedTableGroup
from .ops import _ELEM, ADAM_RULES, UPDATE_RULES, _check_betas, _entry_counts, _index_code, _ptr, _stream

_STATE_TENSORS = {"sgd": 0, "adagrad": 1, "rowwise_adagrad": 1, "adam": 2, "rowwise_adam": 2}


def _mixed_step_group(group, ids, rows, stochastic_rounding, counts):
    """What both mixed steps check first, without the GPU: the group, the refusals, ids and rows.  Returns (group, index
    code, n)."""
    if stochastic_rounding:
        raise ValueError("the optimizer step of a mixed-width group rounds to nearest: stochastic rounding is not "
                         "available for a MixedTableGroup")
    if counts is not None:
        raise ValueError("the optimizer step of a mixed-width group takes one piece: count= or last_id=, not counts=")
    if not isinstance(group, MixedTableGroup):
        from .row_cache import CachedHostTable
        if isinstance(group, CachedHostTable) or (isinstance(group, (list, tuple)) and
                                                  any(isinstance(t, CachedHostTable) for t in group)):
            raise TypeError("tables behind the row cache have no mixed-width optimizer step: a MixedTableGroup holds "
                            "device tensors")
        if not isinstance(group, (list, tuple)):
            raise TypeError("group must be a MixedTableGroup or a list of tables, got %s" % type(group).__name__)
        group = MixedTableGroup(group)
    if group.num_tables > MAX_GROUPED_STEP_TABLES:
        raise ValueError("a grouped step takes at most %d tables, the group has %d"
                         % (MAX_GROUPED_STEP_TABLES, group.num_tables))
    for name, t in (("ids", ids), ("rows", rows)):
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s must be a torch.Tensor" % name)
    it = _index_code("ids", ids)
    if rows.dtype != group.dtype:
        raise TypeError("rows must have the tables' dtype (%s), got %s" % (group.dtype, rows.dtype))
    w_max = max(group.widths)
    if rows.dim() != 2 or rows.shape[1] != w_max:
        raise ValueError("rows must be [entries, W_max = %d], padded to the widest table (a ragged gradient layout is not "
                         "taken), got %r" % (w_max, tuple(rows.shape)))
    if ids.dim() != 1 or rows.shape[0] != ids.numel():
        raise ValueError("ids must hold one entry per row of rows: %d ids, %d rows" % (ids.numel(), rows.shape[0]))
    return group, it, ids.numel()


def _check_mixed_states(group, name, states, rowwise):
    """`states`: a sequence of num_tables float32 tensors, [rows_t, W_t] or (rowwise) [rows_t]."""
    if isinstance(states, torch.Tensor) or not isinstance(states, (list, tuple)):
        raise TypeError("%s must be a sequence of %d float32 tensors, one per table" % (name, group.num_tables))
    if len(states) != group.num_tables:
        raise ValueError("%s must hold one tensor per table: the group has %d tables, got %d"
                         % (name, group.num_tables, len(states)))
    for t, (s, n, w) in enumerate(zip(states, group.row_counts, group.widths)):
        want = (n,) if rowwise else (n, w)
        if not isinstance(s, torch.Tensor):
            raise TypeError("%s[%d] must be a float32 tensor of shape %r" % (name, t, want))
        if s.dtype != torch.float32:
            raise TypeError("%s[%d] must be float32, got %s" % (name, t, s.dtype))
        if tuple(s.shape) != want:
            raise ValueError("%s[%d] must have shape %r, got %r" % (name, t, want, tuple(s.shape)))
    return tuple(states)


def _widths_device(group):
    """The widths as ONE int32 device tensor, built at the first use and kept on the group."""
    if group._widths_device is None:
        group._widths_device = torch.tensor(group.widths, dtype=torch.int32, device=group.device)
    return group._widths_device


def _check_alignment(group, rows_ptr, per_element):
    """ValueError where the library would abort because NO lane width serves the call: a table base or rows that is not
    4-byte aligned (mixed_lane_bytes says so), or a per-element state base (`per_element`: (name, OR of the bases) pairs)
    that the narrowest lane, 4 bytes of a row, cannot move as fp32 words.  Which lane width the launch gets is the
    library's to decide (detail::MixedGroupUpdateLaneBytes; mixed_group_update_launch_shape reports it): nothing here
    repeats that rule."""
    size = group.tables[0].element_size()
    mixed_lane_bytes(group.widths, size,
                     tuple(("tables[%d]" % k, p) for k, p in enumerate(group.host_ptrs)) + (("rows", rows_ptr),))
    align = 4 * (4 // size)
    for name, p in per_element:
        if int(p) % align:
            raise ValueError("%s must be %d-byte aligned for a table of %d-byte elements: the narrowest lane moves that "
                             "much of it" % (name, align, size))


def sparse_row_update_mixed_group(group, ids, rows, *, rule, lr, states=None, eps=1e-8, count=None, last_id=None,
                                  stochastic_rounding=False, counts=None):
    """sparse_row_update on a MixedTableGroup (or a list of tables of different widths), in ONE launch
    (cuembed::SparseRowUpdateMixedGroup): (ids, rows) is the group's compressed gradient as embedding_backward_mixed_group
    returns it -- ascending GLOBAL rows and [entries, W_max] rows with entry k's gradient in rows[k, :W_t].  Returns None.

        rule="sgd"              states=None
        rule="adagrad"          states: num_tables float32 tensors [rows_t, W_t]
        rule="rowwise_adagrad"  states: num_tables float32 tensors [rows_t]

    lr (a float or a one-element fp32 device tensor), eps and the count sources count=int | count=tensor | last_id=tensor
    are sparse_row_update's; a count below zero or above ids.numel() applies nothing.  The result has the bits of
    num_tables sparse_row_update calls, each at width W_t and the group's lane width.  stochastic_rounding=True and
    counts= are refused."""
    group, it, n = _mixed_step_group(group, ids, rows, stochastic_rounding, counts)
    if rule not in UPDATE_RULES:
        raise ValueError("rule must be one of %r, got %r" % (sorted(UPDATE_RULES), rule))
    if rule == "sgd":
        if states is not None:
            raise ValueError("rule='sgd' takes no states")
    else:
        states = _check_mixed_states(group, "states", states, rule == "rowwise_adagrad")
    num_rows, count_word, words64, _, _ = _entry_counts(ids, count, last_id, None, None)
    lr, lr_word = _word("lr", lr, torch.float32)
    # ---- the call is in order: now the devices
    _step_devices(group, (("ids", ids), ("rows", rows), ("count", count_word), ("last_id", last_id), ("lr", lr_word)) +
                  tuple(("states[%d]" % t, s) for t, s in enumerate(states or ())))
    host = dev = None
    per_element = ()
    if states is not None:
        host, dev, bits = _state_ptrs(group, states)
        per_element = (("states", bits),) if rule == "adagrad" else ()
    _check_alignment(group, rows.data_ptr(), per_element)
    if n == 0:
        return None
    with torch.cuda.device(group.device):
        _lib.lib().cuembed_sparse_row_update_mixed_group(
            group._host_array, _ptr(group.table_ptrs), host, _ptr(dev), group._widths_array, _ptr(_widths_device(group)),
            group.num_tables, _ELEM[group.dtype], max(group.widths), _ptr(group.row_base_device), UPDATE_RULES[rule],
            _ptr(ids), it, _ptr(rows), n, int(num_rows), _ptr(count_word), int(words64), _ptr(last_id), lr, _ptr(lr_word),
            float(eps), _stream(rows))
    return None


def sparse_row_adam_mixed_group(group, ids, rows, *, exp_avg, exp_avg_sq, lr, bias_factor=1.0, betas=(0.9, 0.999),
                                eps=1e-8, weight_decay=0.0, rowwise=False, count=None, last_id=None,
                                stochastic_rounding=False, counts=None):
    """sparse_row_adam on a MixedTableGroup, in ONE launch (cuembed::SparseRowAdamMixedGroup): as
    sparse_row_update_mixed_group, with exp_avg a sequence of num_tables float32 tensors [rows_t, W_t] and exp_avg_sq one
    of [rows_t, W_t] tensors, or with rowwise=True of [rows_t] tensors.  lr, bias_factor (a float or a one-element fp32
    device tensor: adam_clock_advance's word, one clock for the group), betas, eps, weight_decay (decoupled, named rows
    only) and the formulas are sparse_row_adam's; the result has the bits of num_tables sparse_row_adam calls, each at
    width W_t and the group's lane width.  Nothing is read back."""
    group, it, n = _mixed_step_group(group, ids, rows, stochastic_rounding, counts)
    exp_avg = _check_mixed_states(group, "exp_avg", exp_avg, False)
    exp_avg_sq = _check_mixed_states(group, "exp_avg_sq", exp_avg_sq, bool(rowwise))
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
                          ("bias_factor", bias_word)) +
                  tuple(("exp_avg[%d]" % t, s) for t, s in enumerate(exp_avg)) +
                  tuple(("exp_avg_sq[%d]" % t, s) for t, s in enumerate(exp_avg_sq)))
    m_host, m_dev, m_bits = _state_ptrs(group, exp_avg)
    v_host, v_dev, v_bits = _state_ptrs(group, exp_avg_sq)
    _check_alignment(group, rows.data_ptr(), (("exp_avg", m_bits),) + ((("exp_avg_sq", v_bits),) if not rowwise else ()))
    if n == 0:
        return None
    with torch.cuda.device(group.device):
        _lib.lib().cuembed_sparse_row_adam_mixed_group(
            group._host_array, _ptr(group.table_ptrs), m_host, _ptr(m_dev), v_host, _ptr(v_dev), group._widths_array,
            _ptr(_widths_device(group)), group.num_tables, _ELEM[group.dtype], max(group.widths),
            _ptr(group.row_base_device), ADAM_RULES["rowwise_adam" if rowwise else "adam"], _ptr(ids), it, _ptr(rows), n,
            int(num_rows), _ptr(count_word), int(words64), _ptr(last_id), lr, _ptr(lr_word), bias_factor, _ptr(bias_word),
            beta1, 1.0 - beta1, beta2, 1.0 - beta2, float(eps), float(weight_decay), _stream(rows))
    return None


def mixed_group_update_launch_shape(elem_dtype, widths, total_entries, rule="sgd", pointer_bits=0, state_pointer_bits=0,
                                    compute_units=256):
    """Launch shape of the mixed-width step (pure host arithmetic when compute_units > 0; 0 = ask the current device).
    rule: one of the five (it decides the LDS bytes: row_base, the table bases, the bases of the rule's state tensors, the
    widths).  pointer_bits: the table bases and rows OR-ed; state_pointer_bits: the per-element state bases OR-ed (0 =
    aligned buffers).  A workgroup is four wavefronts; a wavefront serves tiles of 64 entries in passes, and a pass on
    table t serves entries_per_pass[t] entries with lanes_per_entry[t] lanes each (64 and 1 for a row of more than 64
    lanes, which the wavefront walks in slices)."""
    if elem_dtype not in _ELEM:
        raise TypeError("elem_dtype must be float32, float16 or bfloat16, got %s" % elem_dtype)
    if rule not in _STATE_TENSORS:
        raise ValueError("rule must be one of %r, got %r" % (sorted(_STATE_TENSORS), rule))
    widths = [int(w) for w in widths]
    T = len(widths)
    if T < 1 or T > MAX_GROUPED_STEP_TABLES:
        raise ValueError("a grouped step takes 1 to %d tables, got %d" % (MAX_GROUPED_STEP_TABLES, T))
    if any(w <= 0 or (w * elem_dtype.itemsize) % 4 for w in widths) or sum(widths) > INT_MAX:
        raise ValueError("every row size must be a multiple of 4 bytes and the widths must sum to at most 2^31 - 1")
    if total_entries < 0:
        raise ValueError("total_entries must not be negative")
    if pointer_bits % 4 or state_pointer_bits % 4:
        raise ValueError("every pointer must be 4-byte aligned")
    out = (ctypes.c_int * 3)()
    per_table = (ctypes.c_int * (2 * T))()
    _lib.lib().cuembed_mixed_group_update_launch_shape((ctypes.c_int * T)(*widths), T, _ELEM[elem_dtype],
                                                       int(total_entries), _STATE_TENSORS[rule], int(pointer_bits),
                                                       int(state_pointer_bits), int(compute_units), out, per_table)
    return dict(elems_per_lane=out[0], grid=out[1], lds_bytes=out[2], lanes_per_entry=list(per_table[0::2]),
                entries_per_pass=list(per_table[1::2]))
