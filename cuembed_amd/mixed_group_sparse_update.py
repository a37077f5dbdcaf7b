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
from .group_layout import INT_MAX
from .grouped_backward import MAX_GROUPED_STEP_TABLES, _adam_step, _update_step
from .mixed_group import MixedTableGroup
from .ops import _ELEM, _ptr, _stream

_STATE_TENSORS = {"sgd": 0, "adagrad": 1, "rowwise_adagrad": 1, "adam": 2, "rowwise_adam": 2}


def _mixed_group(group, stochastic_rounding, counts):
    """What only the mixed steps refuse, first and without the GPU, then the group as a MixedTableGroup.  The rest of the
    step is the same-width group's: grouped_backward._update_step / _adam_step."""
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
    return group


def _widths_device(group):
    """The widths as ONE int32 device tensor, built at the first use and kept on the group."""
    if group._widths_device is None:
        group._widths_device = torch.tensor(group.widths, dtype=torch.int32, device=group.device)
    return group._widths_device


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
    group = _mixed_group(group, stochastic_rounding, counts)
    call = _update_step(group, ids, rows, rule, lr, states, eps, count, last_id)
    if call is not None:
        head, tail, _ = call
        with torch.cuda.device(group.device):
            _lib.lib().cuembed_sparse_row_update_mixed_group(*head, group._widths_array, _ptr(_widths_device(group)), *tail,
                                                             _stream(rows))
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
    group = _mixed_group(group, stochastic_rounding, counts)
    call = _adam_step(group, ids, rows, exp_avg, exp_avg_sq, lr, bias_factor, betas, eps, weight_decay, rowwise, count,
                      last_id)
    if call is not None:
        head, tail, _ = call
        with torch.cuda.device(group.device):
            _lib.lib().cuembed_sparse_row_adam_mixed_group(*head, group._widths_array, _ptr(_widths_device(group)), *tail,
                                                           _stream(rows))
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
