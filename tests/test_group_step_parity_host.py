"""The optimizer step of a same-width group (TableGroup) and of a mixed-width group (MixedTableGroup) refuse the same
bad calls with the same words, without a GPU: one table of bad calls goes through sparse_row_update_grouped /
sparse_row_adam_grouped and through sparse_row_update_mixed_group / sparse_row_adam_mixed_group on groups built from the
same tables (the tensors live on the CPU: a call that got as far as the device check raises RuntimeError instead).  Then
what only the mixed step refuses, and the attributes the four group updaters expose."""
import re

import pytest
import torch

import cuembed_amd as ce
from cuembed_amd import optim

ROWS, WIDTH = (3, 5), 8


def groups(rows=ROWS, dtype=torch.float32):
    """(TableGroup, MixedTableGroup) over the same tensors."""
    tables = [torch.zeros(n, WIDTH, dtype=dtype) for n in rows]
    return ce.TableGroup(tables), ce.MixedTableGroup(tables)


def entries(n=4, width=WIDTH, dtype=torch.float32):
    return torch.arange(n, dtype=torch.int32), torch.zeros(n, width, dtype=dtype)


def states(rowwise=False, rows=ROWS, dtype=torch.float32):
    return [torch.zeros((n,) if rowwise else (n, WIDTH), dtype=dtype) for n in rows]


STEPS = dict(update=(ce.sparse_row_update_grouped, ce.sparse_row_update_mixed_group, lambda: dict(rule="sgd", lr=0.1)),
             adam=(ce.sparse_row_adam_grouped, ce.sparse_row_adam_mixed_group,
                   lambda: dict(exp_avg=states(), exp_avg_sq=states(), lr=0.1)))
LAST = torch.zeros(1, dtype=torch.int32)

# (id, which step, the exception, a fragment of its message, what the bad call changes: keywords, or ids / rows / rows_of)
BAD_CALLS = [
    ("unknown rule", "update", ValueError, "rule must be one of", dict(rule="momentum")),
    ("states with sgd", "update", ValueError, "rule='sgd' takes no states", dict(states=states())),
    ("states: wrong length", "update", ValueError, "states must hold one tensor per table: the group has 2 tables, got 1",
     dict(rule="adagrad", states=states()[:1])),
    ("states: wrong dtype", "update", TypeError, r"states\[0\] must be float32",
     dict(rule="adagrad", states=states(dtype=torch.float64))),
    ("states: wrong shape", "update", ValueError, r"states\[1\] must have shape \(5, 8\), got \(6, 8\)",
     dict(rule="adagrad", states=states(rows=(3, 6)))),
    ("states: the other rule's shape", "update", ValueError, r"states\[0\] must have shape \(3,\), got \(3, 8\)",
     dict(rule="rowwise_adagrad", states=states())),
    ("states: one tensor", "update", TypeError, "states must be a sequence of 2 float32 tensors",
     dict(rule="adagrad", states=torch.zeros(8, WIDTH))),
    ("exp_avg: wrong length", "adam", ValueError, "exp_avg must hold one tensor per table", dict(exp_avg=states()[:1])),
    ("exp_avg_sq: wrong dtype", "adam", TypeError, r"exp_avg_sq\[0\] must be float32",
     dict(exp_avg_sq=states(dtype=torch.float16))),
    ("exp_avg_sq: wrong shape", "adam", ValueError, r"exp_avg_sq\[0\] must have shape \(3,\), got \(3, 8\)",
     dict(rowwise=True)),
    ("betas out of range", "adam", ValueError, "betas", dict(betas=(0.9, 1.0))),
    ("negative eps", "adam", ValueError, "eps must not be negative", dict(eps=-1.0)),
    ("negative weight_decay", "adam", ValueError, "weight_decay must not be negative", dict(weight_decay=-0.1)),
    ("bias_factor of two words", "adam", TypeError, "a device-side bias_factor must be a one-element",
     dict(bias_factor=torch.ones(2))),
]
for _step in ("update", "adam"):
    BAD_CALLS += [
        ("rows: wrong dtype", _step, TypeError, "rows must have the tables' dtype", dict(rows=entries(dtype=torch.float16)[1])),
        ("rows: wrong width", _step, ValueError, r"rows must be \[entries, ", dict(rows=entries(width=WIDTH + 2)[1])),
        ("ids / rows count mismatch", _step, ValueError, "ids must hold one entry per row of rows: 5 ids, 4 rows",
         dict(ids=torch.arange(5, dtype=torch.int32))),
        ("ids: not an index type", _step, TypeError, "int32 or int64", dict(ids=torch.arange(4, dtype=torch.int16))),
        ("more than 1023 tables", _step, ValueError, "a grouped step takes at most 1023 tables, the group has 1024",
         dict(rows_of=(1,) * 1024)),
        ("both count and last_id", _step, ValueError, "at most one", dict(count=2, last_id=LAST)),
        ("count beyond the entries", _step, ValueError, "count must be in", dict(count=5)),
        ("lr of two words", _step, TypeError, "a device-side lr must be a one-element", dict(lr=torch.ones(2))),
    ]


def raised(fn, group, ids, rows, kw):
    with pytest.raises(Exception) as info:
        fn(group, ids, rows, **kw)
    return type(info.value), str(info.value)


def same_words(mixed_message):
    """The documented differences: the mixed step names the padded width, and says why."""
    return mixed_message.replace("W_max = %d], padded to the widest table (a ragged gradient layout is not taken)" % WIDTH,
                                 "width = %d]" % WIDTH)


@pytest.mark.parametrize("step, error, fragment, change", [pytest.param(*c[1:], id="%s-%s" % (c[1], c[0])) for c in BAD_CALLS])
def test_both_kinds_of_group_refuse_a_bad_call_with_the_same_words(step, error, fragment, change):
    grouped_fn, mixed_fn, base = STEPS[step]
    change = dict(change)
    same, mixed = groups(change.pop("rows_of", ROWS))
    ids, rows = entries()
    ids, rows = change.pop("ids", ids), change.pop("rows", rows)
    kw = dict(base(), **change)
    if same.num_tables != len(ROWS):
        kw.update({k: [] for k in ("exp_avg", "exp_avg_sq") if k in kw})     # (never looked at: the group is refused first)
    got_type, got = raised(grouped_fn, same, ids, rows, kw)
    mixed_type, mixed_got = raised(mixed_fn, mixed, ids, rows, kw)
    assert got_type is error and mixed_type is error
    assert re.search(fragment, got), got
    assert same_words(mixed_got) == got


def test_a_valid_call_gets_as_far_as_the_device_check_on_both():
    """What the table relies on: with everything in order the first thing that fails on CPU tensors is the device."""
    ids, rows = entries()
    for step in STEPS.values():
        for fn, group in zip(step[:2], groups()):
            with pytest.raises(RuntimeError, match="must live on the GPU"):
                fn(group, ids, rows, **step[2]())


def test_what_only_the_mixed_step_refuses():
    from cuembed_amd.row_cache import CachedHostTable
    _, mixed = groups(dtype=torch.float16)
    ids, rows = entries(dtype=torch.float16)
    cached = CachedHostTable.__new__(CachedHostTable)      # (the type alone is looked at: building one needs the GPU)
    for fn, base in (STEPS["update"][1:], STEPS["adam"][1:]):
        with pytest.raises(ValueError, match="the optimizer step of a mixed-width group rounds to nearest: stochastic "
                                             "rounding is not available for a MixedTableGroup"):
            fn(mixed, ids, rows, stochastic_rounding=True, **base())
        with pytest.raises(ValueError, match="the optimizer step of a mixed-width group takes one piece: count= or "
                                             "last_id=, not counts="):
            fn(mixed, ids, rows, counts=torch.zeros(2, dtype=torch.int32), **base())
        for behind_the_cache in (cached, [cached, mixed.tables[1]]):
            with pytest.raises(TypeError, match="tables behind the row cache have no mixed-width optimizer step: a "
                                                "MixedTableGroup holds device tensors"):
                fn(behind_the_cache, ids, rows, **base())
        with pytest.raises(TypeError, match="group must be a MixedTableGroup or a list of tables, got int"):
            fn(3, ids, rows, **base())
        with pytest.raises(TypeError):       # the mixed steps have no seeds to take
            fn(mixed, ids, rows, seeds=[1, 2], **base())


def test_the_four_group_updaters_expose_the_same_attributes():
    same, mixed = groups(dtype=torch.float16)

    def public(updater):
        return sorted(k for k in vars(updater) if not k.startswith("_"))

    for rule in ("sgd", "adagrad", "rowwise_adagrad"):
        a, b = optim.GroupSparseUpdater(same, rule, 0.1), optim.MixedGroupSparseUpdater(mixed, rule, 0.1)
        assert {"group", "rule", "lr", "eps", "states"} <= set(public(a)) and set(public(b)) <= set(public(a))
        assert set(public(a)) - set(public(b)) <= {"seeds", "stochastic_rounding", "rounding_step"}
        assert (a.rule, a.lr, a.eps) == (b.rule, b.lr, b.eps)
        assert [tuple(t.shape) for t in a.states or ()] == [tuple(t.shape) for t in b.states or ()]
        assert (a.states is None) == (b.states is None) == (rule == "sgd")
    for rowwise in (False, True):
        a = optim.GroupSparseAdamUpdater(same, 0.1, betas=(0.8, 0.9), weight_decay=0.5, rowwise=rowwise, bias_correction=False)
        b = optim.MixedGroupSparseAdamUpdater(mixed, 0.1, betas=(0.8, 0.9), weight_decay=0.5, rowwise=rowwise,
                                              bias_correction=False)
        wanted = {"group", "lr", "betas", "eps", "weight_decay", "rowwise", "bias_correction", "exp_avg", "exp_avg_sq",
                  "powers", "bias_factor"}
        assert wanted <= set(public(a)) and set(public(b)) <= set(public(a))
        assert set(public(a)) - set(public(b)) <= {"seeds", "stochastic_rounding", "rounding_step"}
        for name in ("lr", "betas", "eps", "weight_decay", "rowwise", "bias_correction"):
            assert getattr(a, name) == getattr(b, name)
        for name in ("exp_avg", "exp_avg_sq"):
            assert [tuple(t.shape) for t in getattr(a, name)] == [tuple(t.shape) for t in getattr(b, name)]
        assert a.powers.tolist() == b.powers.tolist() == [0.0, 1.0, 1.0]
        assert a.bias_factor.tolist() == b.bias_factor.tolist() == [1.0] and a._one.tolist() == b._one.tolist() == [1.0]
    for make in (lambda **kw: optim.MixedGroupSparseUpdater(mixed, "sgd", 0.1, **kw),
                 lambda **kw: optim.MixedGroupSparseAdamUpdater(mixed, 0.1, **kw)):
        with pytest.raises(ValueError, match="mixed-width group rounds to nearest: stochastic rounding is not available"):
            make(stochastic_rounding=True)
        with pytest.raises(TypeError):       # no seeds in the mixed updaters' signatures
            make(seeds=[1, 2])
