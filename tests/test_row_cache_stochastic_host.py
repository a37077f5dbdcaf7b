"""On the CPU: the inputs of tests/test_gpu_row_cache_stochastic.py's "the names are the table rows" can tell right from
wrong.  With tests/stochastic_rounding_reference.py on the data of tests/row_cache_stochastic_reference.py, the table
after the three stochastic SGD steps differs from the round-to-nearest one, and from the one obtained when every row's
fields are drawn for another row -- the slot the cache puts it in -- in at least a quarter of the updated elements.  A
condition on the test data, not a measurement."""
import numpy as np
import pytest

import row_cache_stochastic_reference as N

KINDS = ["fp16", "bf16"]


@pytest.mark.parametrize("kind", KINDS)
def test_no_updated_row_sits_in_the_slot_of_its_own_number(kind):
    _, ids, _ = N.problem(kind)
    slots = N.slots(ids)
    assert np.unique(ids).size == N.ENTRIES and not np.intersect1d(ids, N.READ).size
    assert sorted(slots.tolist()) == list(range(10, 10 + N.ENTRIES))
    assert not (slots == ids).any() and ids.min() >= 64       # (no id is a slot number at all)
    assert np.array_equal(np.argsort(ids), np.argsort(slots))   # ascending rows take ascending ways


@pytest.mark.parametrize("kind", KINDS)
def test_the_data_tells_right_from_wrong(kind):
    table, ids, _ = N.problem(kind)
    right = N.trained(kind)
    nearest = N.trained(kind, seed=None)
    misnamed = N.trained(kind, names=N.slots(ids))
    assert np.array_equal(right, N.trained(kind, names=ids))
    untouched = np.setdiff1d(np.arange(N.ROWS), ids)
    for other in (nearest, misnamed):
        assert np.array_equal(other[untouched], table[untouched]) and np.array_equal(right[untouched], table[untouched])
        differing = (right[ids] != other[ids]).mean()
        assert differing >= 0.25, differing
    assert (right[ids] != table[ids]).mean() > 0.9


def test_the_new_entry_points_are_declared_in_plain_c_and_exported():
    import ctypes
    import os
    import re
    from cuembed_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    L = _lib.lib()
    with open(os.path.join(root, "include", "cuembed_amd.h")) as f:
        header = re.sub(r"\s+", " ", f.read())
    tails = {"cuembed_sparse_row_update_placed_stochastic": "const int64_t* state_ids, const int64_t* row_names);",
             "cuembed_sparse_row_adam_placed_stochastic":
                 "const int64_t* exp_avg_ids, const int64_t* exp_avg_sq_ids, const int64_t* row_names);"}
    for name, tail in tails.items():
        assert hasattr(L, name), name
        declared = re.search(r"\bvoid %s ?\(([^)]*\));" % name, header)
        assert declared and (declared.group(1) + ";").endswith("cuembed_stream_t stream, " + tail), name
        base = getattr(L, name.replace("_placed", ""))
        extra = tail.count("int64_t*")
        assert getattr(L, name).argtypes == list(base.argtypes) + [ctypes.c_void_p] * extra and getattr(L, name).restype is None


def test_the_constructors_check_the_rounding_before_anything_is_allocated():
    """optim._check_rounding's checks and messages, on tensors that are neither pinned nor on a device: the check comes
    first.  Without the option the seed is not looked at and the next check (pinned memory) is the one that raises."""
    import torch
    from cuembed_amd.row_cache import AdamRowCache, DynamicRowCache
    single, half = torch.zeros((8, 4), dtype=torch.float32), torch.zeros((8, 4), dtype=torch.float16)
    for build in (lambda t, **kw: DynamicRowCache(t, num_sets=1, **kw),
                  lambda t, **kw: DynamicRowCache(t, num_sets=1, rule="adagrad", **kw),
                  lambda t, **kw: AdamRowCache(t, num_sets=1, **kw)):
        with pytest.raises(TypeError, match="float32 table"):
            build(single, stochastic_rounding=True)
        for seed in (-1, 2 ** 64, True, 1.0):
            with pytest.raises(ValueError, match="seed must be an int"):
                build(half, stochastic_rounding=True, seed=seed)
        with pytest.raises(ValueError, match="PINNED"):
            build(half, stochastic_rounding=True, seed=2 ** 64 - 1)
        with pytest.raises(ValueError, match="PINNED"):
            build(half, seed=-1)
