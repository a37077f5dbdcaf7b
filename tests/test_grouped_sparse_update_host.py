"""The grouped optimizer step without a GPU: the new names and symbols exist and are bound, and every argument error of
sparse_row_update_grouped / sparse_row_adam_grouped and of the two updaters is raised before anything touches a device
(the tensors here live on the CPU: a call that got as far as the device check raises RuntimeError instead)."""
import ctypes
import re

import pytest
import torch

ROWS = (1, 5, 70)
WIDTH = 8


@pytest.fixture(scope="module")
def ce():
    import cuembed_amd
    return cuembed_amd


def group_of(ce, dtype=torch.float32, rows=ROWS):
    return ce.TableGroup([torch.zeros(n, WIDTH, dtype=dtype) for n in rows])


def entries(n=4, dtype=torch.float32, index=torch.int32):
    return torch.arange(n, dtype=index), torch.zeros(n, WIDTH, dtype=dtype)


def states(rowwise=False, rows=ROWS, dtype=torch.float32):
    return [torch.zeros((n,) if rowwise else (n, WIDTH), dtype=dtype) for n in rows]


def test_the_new_names_exist(ce):
    from cuembed_amd import cuembed_pyt, grouped_backward, optim
    assert ce.sparse_row_update_grouped is grouped_backward.sparse_row_update_grouped
    assert ce.sparse_row_adam_grouped is grouped_backward.sparse_row_adam_grouped
    assert callable(optim.GroupSparseUpdater) and callable(optim.GroupSparseAdamUpdater)
    assert hasattr(torch.ops.cuembed_pyt, "cuembed_sparse_row_update_grouped")
    assert hasattr(torch.ops.cuembed_pyt, "cuembed_sparse_row_adam_grouped")
    assert callable(cuembed_pyt.cuembed_sparse_row_update_grouped) and callable(cuembed_pyt.cuembed_sparse_row_adam_grouped)


def test_the_symbols_are_exported_with_argtypes(ce):
    lib = ce._lib.lib()
    for name, count in (("cuembed_sparse_row_update_grouped", 21), ("cuembed_sparse_row_adam_grouped", 30)):
        fn = getattr(lib, name)            # (AttributeError: the shared library does not export it)
        assert fn.restype is None and len(fn.argtypes) == count and fn.argtypes[-1] is ctypes.c_void_p
        assert fn.argtypes[:2] == [ctypes.c_void_p] * 2
    with open(ce._lib.__file__.replace("cuembed_amd/_lib.py", "include/cuembed_amd.h")) as f:
        header = f.read()
    for name in ("cuembed_sparse_row_update_grouped", "cuembed_sparse_row_adam_grouped"):
        declared = re.search(r"\bvoid %s ?\(([^)]*)\);" % name, header)
        assert declared and declared.group(1).startswith("const void* const* tables_host, const void* const* tables_device")
        assert declared.group(1).endswith("cuembed_stream_t stream")
        assert "const int64_t* row_base" in declared.group(1) and "int64_t total_entries" in declared.group(1)


def test_a_valid_call_gets_as_far_as_the_device_check(ce):
    """What the other tests rely on: with everything in order the first thing that fails on CPU tensors is the device."""
    ids, rows = entries()
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        ce.sparse_row_update_grouped(group_of(ce), ids, rows, rule="sgd", lr=0.1)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        ce.sparse_row_update_grouped(group_of(ce), ids, rows, rule="rowwise_adagrad", lr=0.1, states=states(True))
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        ce.sparse_row_adam_grouped(group_of(ce), ids, rows, exp_avg=states(), exp_avg_sq=states(True), lr=0.1, rowwise=True)


@pytest.mark.parametrize("bad, error", [
    (lambda: None, TypeError),                                          # a stateful rule without states
    (lambda: torch.zeros(76, WIDTH), TypeError),                         # one tensor instead of one per table
    (lambda: states()[:2], ValueError),                                  # wrong number
    (lambda: states(rows=(1, 5, 71)), ValueError),                       # wrong shape
    (lambda: states(rowwise=True), ValueError),                          # the other rule's shape
    (lambda: states(dtype=torch.float64), TypeError),                    # wrong dtype
    (lambda: states()[:2] + [None], TypeError),                          # not a tensor
])
def test_update_states_are_checked(ce, bad, error):
    ids, rows = entries()
    with pytest.raises(error):
        ce.sparse_row_update_grouped(group_of(ce), ids, rows, rule="adagrad", lr=0.1, states=bad())


def test_update_rules_and_their_states(ce):
    ids, rows = entries()
    with pytest.raises(ValueError, match="rule must be one of"):
        ce.sparse_row_update_grouped(group_of(ce), ids, rows, rule="momentum", lr=0.1)
    with pytest.raises(ValueError, match="takes no states"):
        ce.sparse_row_update_grouped(group_of(ce), ids, rows, rule="sgd", lr=0.1, states=states())
    with pytest.raises(ValueError):
        ce.sparse_row_update_grouped(group_of(ce), ids, rows, rule="rowwise_adagrad", lr=0.1, states=states())


@pytest.mark.parametrize("which", ["exp_avg", "exp_avg_sq"])
@pytest.mark.parametrize("bad, error", [
    (lambda rw: states(rw)[:1], ValueError),
    (lambda rw: states(rw, rows=(2, 5, 70)), ValueError),
    (lambda rw: states(rw, dtype=torch.float16), TypeError),
    (lambda rw: torch.zeros(3), TypeError),
])
def test_adam_moments_are_checked(ce, which, bad, error):
    ids, rows = entries()
    for rowwise in (False, True):
        kw = dict(exp_avg=states(), exp_avg_sq=states(rowwise))
        kw[which] = bad(rowwise and which == "exp_avg_sq")
        with pytest.raises(error):
            ce.sparse_row_adam_grouped(group_of(ce), ids, rows, lr=0.1, rowwise=rowwise, **kw)
    with pytest.raises(ValueError):       # per-element second moments for the row-wise rule
        ce.sparse_row_adam_grouped(group_of(ce), ids, rows, exp_avg=states(), exp_avg_sq=states(), lr=0.1, rowwise=True)


def test_adam_hyper_parameters_are_checked(ce):
    ids, rows = entries()
    kw = dict(exp_avg=states(), exp_avg_sq=states(), lr=0.1)
    with pytest.raises(ValueError, match="betas"):
        ce.sparse_row_adam_grouped(group_of(ce), ids, rows, betas=(0.9, 1.0), **kw)
    with pytest.raises(ValueError, match="eps"):
        ce.sparse_row_adam_grouped(group_of(ce), ids, rows, eps=-1.0, **kw)
    with pytest.raises(ValueError, match="weight_decay"):
        ce.sparse_row_adam_grouped(group_of(ce), ids, rows, weight_decay=-0.1, **kw)
    with pytest.raises(TypeError, match="bias_factor"):
        ce.sparse_row_adam_grouped(group_of(ce), ids, rows, bias_factor=torch.ones(2), **kw)


def both_steps(ce):
    return (lambda g, i, r, **kw: ce.sparse_row_update_grouped(g, i, r, rule="sgd", lr=0.1, **kw),
            lambda g, i, r, **kw: ce.sparse_row_adam_grouped(
                g, i, r, exp_avg=states(), exp_avg_sq=states(), lr=0.1, **kw))


def test_a_quantized_group_is_refused(ce):
    q = ce.TableGroup([torch.zeros(n, WIDTH + 8, dtype=torch.uint8) for n in ROWS])
    ids, rows = entries()
    for step in both_steps(ce):
        with pytest.raises(TypeError, match="quantized"):
            step(q, ids, rows)
    from cuembed_amd import optim
    with pytest.raises(TypeError, match="quantized"):
        optim.GroupSparseUpdater(q, "sgd", 0.1)
    with pytest.raises(TypeError, match="quantized"):
        optim.GroupSparseAdamUpdater(q, 0.1)


def test_stochastic_rounding_is_refused_at_every_python_layer(ce):
    from cuembed_amd import cuembed_pyt, optim
    ids, rows = entries(dtype=torch.float16)
    group = group_of(ce, torch.float16)
    for step in both_steps(ce):
        with pytest.raises(ValueError, match="stochastic rounding"):
            step(group, ids, rows, stochastic_rounding=True)
    with pytest.raises(ValueError, match="stochastic rounding"):
        optim.GroupSparseUpdater(group, "sgd", 0.1, stochastic_rounding=True)
    with pytest.raises(ValueError, match="stochastic rounding"):
        optim.GroupSparseAdamUpdater(group, 0.1, stochastic_rounding=True)
    assert "stochastic_rounding" in str(torch.ops.cuembed_pyt.cuembed_sparse_row_update_grouped.default._schema)
    assert "stochastic_rounding" in str(torch.ops.cuembed_pyt.cuembed_sparse_row_adam_grouped.default._schema)
    assert callable(cuembed_pyt.cuembed_sparse_row_update_grouped)


def test_the_count_sources_are_checked(ce):
    ids, rows = entries()
    for step in both_steps(ce):
        with pytest.raises(ValueError, match="at most one"):
            step(group_of(ce), ids, rows, count=2, last_id=torch.zeros(1, dtype=torch.int32))
        with pytest.raises(ValueError, match="count must be in"):
            step(group_of(ce), ids, rows, count=5)
        with pytest.raises(ValueError, match="count must be in"):
            step(group_of(ce), ids, rows, count=-1)
        with pytest.raises(TypeError, match="last_id"):
            step(group_of(ce), ids, rows, last_id=torch.zeros(1, dtype=torch.int64))     # not ids' dtype
        with pytest.raises(TypeError, match="count"):
            step(group_of(ce), ids, rows, count=torch.zeros(2, dtype=torch.int32))


def test_ids_and_rows_are_checked(ce):
    for step in both_steps(ce):
        with pytest.raises(ValueError, match="one entry per row"):
            step(group_of(ce), torch.arange(5, dtype=torch.int32), torch.zeros(4, WIDTH))
        with pytest.raises(ValueError, match="width"):
            step(group_of(ce), torch.arange(4, dtype=torch.int32), torch.zeros(4, WIDTH + 1))
        with pytest.raises(TypeError, match="dtype"):
            step(group_of(ce), torch.arange(4, dtype=torch.int32), torch.zeros(4, WIDTH, dtype=torch.float16))
        with pytest.raises(TypeError, match="int32 or int64"):
            step(group_of(ce), torch.arange(4, dtype=torch.int16), torch.zeros(4, WIDTH))
        with pytest.raises(TypeError):
            step(group_of(ce), [0, 1, 2, 3], torch.zeros(4, WIDTH))


def test_the_updaters_own_one_state_tensor_per_table(ce):
    from cuembed_amd import optim
    group = group_of(ce, torch.float16)
    assert optim.GroupSparseUpdater(group, "sgd", 0.1).states is None
    u = optim.GroupSparseUpdater(group, "adagrad", 0.1, initial_accumulator_value=0.5)
    assert [tuple(s.shape) for s in u.states] == [(n, WIDTH) for n in ROWS]
    assert all(s.dtype == torch.float32 and bool((s == 0.5).all()) for s in u.states)
    u = optim.GroupSparseUpdater(group, "rowwise_adagrad", 0.1)
    assert [tuple(s.shape) for s in u.states] == [(n,) for n in ROWS]
    a = optim.GroupSparseAdamUpdater(group, 0.1, rowwise=True)
    assert [tuple(s.shape) for s in a.exp_avg] == [(n, WIDTH) for n in ROWS]
    assert [tuple(s.shape) for s in a.exp_avg_sq] == [(n,) for n in ROWS]
    assert a.powers.tolist() == [0.0, 1.0, 1.0] and a.bias_factor.tolist() == [1.0]
    with pytest.raises(ValueError, match="rule must be one of"):
        optim.GroupSparseUpdater(group, "adam", 0.1)
    with pytest.raises(ValueError, match="betas"):
        optim.GroupSparseAdamUpdater(group, 0.1, betas=(1.0, 0.9))
    with pytest.raises(TypeError, match="GroupedGrad"):
        u.apply((torch.zeros(1), torch.zeros(1, WIDTH)))
    other = ce.GroupedGrad(torch.zeros(1, dtype=torch.int32), torch.zeros(1, WIDTH, dtype=torch.float16),
                           torch.zeros(1, dtype=torch.int32), (0, 2, 7, 77), None)
    with pytest.raises(ValueError, match="other row counts"):
        u.apply(other)


def test_padded_gradients_on_separate_tensors_still_raise(ce):
    """What stays as it is: the autograd surface refuses sparse_grad='padded' on a group of separate tensors (the new
    updaters are the capturable way), with the error of before."""
    from cuembed_amd import cuembed_pyt
    idx = torch.zeros(3, 2, 1, dtype=torch.int32)
    with pytest.raises(ValueError, match="needs a one-storage group"):
        cuembed_pyt.cuemb_embedding_grouped_trainable(group_of(ce), idx, sparse_grad="padded")
