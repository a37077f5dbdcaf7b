"""Training a group with mean pooling and with the per-lookup weight gradient, without a GPU: the new names, symbols and
keywords exist, every new argument error is raised before a device check, the defaults are those of before, the fake
implementations give shape and dtype, and the numpy model (grouped_train_reference) agrees with fp64 on hand-sized
cases."""
import numpy as np
import pytest
import torch

import exact_sums as X
import grouped_cases as C
import grouped_train_reference as R


@pytest.fixture(scope="module")
def ce():
    import cuembed_amd
    return cuembed_amd


@pytest.fixture(scope="module")
def pyt():
    from cuembed_amd import cuembed_pyt
    return cuembed_pyt


def cpu_tables(width=8, dtype=torch.float32):
    return [torch.from_numpy(C.table_values(t, rows, width)).to(dtype) for t, rows in enumerate(C.ROWS)]


def problem(batch=5, width=8, dtype=torch.float32):
    name, ids, off, hot, w = C.layouts(batch)[3]
    assert name == "csr_ragged"
    grad_y = torch.zeros(batch, len(C.ROWS), width, dtype=dtype)
    return torch.from_numpy(ids), torch.from_numpy(off), grad_y


def test_the_new_names_exist(ce, pyt):
    assert callable(ce.embedding_weight_grad_grouped) and callable(ce.grouped_mean_scale)
    from cuembed_amd import grouped_backward
    assert ce.embedding_weight_grad_grouped is grouped_backward.embedding_weight_grad_grouped
    import inspect
    assert inspect.signature(ce.embedding_backward_grouped).parameters["mode"].default == "sum"
    assert list(inspect.signature(ce.embedding_backward_grouped).parameters)[-1] == "mode"
    sig = inspect.signature(pyt.cuemb_embedding_grouped_trainable).parameters
    assert sig["mode"].default == "sum" and sig["weight_grad"].default is False
    sig = inspect.signature(pyt.TrainableEmbeddingBagGroup.__init__).parameters
    assert sig["mode"].default == "sum" and sig["weight_grad"].default is False
    assert list(inspect.signature(ce.embedding_weight_grad_grouped).parameters) == [
        "group", "grad_y", "indices", "offsets", "batch_size", "num_hots", "out"]


def test_the_symbols_are_exported_and_bound(ce):
    import ctypes
    lib = ce._lib.lib()
    for name, count in (("cuembed_embedding_weight_grad_grouped", 14), ("cuembed_grouped_mean_scale", 11)):
        fn = getattr(lib, name)
        assert fn.restype is None and len(fn.argtypes) == count and fn.argtypes[-1] is ctypes.c_void_p
    with open(ce._lib.__file__.replace("cuembed_amd/_lib.py", "include/cuembed_amd.h")) as f:
        header = f.read()
    assert "cuembed_embedding_weight_grad_grouped(" in header and "cuembed_grouped_mean_scale(" in header
    assert hasattr(torch.ops.cuembed_pyt, "cuembed_grouped_weight_grad")
    assert hasattr(torch.ops.cuembed_pyt, "cuembed_grouped_mean_scale")


def test_the_known_answer_program_is_in_both_builds(ce):
    import os
    from cuembed_amd import build
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert os.path.exists(os.path.join(root, "tests", "cpp", "grouped_train_kat.hip"))
    assert callable(build.build_grouped_train_test)
    with open(os.path.join(root, "CMakeLists.txt")) as f:
        assert "tests/cpp/grouped_train_kat.hip" in f.read()
    with open(os.path.join(root, "__graft_entry__.py")) as f:
        assert "build_grouped_train_test" in f.read()


def test_argument_errors_come_before_any_device_check(ce, pyt):
    """Everything below runs on CPU tensors: a device check would raise RuntimeError("... no CPU fallback ...")."""
    tables = cpu_tables()
    group = ce.TableGroup(tables)
    ids, off, grad_y = problem()
    qgroup = ce.TableGroup([torch.zeros(rows, 16, dtype=torch.uint8) for rows in C.ROWS])
    # ---- the weight gradient
    with pytest.raises(TypeError, match="8-bit"):
        ce.embedding_weight_grad_grouped(qgroup, grad_y, ids, off)
    with pytest.raises(ValueError, match="grad_y"):
        ce.embedding_weight_grad_grouped(group, grad_y[:, :2].contiguous(), ids, off)
    with pytest.raises(ValueError, match="grad_y"):
        ce.embedding_weight_grad_grouped(group, grad_y.view(15, 8), ids, off)
    with pytest.raises(ValueError, match="contiguous"):
        ce.embedding_weight_grad_grouped(group, torch.zeros(3, 5, 8).transpose(0, 1), ids, off)
    with pytest.raises(TypeError, match="grad_y"):
        ce.embedding_weight_grad_grouped(group, grad_y.half(), ids, off)
    with pytest.raises(ValueError):
        ce.embedding_weight_grad_grouped(group, grad_y, ids, off[:-1])
    with pytest.raises(ValueError):
        ce.embedding_weight_grad_grouped(group, grad_y, ids, off, num_hots=3)
    with pytest.raises(TypeError):
        ce.embedding_weight_grad_grouped(group, grad_y, ids.float(), off)
    with pytest.raises(ValueError, match="out"):
        ce.embedding_weight_grad_grouped(group, grad_y, ids, off, out=torch.zeros(ids.numel() + 1))
    with pytest.raises(ValueError, match="out"):
        ce.embedding_weight_grad_grouped(group, grad_y, ids, off, out=torch.zeros(ids.numel(), dtype=torch.float16))
    with pytest.raises(TypeError, match="out"):
        ce.embedding_weight_grad_grouped(group, grad_y, ids, off, out=[0.0] * ids.numel())
    # ---- the mode of the functional backward
    for bad in ("max", "concat", None, 0):
        with pytest.raises(ValueError, match="mode"):
            ce.embedding_backward_grouped(group, grad_y, ids, off, mode=bad)
    with pytest.raises(ValueError, match="reference_sums"):
        ce.embedding_backward_grouped(group, grad_y, ids, off, reference_sums=True, mode="mean")
    with pytest.raises(TypeError, match="8-bit"):
        ce.embedding_backward_grouped(qgroup, grad_y, ids, off, mode="mean")
    # ---- the scale
    with pytest.raises(TypeError, match="8-bit"):
        ce.grouped_mean_scale(qgroup, grad_y, off)
    with pytest.raises(ValueError, match="grad_y"):
        ce.grouped_mean_scale(group, grad_y.view(15, 8), off)
    with pytest.raises(TypeError, match="grad_y"):
        ce.grouped_mean_scale(group, grad_y.half(), off)
    with pytest.raises(ValueError):
        ce.grouped_mean_scale(group, grad_y, off[:-1])
    with pytest.raises(ValueError):
        ce.grouped_mean_scale(group, grad_y)
    with pytest.raises(TypeError, match="weights"):
        ce.grouped_mean_scale(group, grad_y, off, weights=torch.zeros(ids.numel(), dtype=torch.float16))
    with pytest.raises(ValueError, match="weights"):
        ce.grouped_mean_scale(group, grad_y, None, weights=torch.zeros(7), num_hots=2)
    with pytest.raises(ValueError, match="out"):
        ce.grouped_mean_scale(group, grad_y, off, out=torch.zeros(5, 3, 4))
    # ---- the autograd surface
    needs_grad = [t.clone().requires_grad_(True) for t in tables]
    weights = torch.ones(ids.numel(), requires_grad=True)
    for bad in ("max", "concat", None):
        with pytest.raises(ValueError, match="mode"):
            pyt.cuemb_embedding_grouped_trainable(ce.TableGroup(needs_grad), ids, off, mode=bad)
        with pytest.raises(ValueError, match="mode"):
            pyt.TrainableEmbeddingBagGroup(ce.TableGroup(needs_grad), mode=bad)
    with pytest.raises(ValueError, match="weight_grad"):
        pyt.cuemb_embedding_grouped_trainable(ce.TableGroup(needs_grad), ids, off, weight_grad="yes")
    with pytest.raises(ValueError, match="weighted mean"):
        pyt.cuemb_embedding_grouped_trainable(ce.TableGroup(needs_grad), ids, off, weights, mode="mean", weight_grad=True)
    with pytest.raises(ValueError, match="weighted mean"):      # ... also when no table requires grad
        pyt.cuemb_embedding_grouped_trainable(group, ids, off, weights, mode="mean", weight_grad=True)
    with pytest.raises(ValueError, match="padded"):
        pyt.cuemb_embedding_grouped_trainable(ce.TableGroup(needs_grad), ids, off, sparse_grad="padded", mode="mean")
    with pytest.raises(TypeError, match="8-bit"):
        pyt.cuemb_embedding_grouped_trainable(qgroup, ids, off, mode="mean")
    # ---- ... and a call that is in order reaches the device check
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ce.embedding_weight_grad_grouped(group, grad_y, ids, off)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ce.embedding_weight_grad_grouped(group, grad_y, ids, off, out=torch.zeros(ids.numel()))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ce.embedding_backward_grouped(group, grad_y, ids, off, mode="mean")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ce.embedding_backward_grouped(group, grad_y, ids, off, mode="sum")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ce.grouped_mean_scale(group, grad_y, off)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ce.grouped_mean_scale(group, grad_y, None, num_hots=2, out=grad_y)


def test_the_default_weight_gradient_error_is_unchanged(ce, pyt):
    needs_grad = [t.clone().requires_grad_(True) for t in cpu_tables()]
    ids, off, _ = problem()
    weights = torch.ones(ids.numel(), requires_grad=True)
    with pytest.raises(ValueError, match="weight gradient") as e:
        pyt.cuemb_embedding_grouped_trainable(ce.TableGroup(needs_grad), ids, off, weights)
    assert "weight_grad=True" in str(e.value)
    with pytest.raises(ValueError, match="weight gradient"):
        pyt.cuemb_embedding_grouped_trainable(ce.TableGroup(needs_grad), ids, off, weights, mode="mean")
    with pytest.raises(ValueError, match="weight gradient"):
        pyt.TrainableEmbeddingBagGroup(ce.TableGroup(needs_grad))(ids, off, weights)


def test_the_module_stores_mode_and_weight_grad(ce, pyt):
    param = torch.nn.Parameter(torch.zeros(sum(C.ROWS), 8))
    group = ce.TableGroup.from_flat(param, C.ROWS)
    bags = pyt.TrainableEmbeddingBagGroup(group)
    assert bags.mode == "sum" and bags.weight_grad is False and bags.sparse_grad is False
    bags = pyt.TrainableEmbeddingBagGroup(group, sparse_grad="padded", mode="mean", weight_grad=True)
    assert bags.mode == "mean" and bags.weight_grad is True and bags.sparse_grad == "padded"
    assert [p is param for p in bags.parameters()] == [True]


def test_fake_implementations_give_shape_and_dtype(pyt):
    from torch._subclasses.fake_tensor import FakeTensorMode
    T, batch, width = 3, 5, 8
    with FakeTensorMode():
        for dtype in (torch.float32, torch.float16, torch.bfloat16):
            tables = [torch.empty((rows, width), dtype=dtype) for rows in C.ROWS]
            ptrs = torch.empty((T,), dtype=torch.int64)
            y_grad = torch.empty((batch, T, width), dtype=dtype)
            off = torch.empty((T * batch + 1,), dtype=torch.int64)
            for idx, o, hot in ((torch.empty((40,), dtype=torch.int64), off, 0),
                                (torch.empty((T, batch, 7), dtype=torch.int32), None, 7)):
                g = torch.ops.cuembed_pyt.cuembed_grouped_weight_grad(tables, ptrs, idx, o, y_grad)
                assert g.shape == idx.shape and g.dtype == dtype
                for w in (None, torch.empty((idx.numel(),), dtype=dtype)):
                    s = torch.ops.cuembed_pyt.cuembed_grouped_mean_scale(y_grad, o, w, T, hot)
                    assert s.shape == y_grad.shape and s.dtype == dtype


# ---- the numpy model against fp64, by hand-sized cases -------------------------------------------------------------------
def test_the_mean_factor_of_the_model():
    # T = 2, B = 3: bags (t, b) of lengths [[2, 0, 1], [3, 4, 0]]
    offsets = np.array([0, 2, 2, 3, 6, 10, 10])
    f = R.mean_factor(2, 3, offsets, 0)
    assert f.dtype == np.float32 and f.shape == (3, 2)
    want = np.array([[1 / 2, 1 / 3], [0.0, 1 / 4], [1.0, 0.0]])
    assert np.array_equal(f, want.astype(np.float32))
    assert np.array_equal(R.mean_factor(2, 3, None, 4), np.full((3, 2), 0.25, dtype=np.float32))
    assert np.array_equal(R.mean_factor64(2, 3, offsets, 0), want)
    w = np.array([0.5, 0.25, 0.5, 0.25, 0.25, 0.5, 0.5, -0.5, 0.25, -0.25], dtype=np.float32)
    f = R.mean_factor(2, 3, offsets, 0, w)
    sums = np.array([[0.75, 1.0], [0.0, 0.0], [0.5, 0.0]])      # bag (1, 1): 0.5 - 0.5 + 0.25 - 0.25 = 0 -> factor 0
    want = np.where(sums == 0, 0.0, 1.0 / np.where(sums == 0, 1.0, sums))
    assert np.array_equal(f, want.astype(np.float32))
    assert np.array_equal(R.mean_factor64(2, 3, offsets, 0, w), want)
    # fixed hotness, weighted
    f = R.mean_factor(1, 2, None, 2, np.array([0.5, 0.25, 1.0, 3.0], dtype=np.float32))
    assert np.array_equal(f, np.array([[1 / 0.75], [0.25]], dtype=np.float32))


@pytest.mark.parametrize("kind", ["f32", "f16", "bf16"])
def test_the_scaled_rows_of_the_model_against_fp64(kind):
    rng = np.random.default_rng(11)
    T, B, W = 2, 4, 6
    lengths = np.array([[3, 0, 7, 300], [1, 9, 33, 64]])
    offsets = np.concatenate([[0], np.cumsum(lengths.reshape(-1))])
    g = X.round_to(kind, rng.uniform(-1, 1, (B, T, W)))
    w = X.round_to(kind, C.weights_for(rng, int(offsets[-1])))
    for weights in (None, w):
        got = R.mean_scale(kind, g, R.mean_factor(T, B, offsets, 0, weights))
        assert got.dtype == np.float32 and np.array_equal(got, X.round_to(kind, got))
        exact = g.astype(np.float64) * R.mean_factor64(T, B, offsets, 0, weights)[:, :, None]
        bound = R.mean_scale_bound(kind, exact, lengths.T)
        assert np.all(np.abs(got - exact) <= bound)
        assert np.all(got[1, 0] == 0)                                   # the empty bag (t = 0, b = 1)
        assert np.any(np.abs(got - exact) > 0) or kind == "f32"         # ... and the bound is not vacuous:
        assert np.all(bound <= (2.0 * X.EPS[kind] + 302 * 2.0 ** -24) * np.abs(exact) + X.SPACING[kind])
    # one multiply, one rounding: the unweighted factor of a power-of-two length is exact, and so is the product
    lengths = np.full((T, B), 8)
    got = R.mean_scale(kind, g, R.mean_factor(T, B, None, 8))
    assert np.array_equal(got.astype(np.float64), g.astype(np.float64) / 8.0)


def test_the_weight_gradient_of_the_model():
    tables = [np.array([[1.0, 2.0], [3.0, 4.0]]), np.array([[10.0, 20.0]])]
    # T = 2, B = 2; bags: (0,0) = [1, 0], (0,1) = [], (1,0) = [0], (1,1) = [0, 0]
    offsets = np.array([0, 2, 2, 3, 5])
    ids = np.array([1, 0, 0, 0, 0])
    gy = np.arange(8, dtype=np.float64).reshape(2, 2, 2)               # gy[b, t] = [4 b + 2 t, 4 b + 2 t + 1]
    exact, scale = R.weight_grad64(tables, 2, ids, offsets, 0, gy)
    want = [3 * 0 + 4 * 1, 1 * 0 + 2 * 1, 10 * 2 + 20 * 3, 10 * 6 + 20 * 7, 10 * 6 + 20 * 7]
    assert exact.tolist() == want and scale.tolist() == want
    t, b = R.lookup_bags(2, 2, offsets, 0)
    assert t.tolist() == [0, 0, 1, 1, 1] and b.tolist() == [0, 0, 0, 1, 1]
    # fixed hotness: [T, B, H]
    exact, _ = R.weight_grad64(tables, 2, np.array([0, 1, 1, 1, 0, 0, 0, 0]), None, 2, gy)
    assert exact.tolist() == [1 * 0 + 2 * 1, 4, 3 * 4 + 4 * 5, 32, 80, 80, 200, 200]
