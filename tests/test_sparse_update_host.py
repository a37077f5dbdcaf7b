"""CPU-side checks of the sparse optimizer step: the fp64 reference against torch's own optimizers, the error bounds
against implementations that should and should not meet them, the C ABI, and the argument contract of the host layer
(every rejection raised before any launch)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import optimizer_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cuembed_amd.h")


def _problem(seed, ncat=300, width=16, n=40):
    rng = np.random.default_rng(seed)
    ids = np.sort(rng.choice(ncat, size=n, replace=False))
    return ids, rng.uniform(-1, 1, (ncat, width)), rng.uniform(-1, 1, (n, width))


@pytest.mark.parametrize("rule", ["sgd", "adagrad"])
def test_reference_agrees_with_torch_cpu_optimizers_in_fp64(rule):
    """An independent statement of the semantics: torch.optim.SGD / Adagrad on the CPU in fp64, stepping the same
    coalesced sparse gradient twice (the state carries over)."""
    ids, table, _ = _problem(1)
    lr, eps = float(np.float32(0.05)), float(np.float32(1e-8))
    p = torch.nn.Parameter(torch.from_numpy(table.copy()))
    opt = torch.optim.SGD([p], lr=lr) if rule == "sgd" else torch.optim.Adagrad([p], lr=lr, eps=eps)
    w = table.copy()
    s = None if rule == "sgd" else np.zeros_like(table)
    for step in range(2):
        g = np.random.default_rng(10 + step).uniform(-1, 1, (ids.size, table.shape[1]))
        p.grad = torch.sparse_coo_tensor(torch.from_numpy(ids).unsqueeze(0), torch.from_numpy(g), size=table.shape,
                                         is_coalesced=True)
        opt.step()
        w_new, _, s_new = R.step(rule, w[ids], g, None if s is None else s[ids], lr, eps)
        w[ids] = w_new
        if s is not None:
            s[ids] = s_new
        assert np.allclose(p.detach().numpy(), w, rtol=1e-12, atol=0)
    other = np.ones(table.shape[0], dtype=bool)
    other[ids] = False
    assert np.array_equal(p.detach().numpy()[other], table[other])
    if rule == "adagrad":
        assert np.allclose(opt.state[p]["sum"].numpy(), s, rtol=1e-12, atol=0)


def test_rowwise_reference_is_adagrad_on_the_row_mean():
    ids, table, g = _problem(2)
    s0 = np.random.default_rng(3).uniform(0, 1, ids.size)
    w_new, d, s_new = R.step("rowwise_adagrad", table[ids], g, s0, 0.1, 1e-8)
    assert np.allclose(s_new, s0 + (g ** 2).mean(axis=1), rtol=1e-15)
    assert np.allclose(w_new, table[ids] - float(np.float32(0.1)) * g / (np.sqrt(s_new)[:, None] + float(np.float32(1e-8))),
                       rtol=1e-15)
    assert np.allclose(w_new + d, table[ids], rtol=1e-15)


def _fp32_step(rule, w, g, s, lr, eps, term_dtype=np.float32):
    """The rules in plain numpy at `term_dtype` precision for the update term (fp32 = what the kernel does; fp16 = a
    kernel that forms the update in the table's type).  The row-wise sum has the shape the bound was derived for: 8
    sequential additions per lane, then a pairwise tree over the lanes.  (A fully sequential fp32 sum of 256 squares is
    NOT covered by K = 16 on every input: on fp16 gradients scaled by 2^-14 -- subnormal, i.e. integer multiples of
    2^-24, whose sums hit rounding ties -- it measured up to 34.5 * 2^-24 relative, and 12.7 .. 17.1 on the other
    draws; the lane-and-tree order stays below 2.4 everywhere.)"""
    f = np.float32
    w32, g32 = w.astype(f), g.astype(f)
    lr, eps = f(lr), f(eps)
    t = term_dtype
    if rule == "sgd":
        d = (lr.astype(t) * g32.astype(t)).astype(t)
        return (w32 - d.astype(f)).astype(f), None
    if rule == "adagrad":
        s_new = (s.astype(f) + g32 * g32).astype(f)
        denom = (np.sqrt(s_new) + eps).astype(f)
    else:
        sq = (g32 * g32).astype(f).reshape(g.shape[0], -1, 8)
        acc = np.zeros(sq.shape[:2], dtype=f)
        for e in range(8):
            acc = (acc + sq[:, :, e]).astype(f)
        while acc.shape[1] > 1:
            acc = (acc[:, : acc.shape[1] // 2] + acc[:, acc.shape[1] // 2:]).astype(f)
        s_new = (s.astype(f) + acc[:, 0] / f(g.shape[1])).astype(f)
        denom = (np.sqrt(s_new) + eps).astype(f)[:, None]
    with np.errstate(all="ignore"):      # (the fp16 variant overflows and divides 0 by 0 on small gradients)
        d = ((lr.astype(t) * g32.astype(t)).astype(t) / denom.astype(t)).astype(t)
    return (w32 - d.astype(f)).astype(f), s_new


@pytest.mark.parametrize("kind", ["f32", "f16"])
@pytest.mark.parametrize("rule", R.RULES)
def test_bounds_hold_for_fp32_math_and_catch_fp16_math(rule, kind):
    store = np.float32 if kind == "f32" else np.float16
    rng = np.random.default_rng(7)
    n, width = 64, 256
    outside = 0
    for scale in (1.0, 2.0 ** -6, 2.0 ** -14):
        w = rng.uniform(-1, 1, (n, width)).astype(store)
        g = (rng.uniform(-1, 1, (n, width)) * scale).astype(store)
        s = None if rule == "sgd" else np.zeros((n, width) if rule == "adagrad" else (n,), dtype=np.float32)
        w_new, d, s_new = R.step(rule, w.astype(np.float64), g.astype(np.float64), s, 0.05, 1e-8)
        bound = R.weight_bound(kind, w_new, w.astype(np.float64), d, R.k_for(width))
        got_w, got_s = _fp32_step(rule, w, g, s, 0.05, 1e-8)
        assert R.worst_ratio(got_w.astype(store).astype(np.float64), w_new, bound) <= 1.0
        if s is not None:
            assert R.worst_ratio(got_s.astype(np.float64), s_new, R.state_bound(s_new, R.k_for(width))) <= 1.0
        bad_w, _ = _fp32_step(rule, w, g, s, 0.05, 1e-8, term_dtype=np.float16)
        outside += int((np.abs(bad_w.astype(store).astype(np.float64) - w_new) > bound).sum())
    assert outside > 0, "an update term formed in fp16 must be visible to the bound"


# ---- C ABI ---------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_in_plain_c_and_exported():
    from cuembed_amd import build
    pre = subprocess.run(["gcc", "-E", "-P", HEADER], check=True, stdout=subprocess.PIPE, text=True).stdout
    assert re.search(r"\bcuembed_sparse_row_update\s*\(", pre)
    for name in ("CUEMBED_UPDATE_SGD", "CUEMBED_UPDATE_ADAGRAD", "CUEMBED_UPDATE_ROWWISE_ADAGRAD"):
        assert name in pre
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", HEADER], check=True)
    L = ctypes.CDLL(build.build())
    assert hasattr(L, "cuembed_sparse_row_update") and hasattr(L, "cuembed_sparse_row_update_launch_shape")
    assert "c_api_optimizer.hip" in build.UNITS


def test_launch_shapes():
    import cuembed_amd as ce
    # C4: 512-byte fp16 rows -> half a wave per entry, one slice per lane, a grid as large as the device holds
    s = ce.sparse_row_update_launch_shape(torch.float16, 256, 4194304)
    assert s == dict(lane_bytes=16, lanes_per_row=32, lanes_per_entry=32, slices_per_lane=1, grid=2048)
    assert ce.sparse_row_update_launch_shape(torch.float32, 32, 100)["grid"] == 4       # 8 lanes, 32 entries a workgroup
    assert ce.sparse_row_update_launch_shape(torch.float32, 50, 100)["lane_bytes"] == 8
    assert ce.sparse_row_update_launch_shape(torch.float16, 50, 100)["lane_bytes"] == 4
    wide = ce.sparse_row_update_launch_shape(torch.float32, 1000, 100)
    assert (wide["lanes_per_row"], wide["lanes_per_entry"], wide["slices_per_lane"]) == (250, 64, 4)
    assert ce.sparse_row_update_launch_shape(torch.float32, 2048, 100)["slices_per_lane"] == 0


# ---- argument contract (CPU tensors: every rejection comes before the device check) -----------------------------------
def _args(dtype=torch.float32, ncat=20, width=8, n=5):
    return torch.zeros((ncat, width), dtype=dtype), torch.arange(n, dtype=torch.int64), torch.zeros((n, width), dtype=dtype)


def test_sparse_row_update_rejects_misuse_before_any_launch():
    import cuembed_amd as ce
    table, ids, rows = _args()
    with pytest.raises(ValueError, match="rule"):
        ce.sparse_row_update(table, ids, rows, rule="adam", lr=0.1)
    with pytest.raises(TypeError, match="dtype"):
        ce.sparse_row_update(table, ids, rows.half(), rule="sgd", lr=0.1)
    with pytest.raises(TypeError):
        ce.sparse_row_update(table.double(), ids, rows.double(), rule="sgd", lr=0.1)
    with pytest.raises(TypeError):
        ce.sparse_row_update(table, ids.to(torch.int16), rows, rule="sgd", lr=0.1)
    with pytest.raises(ValueError, match="state"):
        ce.sparse_row_update(table, ids, rows, rule="sgd", lr=0.1, state=torch.zeros(20))
    with pytest.raises(TypeError, match="state"):
        ce.sparse_row_update(table, ids, rows, rule="adagrad", lr=0.1)
    with pytest.raises(ValueError, match="shape"):
        ce.sparse_row_update(table, ids, rows, rule="adagrad", lr=0.1, state=torch.zeros(20))
    with pytest.raises(ValueError, match="shape"):
        ce.sparse_row_update(table, ids, rows, rule="rowwise_adagrad", lr=0.1, state=torch.zeros((20, 8)))
    with pytest.raises(TypeError, match="float32"):
        ce.sparse_row_update(table, ids, rows, rule="rowwise_adagrad", lr=0.1, state=torch.zeros(20, dtype=torch.float16))
    word = torch.tensor([3], dtype=torch.int32)
    with pytest.raises(ValueError, match="at most one"):
        ce.sparse_row_update(table, ids, rows, rule="sgd", lr=0.1, count=3, last_id=word.long())
    with pytest.raises(ValueError, match="at most one"):
        ce.sparse_row_update(table, ids, rows, rule="sgd", lr=0.1, count=word, counts=word, piece_rows=5)
    with pytest.raises(ValueError, match="count"):
        ce.sparse_row_update(table, ids, rows, rule="sgd", lr=0.1, count=6)
    with pytest.raises(TypeError, match="last_id"):
        ce.sparse_row_update(table, ids, rows, rule="sgd", lr=0.1, last_id=word)            # ids are int64
    with pytest.raises(ValueError, match="piece_rows"):
        ce.sparse_row_update(table, ids, rows, rule="sgd", lr=0.1, counts=torch.tensor([1, 2]), piece_rows=2)
    with pytest.raises(ValueError):
        ce.sparse_row_update(table, ids, rows[:, :4], rule="sgd", lr=0.1)
    with pytest.raises(TypeError, match="lr"):
        ce.sparse_row_update(table, ids, rows, rule="sgd", lr=torch.tensor([0.1], dtype=torch.float64))
    with pytest.raises(RuntimeError, match="GPU"):        # everything else in order: only the device is wrong
        ce.sparse_row_update(table, ids, rows, rule="sgd", lr=0.1)


@pytest.mark.parametrize("name", ["SparseSGD", "SparseAdagrad", "RowwiseAdagrad"])
def test_optimizers_reject_dense_and_uncoalesced_gradients(name):
    from cuembed_amd import optim
    p = torch.nn.Parameter(torch.zeros((20, 8)))
    opt = getattr(optim, name)([p], lr=0.1)
    p.grad = torch.zeros((20, 8))
    with pytest.raises(ValueError, match="dense.*sparse_grad=True.*backward_and_apply"):
        opt.step()
    p.grad = torch.sparse_coo_tensor(torch.tensor([[1, 1, 3]]), torch.ones((3, 8)), size=(20, 8))
    assert not p.grad.is_coalesced()
    with pytest.raises(ValueError, match="(?s)COALESCED.*sparse_grad=True.*backward_and_apply"):
        opt.step()
    assert float(p.detach().abs().max()) == 0.0           # no silent .coalesce(): nothing was applied


def test_updater_and_optimizer_state():
    from cuembed_amd import optim
    table = torch.zeros((20, 8), dtype=torch.float16)
    with pytest.raises(ValueError, match="rule"):
        optim.SparseUpdater(table, "adam", 0.1)
    with pytest.raises(TypeError):
        optim.SparseUpdater(table.double(), "sgd", 0.1)
    assert optim.SparseUpdater(table, "sgd", 0.1).state is None
    u = optim.SparseUpdater(table, "adagrad", 0.1, initial_accumulator_value=0.5)
    assert u.state.shape == (20, 8) and u.state.dtype == torch.float32 and float(u.state.min()) == 0.5
    assert optim.SparseUpdater(table, "rowwise_adagrad", 0.1).state.shape == (20,)
    with pytest.raises(TypeError, match="dtype"):
        u.backward_and_apply(torch.zeros((4, 8)), torch.zeros((4, 2), dtype=torch.int32))
    # state_dict round trip keeps the fp32 accumulator of a 16-bit table exactly
    p = torch.nn.Parameter(table.clone())
    a = optim.RowwiseAdagrad([p], lr=0.1, initial_accumulator_value=1.0 + 2.0 ** -20)
    b = optim.RowwiseAdagrad([p], lr=0.3)
    b.load_state_dict(a.state_dict())
    assert b.state[p]["sum"].dtype == torch.float32 and torch.equal(b.state[p]["sum"], a.state[p]["sum"])
    assert b.param_groups[0]["lr"] == 0.1
    assert b.state[p]["sum"].data_ptr() != a.state[p]["sum"].data_ptr()
