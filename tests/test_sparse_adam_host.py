"""CPU-side checks of the sparse Adam step: the fp64 reference against torch.optim.SparseAdam, the error bounds against
implementations that should and should not meet them, the C ABI, the argument contract of the host layer (every
rejection raised before any launch), the bias-factor helper and the optimizers' state dicts."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import adam_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cuembed_amd.h")


# ---- the reference is torch.optim.SparseAdam's formula ----------------------------------------------------------------
def test_reference_agrees_with_torch_sparse_adam_in_fp64():
    """torch.optim.SparseAdam on the CPU in fp64, three steps, rows named in only some of them (their moments must not
    decay in between).  Every element agrees to 1e-12 relative: the second moment (a sum of positive terms) relative to
    itself; the first moment and the weight, which are differences and can cancel (at this seed one weight lands within
    1e-3 of zero and two correct fp64 evaluations differ by 1.3e-12 of IT), relative to the terms they are made of,
    |beta1 m| + |(1 - beta1) g| and |w| + |update| (torch forms the moment as m + (1 - beta1) (g - m))."""
    rng = np.random.default_rng(1)
    ncat, width = 300, 16
    table = rng.uniform(-1, 1, (ncat, width))
    betas, lr, eps = (0.9, 0.999), float(np.float32(0.05)), float(np.float32(1e-8))
    p = torch.nn.Parameter(torch.from_numpy(table.copy()))
    opt = torch.optim.SparseAdam([p], lr=lr, betas=betas, eps=eps)
    w, m, v = table.copy(), np.zeros_like(table), np.zeros_like(table)
    terms, operands = np.zeros_like(table), np.abs(table)
    named_in = []
    for t in (1, 2, 3):
        ids = np.sort(rng.choice(ncat, size=40 + 10 * t, replace=False))
        named_in.append(set(ids.tolist()))
        g = rng.uniform(-1, 1, (ids.size, width))
        p.grad = torch.sparse_coo_tensor(torch.from_numpy(ids).unsqueeze(0), torch.from_numpy(g), size=table.shape,
                                         is_coalesced=True)
        opt.step()
        sc = dict(beta1=betas[0], omb1=1.0 - betas[0], beta2=betas[1], omb2=1.0 - betas[1], eps=eps,
                  step=lr * R.bias_factor(t, betas), decay=0.0)
        r = R.step("adam", w[ids], g, m[ids], v[ids], sc)
        w_before = w.copy()
        w[ids], m[ids], v[ids] = r["w"], r["m"], r["v"]
        terms[ids] = r["m_terms"]             # (a row that is not named keeps the scale of its last step: so does its error)
        operands[ids] = np.abs(w_before[ids]) + np.abs(w_before[ids] - r["w"])
        assert np.all(np.abs(p.detach().numpy() - w) <= 1e-12 * operands)
        assert np.all(np.abs(opt.state[p]["exp_avg_sq"].numpy() - v) <= 1e-12 * np.abs(v))
        assert np.all(np.abs(opt.state[p]["exp_avg"].numpy() - m) <= 1e-12 * terms)
    some = named_in[0] ^ named_in[2]
    assert some and (named_in[0] - named_in[1])           # rows named in only some steps exist
    never = np.array(sorted(set(range(ncat)) - named_in[0] - named_in[1] - named_in[2]))
    assert never.size and np.array_equal(p.detach().numpy()[never], table[never])
    assert not opt.state[p]["exp_avg"].numpy()[never].any()


def test_rowwise_reference_is_adam_on_the_row_mean():
    rng = np.random.default_rng(2)
    w, g, m = rng.uniform(-1, 1, (3, 20, 8))
    v = rng.uniform(0, 1, 20)
    sc = R.scalars(0.1, R.bias_factor(4), (0.9, 0.999), 1e-8, 0.01)
    r = R.step("rowwise_adam", w, g, m, v, sc)
    assert np.allclose(r["v"], sc["beta2"] * v + sc["omb2"] * (g ** 2).mean(axis=1), rtol=1e-15)
    assert np.allclose(r["m"], sc["beta1"] * m + sc["omb1"] * g, rtol=1e-13)
    want = w - sc["decay"] * w - sc["step"] * r["m"] / (np.sqrt(r["v"])[:, None] + sc["eps"])
    assert np.allclose(r["w"], want, rtol=1e-13)
    assert sc["step"] == float(np.float32(np.float32(0.1) * np.float32(R.bias_factor(4))))
    assert sc["decay"] == float(np.float32(np.float32(0.1) * np.float32(0.01)))
    assert R.scalars(0.1)["decay"] == 0.0 and R.scalars(0.1)["omb2"] == float(np.float32(1.0 - 0.999))


# ---- the bounds accept the kernel's arithmetic and see a real error ---------------------------------------------------
def _fp32_step(rule, w, g, m, v, sc, term_dtype=np.float32):
    """The kernel's operation order in numpy, every operation rounded to fp32 (term_dtype=fp16: a kernel that forms the
    update term in the table's type).  The row-wise sum has the kernel's shape: 8 sequential additions per lane, then a
    pairwise tree over the lanes."""
    f = np.float32
    t = term_dtype
    w32, g32, m32, v32 = w.astype(f), g.astype(f), m.astype(f), v.astype(f)
    b1, omb1, b2, omb2 = f(sc["beta1"]), f(sc["omb1"]), f(sc["beta2"]), f(sc["omb2"])
    eps, step, decay = f(sc["eps"]), f(sc["step"]), f(sc["decay"])
    if sc["decay"] != 0.0:
        w32 = (w32 - (decay * w32).astype(f)).astype(f)
    m_new = ((b1 * m32).astype(f) + (omb1 * g32).astype(f)).astype(f)
    sq = (g32 * g32).astype(f)
    with np.errstate(all="ignore"):      # (the fp16 variant underflows to 0 / 0 on small gradients)
        if rule == "adam":
            v_new = ((b2 * v32).astype(f) + (omb2 * sq).astype(f)).astype(f)
            denom = (np.sqrt(v_new).astype(f) + eps).astype(f)
            d = ((step.astype(t) * m_new.astype(t)).astype(t) / denom.astype(t)).astype(t)
        else:
            lanes = sq.reshape(g.shape[0], -1, 8)
            acc = np.zeros(lanes.shape[:2], dtype=f)
            for e in range(8):
                acc = (acc + lanes[:, :, e]).astype(f)
            while acc.shape[1] > 1:
                acc = (acc[:, : acc.shape[1] // 2] + acc[:, acc.shape[1] // 2:]).astype(f)
            mean = (acc[:, 0] / f(g.shape[1])).astype(f)
            v_new = ((b2 * v32).astype(f) + (omb2 * mean).astype(f)).astype(f)
            denom = (np.sqrt(v_new).astype(f) + eps).astype(f)
            scale = (step.astype(t) / denom.astype(t)).astype(t)[:, None]
            d = (scale * m_new.astype(t)).astype(t)
    return (w32 - d.astype(f)).astype(f), m_new, v_new


def _round_to(x32, kind):
    if kind == "f32":
        return x32.astype(np.float64)
    if kind == "f16":
        with np.errstate(over="ignore"):
            return x32.astype(np.float16).astype(np.float64)
    return torch.from_numpy(np.ascontiguousarray(x32)).to(torch.bfloat16).double().numpy()


def _stored(x, kind):
    """Random fp64 data rounded to values the table's type holds."""
    return _round_to(x.astype(np.float32), kind)


@pytest.mark.parametrize("kind", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("rule", R.RULES)
def test_bounds_hold_for_fp32_math_and_catch_fp16_math(rule, kind):
    rng = np.random.default_rng(7)
    n, width = 64, 256
    k = R.k_for(width)
    for scale in (1.0, 2.0 ** -6, 2.0 ** -14):
        outside = 0
        for bias_step, wd in ((1, 0.0), (3, 0.01)):
            sc = R.scalars(0.05, R.bias_factor(bias_step), (0.9, 0.999), 1e-8, wd)
            w = _stored(rng.uniform(-1, 1, (n, width)), kind)
            g = _stored(rng.uniform(-1, 1, (n, width)) * scale, kind)
            m = (rng.uniform(-1, 1, (n, width)) * scale * (bias_step > 1)).astype(np.float32).astype(np.float64)
            v_shape = (n, width) if rule == "adam" else (n,)
            v = (rng.uniform(0, 1, v_shape) * scale * scale * (bias_step > 1)).astype(np.float32).astype(np.float64)
            r = R.step(rule, w, g, m, v, sc)
            bound = R.weight_bound(kind, r, w, k)
            got_w, got_m, got_v = _fp32_step(rule, w, g, m, v, sc)
            assert R.worst_ratio(_round_to(got_w, kind), r["w"], bound) <= 1.0
            assert R.worst_ratio(got_m.astype(np.float64), r["m"], R.exp_avg_bound(r, k)) <= 1.0
            assert R.worst_ratio(got_v.astype(np.float64), r["v"], R.exp_avg_sq_bound(r, k)) <= 1.0
            bad_w = _round_to(_fp32_step(rule, w, g, m, v, sc, term_dtype=np.float16)[0], kind)
            # only finite results count: the 0 / 0 of an fp16 term on the smallest gradients proves nothing about the bound
            outside += int((np.isfinite(bad_w) & (np.abs(bad_w - r["w"]) > bound)).sum())
            if scale == 1.0:
                assert np.isfinite(bad_w).all()
        assert outside > 0, "an update term formed in fp16 must be visible to the bound at gradient scale %g" % scale


# ---- C ABI ---------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_in_plain_c_and_exported():
    from cuembed_amd import build
    pre = subprocess.run(["gcc", "-E", "-P", HEADER], check=True, stdout=subprocess.PIPE, text=True).stdout
    for name in ("cuembed_sparse_row_adam", "cuembed_sparse_row_adam_stochastic", "cuembed_adam_clock_advance"):
        assert re.search(r"\b%s\s*\(" % name, pre), name
    for name in ("CUEMBED_ADAM", "CUEMBED_ROWWISE_ADAM"):
        assert re.search(r"\b%s\b" % name, pre), name
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", HEADER], check=True)
    L = ctypes.CDLL(build.build())
    for name in ("cuembed_sparse_row_adam", "cuembed_sparse_row_adam_stochastic", "cuembed_adam_clock_advance"):
        assert hasattr(L, name), name
    assert "c_api_optimizer_adam.hip" in build.UNITS


# ---- argument contract (CPU tensors: every rejection comes before the device check) -----------------------------------
def _args(dtype=torch.float32, ncat=20, width=8, n=5):
    return torch.zeros((ncat, width), dtype=dtype), torch.arange(n, dtype=torch.int64), torch.zeros((n, width), dtype=dtype)


def test_sparse_row_adam_rejects_misuse_before_any_launch():
    import cuembed_amd as ce
    table, ids, rows = _args()
    m, v, v_row = torch.zeros((20, 8)), torch.zeros((20, 8)), torch.zeros(20)

    def call(table=table, ids=ids, rows=rows, exp_avg=m, exp_avg_sq=v, lr=0.1, **kw):
        ce.sparse_row_adam(table, ids, rows, exp_avg=exp_avg, exp_avg_sq=exp_avg_sq, lr=lr, **kw)

    with pytest.raises(TypeError, match="dtype"):
        call(rows=rows.half())
    with pytest.raises(TypeError):
        call(table=table.double(), rows=rows.double())
    with pytest.raises(TypeError):
        call(ids=ids.to(torch.int16))
    # the moments, for each rule: missing, wrong dtype, wrong shape
    for rowwise, good_v, bad_v in ((False, v, v_row), (True, v_row, v)):
        with pytest.raises(TypeError, match="exp_avg"):
            call(exp_avg=None, exp_avg_sq=good_v, rowwise=rowwise)
        with pytest.raises(TypeError, match="exp_avg_sq"):
            call(exp_avg_sq=None, rowwise=rowwise)
        with pytest.raises(TypeError, match="float32"):
            call(exp_avg=m.half(), exp_avg_sq=good_v, rowwise=rowwise)
        with pytest.raises(TypeError, match="float32"):
            call(exp_avg_sq=good_v.double(), rowwise=rowwise)
        with pytest.raises(ValueError, match="shape"):
            call(exp_avg=torch.zeros(20), exp_avg_sq=good_v, rowwise=rowwise)
        with pytest.raises(ValueError, match="shape"):
            call(exp_avg_sq=bad_v, rowwise=rowwise)        # (rowwise=True with a 2-D exp_avg_sq is one of these)
        with pytest.raises(ValueError, match="shape"):
            call(exp_avg_sq=torch.zeros((19,) if rowwise else (19, 8)), rowwise=rowwise)
    for betas in ((1.0, 0.999), (0.9, 1.0), (-0.1, 0.999), (0.9, 1.5), (0.9,), None):
        with pytest.raises(ValueError, match="betas"):
            call(betas=betas)
    with pytest.raises(ValueError, match="eps"):
        call(eps=-1e-8)
    with pytest.raises(ValueError, match="weight_decay"):
        call(weight_decay=-0.01)
    word = torch.tensor([3], dtype=torch.int32)
    with pytest.raises(ValueError, match="at most one"):
        call(count=3, last_id=word.long())
    with pytest.raises(ValueError, match="at most one"):
        call(count=word, counts=word, piece_rows=5)
    with pytest.raises(ValueError, match="at most one"):
        call(last_id=word.long(), counts=word, piece_rows=5)
    with pytest.raises(ValueError, match="count"):
        call(count=6)
    with pytest.raises(TypeError, match="last_id"):
        call(last_id=word)                                  # ids are int64
    with pytest.raises(ValueError, match="piece_rows"):
        call(counts=torch.tensor([1, 2]), piece_rows=2)
    with pytest.raises(ValueError):
        call(rows=rows[:, :4])
    with pytest.raises(TypeError, match="lr"):
        call(lr=torch.tensor([0.1], dtype=torch.float64))
    with pytest.raises(TypeError, match="bias_factor"):
        call(bias_factor=torch.tensor([0.1], dtype=torch.float64))
    with pytest.raises(TypeError, match="float16 / bfloat16"):
        call(stochastic_rounding=True, seed=1)             # an fp32 table is not rounded
    h_table, _, h_rows = _args(torch.float16)
    with pytest.raises(ValueError, match="seed"):
        call(table=h_table, rows=h_rows, stochastic_rounding=True, seed=-1)
    with pytest.raises(RuntimeError, match="GPU"):        # everything else in order: only the device is wrong
        call()
    with pytest.raises(RuntimeError, match="GPU"):
        call(exp_avg_sq=v_row, rowwise=True, weight_decay=0.01, bias_factor=0.3, betas=(0.0, 0.5))
    with pytest.raises(RuntimeError, match="GPU"):
        call(table=h_table, rows=h_rows, stochastic_rounding=True, seed=5, step=2)
    # the clock's functions validate the same way
    with pytest.raises(TypeError, match="powers"):
        ce.adam_clock_advance(torch.zeros(3), torch.ones(1))
    with pytest.raises(TypeError, match="bias_factor"):
        ce.adam_clock_advance(torch.zeros(3, dtype=torch.float64), torch.ones(2))
    with pytest.raises(ValueError, match="betas"):
        ce.adam_clock_advance(torch.zeros(3, dtype=torch.float64), torch.ones(1), betas=(1.0, 0.5))
    with pytest.raises(RuntimeError, match="GPU"):
        ce.adam_clock_advance(torch.zeros(3, dtype=torch.float64), torch.ones(1))


@pytest.mark.parametrize("name", ["SparseAdam", "RowwiseAdam"])
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
    assert opt.state[p]["step"] == 0 and float(opt.state[p]["exp_avg"].abs().max()) == 0.0
    with pytest.raises(ValueError, match="betas"):
        getattr(optim, name)([p], lr=0.1, betas=(0.9, 1.0))
    with pytest.raises(ValueError):
        getattr(optim, name)([p], lr=0.1, weight_decay=-1.0)
    with pytest.raises(TypeError):
        getattr(optim, name)([p], lr=0.1, stochastic_rounding=True)       # an fp32 table


# ---- helpers and state dicts --------------------------------------------------------------------------------------------
def test_adam_bias_factor_is_the_double_formula():
    import cuembed_amd as ce
    for betas in ((0.9, 0.999), (0.5, 0.75), (0.0, 0.99)):
        for t in (1, 2, 3, 10, 1000, 100000):
            want = math.sqrt(1.0 - betas[1] ** t) / (1.0 - betas[0] ** t)
            assert ce.adam_bias_factor(t, betas) == want
    assert ce.adam_bias_factor(1, (0.5, 0.75)) == 1.0
    assert abs(ce.adam_bias_factor(10 ** 6) - 1.0) < 1e-12
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="step"):
            ce.adam_bias_factor(bad)
    with pytest.raises(ValueError, match="betas"):
        ce.adam_bias_factor(1, (0.9, 1.0))


def test_updater_owns_fp32_moments_and_a_clock():
    from cuembed_amd import optim
    table = torch.zeros((20, 8), dtype=torch.float16)
    u = optim.SparseAdamUpdater(table, 0.1)
    assert u.exp_avg.shape == (20, 8) and u.exp_avg_sq.shape == (20, 8)
    assert u.exp_avg.dtype == u.exp_avg_sq.dtype == torch.float32
    assert u.powers.dtype == torch.float64 and u.powers.tolist() == [0.0, 1.0, 1.0]
    assert u.bias_factor.dtype == torch.float32 and u.bias_factor.tolist() == [1.0]
    assert optim.SparseAdamUpdater(table, 0.1, rowwise=True).exp_avg_sq.shape == (20,)
    with pytest.raises(TypeError):
        optim.SparseAdamUpdater(table.double(), 0.1)
    with pytest.raises(ValueError, match="betas"):
        optim.SparseAdamUpdater(table, 0.1, betas=(0.9, 1.0))
    with pytest.raises(ValueError):
        optim.SparseAdamUpdater(table, 0.1, eps=-1.0)
    with pytest.raises(TypeError):
        optim.SparseAdamUpdater(table.float(), 0.1, stochastic_rounding=True)
    with pytest.raises(TypeError, match="dtype"):
        u.backward_and_apply(torch.zeros((4, 8)), torch.zeros((4, 2), dtype=torch.int32))


@pytest.mark.parametrize("name", ["SparseAdam", "RowwiseAdam"])
def test_state_dict_round_trip_keeps_the_fp32_moments_of_a_16_bit_table(name):
    from cuembed_amd import optim
    cls = getattr(optim, name)
    p = torch.nn.Parameter(torch.zeros((20, 8), dtype=torch.float16))
    a = cls([p], lr=0.1, betas=(0.8, 0.9), weight_decay=0.01)
    assert sorted(a.state[p]) == ["exp_avg", "exp_avg_sq", "step"]
    a.state[p]["exp_avg"].fill_(1.0 + 2.0 ** -20)            # not a float16 value
    a.state[p]["exp_avg_sq"].fill_(3.0 + 2.0 ** -20)
    a.state[p]["step"] = 7
    b = cls([p], lr=0.3)
    b.load_state_dict(a.state_dict())
    for key in ("exp_avg", "exp_avg_sq"):
        assert b.state[p][key].dtype == torch.float32 and torch.equal(b.state[p][key], a.state[p][key])
        assert b.state[p][key].data_ptr() != a.state[p][key].data_ptr()
    assert b.state[p]["step"] == 7 and isinstance(b.state[p]["step"], int)
    assert b.param_groups[0]["lr"] == 0.1 and tuple(b.param_groups[0]["betas"]) == (0.8, 0.9)
    assert b.param_groups[0]["weight_decay"] == 0.01


def test_state_dicts_are_exchanged_with_torch_sparse_adam():
    """The keys are torch.optim.SparseAdam's: its state dict (an fp32 table, two steps taken) loads here, and this
    optimizer's loads there and steps."""
    from cuembed_amd import optim
    torch.manual_seed(0)
    p = torch.nn.Parameter(torch.rand((20, 8)))
    t_opt = torch.optim.SparseAdam([p], lr=0.05, betas=(0.8, 0.95))
    for _ in range(2):
        p.grad = torch.sparse_coo_tensor(torch.tensor([[1, 4, 9]]), torch.rand((3, 8)), size=(20, 8), is_coalesced=True)
        t_opt.step()
    ours = optim.SparseAdam([p], lr=0.5)
    ours.load_state_dict(t_opt.state_dict())
    st = ours.state[p]
    assert st["step"] == 2 and isinstance(st["step"], int)
    assert torch.equal(st["exp_avg"], t_opt.state[p]["exp_avg"]) and st["exp_avg"].dtype == torch.float32
    assert torch.equal(st["exp_avg_sq"], t_opt.state[p]["exp_avg_sq"])
    assert float(st["exp_avg"][4].abs().min()) > 0 and float(st["exp_avg"][0].abs().max()) == 0
    assert ours.param_groups[0]["lr"] == 0.05 and tuple(ours.param_groups[0]["betas"]) == (0.8, 0.95)
    # ... and the reverse
    back = torch.optim.SparseAdam([p], lr=0.7)
    back.load_state_dict(ours.state_dict())
    assert int(back.state[p]["step"]) == 2 and torch.equal(back.state[p]["exp_avg"], st["exp_avg"])
    before = p.detach().clone()
    p.grad = torch.sparse_coo_tensor(torch.tensor([[4]]), torch.ones((1, 8)), size=(20, 8), is_coalesced=True)
    back.step()
    assert int(back.state[p]["step"]) == 3 and not torch.equal(p.detach()[4], before[4])
    fresh = optim.SparseAdam([torch.nn.Parameter(torch.rand((20, 8)))], lr=0.01, weight_decay=0.1)
    to_torch = torch.optim.SparseAdam([p], lr=0.7)
    to_torch.load_state_dict(fresh.state_dict())
    p.grad = torch.sparse_coo_tensor(torch.tensor([[2]]), torch.ones((1, 8)), size=(20, 8), is_coalesced=True)
    to_torch.step()                                         # torch's step finds every key it looks up
    assert int(to_torch.state[p]["step"]) == 1
