"""cuemb_embedding_grouped_trainable: the gradient of a group through autograd equals the gradients of num_tables
cuemb_embedding calls stacked (exact data, torch.equal) for every gradient form of a one-storage group and of separate
tensors; one "padded" step is captured into a HIP graph and replayed; the two new ops trace with fake tensors."""
import numpy as np
import pytest
import torch

import grouped_backward_cases as G
import grouped_cases as C

pytestmark = pytest.mark.gpu

WIDTH = 64
T = len(C.ROWS)
TOTAL = sum(C.ROWS)
BASE = [0, 5000, 5017, 5317]


@pytest.fixture(scope="module")
def ce():
    import cuembed_amd
    assert torch.cuda.is_available()
    return cuembed_amd


@pytest.fixture(scope="module")
def pyt():
    from cuembed_amd import cuembed_pyt
    return cuembed_pyt


def values(dtype):
    return [torch.from_numpy(C.table_values(t, rows, WIDTH)).cuda().to(dtype) for t, rows in enumerate(C.ROWS)]


def stacked_reference(pyt, tables, batch, ids, offsets, hot, w_d, c):
    """out and the dense per-table gradients of sum(out * c) from num_tables cuemb_embedding calls stacked on dim 1."""
    params = [t.clone().requires_grad_(True) for t in tables]
    outs = []
    for t in range(T):
        i_t, o_t, w_t = G.table_problem(t, batch, ids, offsets, hot, w_d, index_dtype=np.int64)
        if o_t is None:
            o_t = torch.arange(0, batch * hot + 1, hot, dtype=torch.int64, device="cuda")
        outs.append(pyt.cuemb_embedding(params[t], i_t, o_t, w_t))
    out = torch.stack(outs, dim=1)
    (out * c).sum().backward()
    return out.detach(), [torch.zeros_like(p) if p.grad is None else p.grad for p in params]


def problems(batch, dtype, seed):
    for k, (name, ids, offsets, hot, _) in enumerate(C.layouts(batch)):
        rng = np.random.default_rng(seed + k)
        c = G.dev(rng.integers(-4, 5, (batch, T, WIDTH)).astype(np.float32)).to(dtype)
        w_d = G.dev(G.exact_weights(rng, ids.size)).to(dtype)
        idx = G.dev(ids) if offsets is not None else G.dev(ids).view(T, batch, hot)
        yield name, ids, offsets, hot, idx, G.dev(offsets), w_d, c


@pytest.mark.parametrize("batch", [5, 1023])
@pytest.mark.parametrize("kind", ["f32", "f16"])
def test_one_storage_group_every_gradient_form(ce, pyt, kind, batch):
    dtype = G.DTYPES[kind]
    tables = values(dtype)
    for name, ids, offsets, hot, idx, off, w_d, c in problems(batch, dtype, 100 * batch):
        for weights in (None, w_d):
            want_out, want_grads = stacked_reference(pyt, tables, batch, ids, offsets, hot, weights, c)
            want = torch.cat(want_grads)
            distinct = np.unique(G.global_problem(C.ROWS, batch, ids, offsets, hot)[0]).size
            for sparse_grad in (False, True, "padded"):
                flat = torch.nn.Parameter(torch.cat(tables))
                group = ce.TableGroup.from_flat(flat, C.ROWS)
                out = pyt.cuemb_embedding_grouped_trainable(group, idx, off, weights, sparse_grad=sparse_grad)
                assert out.requires_grad and torch.equal(out.detach(), want_out), (name, sparse_grad)
                loss = (out * c).sum()
                if sparse_grad is True:       # the gradient as the backward returns it (accumulation into .grad drops
                    direct, = torch.autograd.grad(loss, [flat], retain_graph=True)     # the is_coalesced flag)
                    assert direct.is_coalesced() and direct._nnz() == distinct, (name, direct._nnz(), distinct)
                loss.backward()
                grad = flat.grad
                assert tuple(grad.shape) == (TOTAL, WIDTH) and grad.dtype == dtype
                if sparse_grad is False:
                    assert grad.layout == torch.strided
                    dense = grad
                else:
                    assert grad.layout == torch.sparse_coo
                    if sparse_grad is True:
                        assert grad._nnz() == distinct, (name, grad._nnz(), distinct)
                        assert bool((grad._indices()[0][1:] > grad._indices()[0][:-1]).all())
                    else:
                        assert grad._nnz() == min(ids.size, TOTAL)
                    dense = grad.to_dense()
                assert torch.equal(dense, want), (name, sparse_grad, weights is not None)


@pytest.mark.parametrize("batch", [5, 1023])
def test_separate_tensors_only_the_tables_that_require_grad(ce, pyt, batch):
    dtype = torch.float32
    tables = values(dtype)
    for name, ids, offsets, hot, idx, off, w_d, c in problems(batch, dtype, 7 * batch):
        want_out, want_grads = stacked_reference(pyt, tables, batch, ids, offsets, hot, w_d, c)
        keys = G.global_problem(C.ROWS, batch, ids, offsets, hot)[0]
        for sparse_grad in (False, True):
            params = [t.clone() for t in tables]
            params[0].requires_grad_(True)
            params[2].requires_grad_(True)
            group = ce.TableGroup(params)
            assert group.flat is None
            out = pyt.cuemb_embedding_grouped_trainable(group, idx, off, w_d, sparse_grad=sparse_grad)
            assert torch.equal(out.detach(), want_out), name
            loss = (out * c).sum()
            if sparse_grad:                   # as the backward returns them (accumulation drops the is_coalesced flag)
                direct = torch.autograd.grad(loss, [params[0], params[2]], retain_graph=True)
                assert all(d.layout == torch.sparse_coo and d.is_coalesced() for d in direct)
            loss.backward()
            assert params[1].grad is None
            for t in (0, 2):
                grad = params[t].grad
                assert tuple(grad.shape) == (C.ROWS[t], WIDTH)
                if sparse_grad:
                    assert grad.layout == torch.sparse_coo
                    assert grad._nnz() == np.unique(keys[(keys >= BASE[t]) & (keys < BASE[t + 1])]).size
                    assert bool((grad._indices()[0][1:] > grad._indices()[0][:-1]).all())
                    grad = grad.to_dense()
                assert torch.equal(grad, want_grads[t]), (name, t, sparse_grad)


def test_without_grad_the_call_is_the_forward(ce, pyt):
    tables = values(torch.float16)
    name, ids, offsets, hot, _ = C.layouts(5)[3]
    group = ce.TableGroup.from_flat(torch.nn.Parameter(torch.cat(tables)), C.ROWS)
    want = ce.embedding_forward_grouped(tables, G.dev(ids), G.dev(offsets))
    with torch.no_grad():
        out = pyt.cuemb_embedding_grouped_trainable(group, G.dev(ids), G.dev(offsets))
    assert not out.requires_grad and torch.equal(out, want)
    frozen = ce.TableGroup(tables)
    out = pyt.cuemb_embedding_grouped_trainable(frozen, G.dev(ids), G.dev(offsets), sparse_grad=True)
    assert not out.requires_grad and torch.equal(out, want)


def test_the_module_trains_its_flat_parameter(ce, pyt):
    tables = values(torch.float32)
    name, ids, offsets, hot, idx, off, w_d, c = list(problems(5, torch.float32, 3))[0]
    assert offsets is None
    _, want_grads = stacked_reference(pyt, tables, 5, ids, offsets, hot, None, c)
    flat = torch.nn.Parameter(torch.cat(tables))
    bags = pyt.TrainableEmbeddingBagGroup(ce.TableGroup.from_flat(flat, C.ROWS), sparse_grad=True)
    assert list(bags.parameters())[0] is flat
    (bags(idx) * c).sum().backward()
    assert torch.equal(flat.grad.to_dense(), torch.cat(want_grads))
    opt = torch.optim.SGD(bags.parameters(), lr=0.5)
    before = flat.detach().clone()
    opt.step()
    assert torch.equal(flat.detach(), before - 0.5 * torch.cat(want_grads))


def test_a_padded_step_under_hip_graph_capture(ce, pyt):
    """One linear stream, no parallel branches: forward + backward of a one-storage group with sparse_grad="padded"
    (nothing is read back) captured once at B = 5; the indices are rewritten in place between replays and the replayed
    gradient has the eager bits."""
    batch, dtype = 5, torch.float16
    tables = values(dtype)
    lengths = np.full((T, batch), 9)
    offsets = G.dev(np.concatenate([[0], np.cumsum(lengths.reshape(-1))]))
    idx = G.dev(C.draw_ids(np.random.default_rng(3), C.ROWS, lengths))
    c = G.dev(np.random.default_rng(4).integers(-4, 5, (batch, T, WIDTH)).astype(np.float32)).to(dtype)
    flat = torch.nn.Parameter(torch.cat(tables))
    group = ce.TableGroup.from_flat(flat, C.ROWS)
    group.row_base_device                                    # built before the capture
    static = {}

    def step():
        flat.grad = None
        out = pyt.cuemb_embedding_grouped_trainable(group, idx, offsets, sparse_grad="padded")
        (out * c).sum().backward()
        static["out"], static["grad"] = out.detach(), flat.grad

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()                                               # warm-up outside capture (library / module loading)
        torch.cuda.current_stream().synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            step()
    for seed in (5, 6):
        idx.copy_(G.dev(C.draw_ids(np.random.default_rng(seed), C.ROWS, lengths)))
        g.replay()
        torch.cuda.synchronize()
        eager_flat = torch.nn.Parameter(torch.cat(tables))
        eager_group = ce.TableGroup.from_flat(eager_flat, C.ROWS)
        out = pyt.cuemb_embedding_grouped_trainable(eager_group, idx, offsets, sparse_grad="padded")
        (out * c).sum().backward()
        assert torch.equal(static["out"], out.detach()), seed
        assert torch.equal(static["grad"].to_dense(), eager_flat.grad.to_dense()), seed
        assert torch.equal(static["grad"]._indices(), eager_flat.grad._indices()), seed


def test_fake_implementations_give_shape_and_dtype(pyt):
    from torch._subclasses.fake_tensor import FakeTensorMode
    batch = 5
    with FakeTensorMode():
        base = torch.empty((T + 1,), dtype=torch.int64, device="cuda")
        off = torch.empty((T * batch + 1,), dtype=torch.int64, device="cuda")
        for idx, o, hot in ((torch.empty((40,), dtype=torch.int64, device="cuda"), off, 0),
                            (torch.empty((T, batch, 7), dtype=torch.int32, device="cuda"), None, 7)):
            for narrow, want in ((True, torch.int32), (False, torch.int64)):
                keys, sids = torch.ops.cuembed_pyt.cuembed_grouped_backward_keys(idx, o, base, T, batch, hot, narrow)
                for r in (keys, sids):
                    assert tuple(r.shape) == (idx.numel(),) and r.dtype == want and r.device.type == "cuda"
        ids = torch.empty((33,), dtype=torch.int32, device="cuda")
        word = torch.empty((1,), dtype=torch.int32, device="cuda")
        for args in ((ids, word, base), (ids, word, base, True)):
            cuts = torch.ops.cuembed_pyt.cuembed_grouped_table_cuts(*args)
            assert tuple(cuts.shape) == (T + 1,) and cuts.dtype == torch.int64 and cuts.device.type == "cuda"
