"""Mean pooling on a trained group, and the weight gradient through autograd.

    scale kernel   grouped_mean_scale against the numpy model (grouped_train_reference): bit for bit unweighted on
                   arbitrary data and weighted on weights whose partial sums are exact; arbitrary positive weights
                   against fp64 within the bound of one fp32 sum, one reciprocal, one product and one rounding; bags
                   that are empty or whose weights sum to 0 give zeros; in place and out of place;
    functional     embedding_backward_grouped(mode="mean") = embedding_backward_grouped(mode="sum") on the model's
                   scaled grad_y, bit for bit: dense, compressed, reference_sums;
    autograd       mode="mean" against torch.nn.functional.embedding_bag(mode="mean") per table on fp64 CPU copies, every
                   sparse_grad form; weight_grad=True gives the functional weight gradient's bits, also when no table
                   requires grad; the module trains with mode="mean"; one padded mean step is captured and replayed.
"""
import numpy as np
import pytest
import torch

import exact_sums as X
import grouped_backward_cases as G
import grouped_cases as C
import grouped_train_reference as R

pytestmark = pytest.mark.gpu

T = len(C.ROWS)
TOTAL = sum(C.ROWS)
BASE = [0, 5000, 5017, 5317]
WIDTH = 64


@pytest.fixture(scope="module")
def ce():
    import cuembed_amd
    assert torch.cuda.is_available()
    return cuembed_amd


@pytest.fixture(scope="module")
def pyt():
    from cuembed_amd import cuembed_pyt
    return cuembed_pyt


def ibits(t):
    t = t.contiguous()
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()]).view(-1)


def values(dtype, width=WIDTH):
    return [torch.from_numpy(C.table_values(t, rows, width)).cuda().to(dtype) for t, rows in enumerate(C.ROWS)]


def of_kind(kind, a32):
    """fp32 values -> (the same values rounded to `kind` as fp32, the device tensor of `kind`)."""
    r = X.round_to(kind, a32)
    return r, G.dev(r).to(G.DTYPES[kind])


# ---- the scale kernel --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [6, 36, 64])
@pytest.mark.parametrize("kind", ["f32", "f16", "bf16"])
def test_scale_unweighted_has_the_bits_of_the_model(ce, kind, width):
    group = ce.TableGroup(values(G.DTYPES[kind], width))
    for batch in C.BATCHES:
        rng = np.random.default_rng(width + batch)
        gy32, grad_y = of_kind(kind, rng.uniform(-1.0, 1.0, (batch, T, width)))
        for name, ids, offsets, hot, _ in C.layouts(batch):
            want = G.dev(R.mean_scale(kind, gy32, R.mean_factor(T, batch, offsets, hot))).to(grad_y.dtype)
            before = grad_y.clone()
            got = ce.grouped_mean_scale(group, grad_y, G.dev(offsets), num_hots=hot)
            assert got.shape == grad_y.shape and got.dtype == grad_y.dtype and got.data_ptr() != grad_y.data_ptr()
            assert torch.equal(ibits(got), ibits(want)), (name, batch)
            assert torch.equal(ibits(grad_y), ibits(before))                  # out of place: the source is left alone
            for odt in (np.int32, np.int64):                                  # in place
                work = grad_y.clone()
                back = ce.grouped_mean_scale(group, work, None if offsets is None else G.dev(offsets.astype(odt)),
                                             num_hots=hot, out=work)
                assert back is work and torch.equal(ibits(work), ibits(want)), (name, batch, odt.__name__)


@pytest.mark.parametrize("kind", ["f32", "f16", "bf16"])
def test_scale_weighted_bits_on_exactly_summable_weights(ce, kind):
    """Weights of 0.5 and 0.25: a bag's partial sums are exact in fp32 in any order, so the factor is the model's."""
    for width in (6, 64):
        group = ce.TableGroup(values(G.DTYPES[kind], width))
        for batch in C.BATCHES:
            rng = np.random.default_rng(31 * width + batch)
            gy32, grad_y = of_kind(kind, rng.uniform(-1.0, 1.0, (batch, T, width)))
            for name, ids, offsets, hot, _ in C.layouts(batch):
                w32, w_d = of_kind(kind, G.exact_weights(rng, ids.size))
                want = G.dev(R.mean_scale(kind, gy32, R.mean_factor(T, batch, offsets, hot, w32))).to(grad_y.dtype)
                got = ce.grouped_mean_scale(group, grad_y, G.dev(offsets), w_d, num_hots=hot)
                assert torch.equal(ibits(got), ibits(want)), (name, batch, width)
                work = grad_y.clone()
                ce.grouped_mean_scale(group, work, G.dev(offsets), w_d, num_hots=hot, out=work)
                assert torch.equal(ibits(work), ibits(want)), (name, batch, width, "in place")


@pytest.mark.parametrize("kind", ["f32", "f16", "bf16"])
def test_scale_weighted_within_the_bound_of_fp64(ce, kind):
    """Arbitrary positive weights: |got - exact| <= EPS * |exact| + (len + 2) * 2^-24 * |exact| + SPACING."""
    width = 64
    group = ce.TableGroup(values(G.DTYPES[kind], width))
    for batch in (5, 1023):
        rng = np.random.default_rng(batch)
        gy32, grad_y = of_kind(kind, rng.uniform(-1.0, 1.0, (batch, T, width)))
        for name, ids, offsets, hot, w in C.layouts(batch):
            w32, w_d = of_kind(kind, w)
            assert w32.size == 0 or w32.min() > 0
            lengths = R.bag_lengths(T, batch, offsets, hot).reshape(T, batch).T
            exact = gy32.astype(np.float64) * R.mean_factor64(T, batch, offsets, hot, w32)[:, :, None]
            bound = R.mean_scale_bound(kind, exact, lengths)
            got = ce.grouped_mean_scale(group, grad_y, G.dev(offsets), w_d, num_hots=hot).double().cpu().numpy()
            err = np.abs(got - exact)
            print(name, kind, batch, "max error / bound", float((err / bound).max()))
            assert np.all(err <= bound), (name, batch, float((err - bound).max()))
            assert np.all(got[lengths == 0] == 0)


def test_scale_edges(ce):
    kind, width, batch = "f16", 64, 2
    group = ce.TableGroup(values(torch.float16, width))
    # bags g = t * 2 + b: lengths 2, 0 | 4, 1 | 0, 3;  bag 2's weights sum to 0
    offsets = G.dev(np.array([0, 2, 2, 6, 7, 7, 10]))
    w = G.dev(np.array([0.5, 0.25, 0.5, -0.5, 0.25, -0.25, 2.0, 1.0, 1.0, 2.0], dtype=np.float32)).half()
    grad_y = torch.ones((batch, T, width), dtype=torch.float16, device="cuda")
    got = ce.grouped_mean_scale(group, grad_y, offsets, w)
    want = torch.tensor([[1 / 0.75, 0.0, 0.0], [0.0, 0.5, 0.25]], dtype=torch.float32).half().cuda()      # [b, t]
    assert torch.equal(got, want[:, :, None].expand(batch, T, width))
    got = ce.grouped_mean_scale(group, grad_y, offsets)
    want = torch.tensor([[0.5, 0.25, 0.0], [0.0, 1.0, 1 / 3]], dtype=torch.float32).half().cuda()
    assert torch.equal(got, want[:, :, None].expand(batch, T, width))
    # fixed hotness, weighted: every bag sums its own H weights
    w = G.dev(np.array([1, 1, 2, 2, 0.5, -0.5, 0.25, 0.25, 4, 4, 1, 0], dtype=np.float32)).half()
    got = ce.grouped_mean_scale(group, grad_y, None, w, num_hots=2)
    want = torch.tensor([[0.5, 0.0, 0.125], [0.25, 2.0, 1.0]], dtype=torch.float32).half().cuda()
    assert torch.equal(got, want[:, :, None].expand(batch, T, width))
    # an empty batch
    empty = ce.grouped_mean_scale(group, grad_y[:0].contiguous(), torch.zeros(1, dtype=torch.int64, device="cuda"))
    assert empty.shape == (0, T, width)


# ---- the functional backward -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", C.BATCHES)
@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("kind", ["f32", "f16", "bf16"])
def test_functional_mean_is_the_sum_on_the_scaled_gradient(ce, kind, weighted, batch):
    """Arbitrary data.  reference_sums adds in lookup order: the same bits on every run, at every batch.  The default
    arithmetic combines the pieces of a run that crosses workgroups with float atomics, whose result depends on their
    arrival order once there are three or more: it is compared at B = 1 and 5, where a table row is looked up a few
    dozen times at most and a run has at most two pieces (a + b = b + a)."""
    group = ce.TableGroup(values(G.DTYPES[kind]))
    ce.capacity_overflowed(reset=True)
    for k, (name, ids, offsets, hot, _) in enumerate(C.layouts(batch)):
        rng = np.random.default_rng(17 * batch + k)
        gy32, grad_y = of_kind(kind, rng.uniform(-1.0, 1.0, (batch, T, WIDTH)))
        w32, w_d = of_kind(kind, G.exact_weights(rng, ids.size)) if weighted else (None, None)
        scaled = G.dev(R.mean_scale(kind, gy32, R.mean_factor(T, batch, offsets, hot, w32))).to(grad_y.dtype)
        ids_d, off_d = G.dev(ids), G.dev(offsets)
        before = grad_y.clone()
        for extra in (dict(), dict(reference_sums=True)) if batch <= 5 else (dict(reference_sums=True),):
            got, views = ce.embedding_backward_grouped(group, grad_y, ids_d, off_d, w_d, num_hots=hot, dense=True,
                                                       mode="mean", **extra)
            want, _ = ce.embedding_backward_grouped(group, scaled, ids_d, off_d, w_d, num_hots=hot, dense=True, **extra)
            assert torch.equal(ibits(got), ibits(want)), (name, extra)
            assert len(views) == T and views[1].data_ptr() == got[BASE[1]:].data_ptr()
        if batch > 5:
            continue
        g = ce.embedding_backward_grouped(group, grad_y, ids_d, off_d, w_d, num_hots=hot, mode="mean")
        h = ce.embedding_backward_grouped(group, scaled, ids_d, off_d, w_d, num_hots=hot, mode="sum")
        count = int(g.last_id) + 1
        assert count == int(h.last_id) + 1 and torch.equal(g.ids[:count], h.ids[:count]), name
        assert torch.equal(ibits(g.rows[:count]), ibits(h.rows[:count])), name
        assert torch.equal(ibits(grad_y), ibits(before)), name                 # the caller's grad_y is left alone
    assert not ce.capacity_overflowed()


# ---- autograd -----------------------------------------------------------------------------------------------------------
def mean_reference(tables, batch, ids, offsets, hot, c):
    """Per table, torch.nn.functional.embedding_bag(mode="mean") on fp64 CPU copies: the stacked output and the dense
    gradients of sum(out * c), and the bound ingredients of the gradient (exact_sums / fp64_sums on the terms
    c[b, t] / length)."""
    c64 = c.double().cpu()
    outs, grads = [], []
    for t in range(T):
        i_t, o_t, _ = C.table_slice(t, batch, ids, offsets, hot, np.zeros(ids.size, dtype=np.float32))
        if o_t is None:
            o_t = np.arange(0, batch * hot + 1, hot)
        p = tables[t].double().cpu().requires_grad_(True)
        out = torch.nn.functional.embedding_bag(torch.from_numpy(i_t.astype(np.int64)), p,
                                                torch.from_numpy(o_t[:-1].astype(np.int64)), mode="mean")
        (out * c64[:, t]).sum().backward()
        outs.append(out.detach())
        grads.append(p.grad)
    keys, sids = G.global_problem(C.ROWS, batch, ids, offsets, hot)
    terms = c64.numpy() * R.mean_factor64(T, batch, offsets, hot)[:, :, None]
    exact, scale, walk, run_len = G.fp64_sums(keys, sids, terms.reshape(batch * T, -1), None, TOTAL)
    want = torch.cat(grads).numpy()
    assert np.all(np.abs(exact - want) <= 1e-12 * scale)      # two fp64 sums of the same terms, in two orders
    return torch.stack(outs, dim=1).numpy(), want, scale, walk, run_len


def mean_gradient_bound(kind, exact, scale, walk, run_len):
    """exact_sums.error_bound for the scatter-add (rounded once per workgroup piece: flushes_conservative), plus what the
    scale launch adds: every term c * f is rounded to the gradient's type once before it is summed -- EPS of its
    magnitude each, EPS * scale in all at most."""
    return X.error_bound(kind, exact, scale, walk, X.flushes_conservative(run_len)) + X.EPS[kind] * scale


def check_mean_out(kind, out, want_out, tables, batch, ids, offsets, hot):
    """The forward is the grouped forward's mean: an fp32 pool rounded once (forward_split_bound covers it)."""
    lengths = R.bag_lengths(T, batch, offsets, hot).reshape(T, batch).T
    bound = X.EPS[kind] * np.abs(want_out) + (lengths[:, :, None] + 4.0) * 2.0 ** -24 * (np.abs(want_out) + 1.0) + X.SPACING[kind]
    assert np.all(np.abs(out.detach().double().cpu().numpy() - want_out) <= bound)


@pytest.mark.parametrize("batch", [5, 1023])
@pytest.mark.parametrize("kind", ["f32", "f16"])
def test_mean_on_a_one_storage_group_every_gradient_form(ce, pyt, kind, batch):
    dtype = G.DTYPES[kind]
    tables = values(dtype)
    for k, (name, ids, offsets, hot, _) in enumerate(C.layouts(batch)):
        rng = np.random.default_rng(100 * batch + k)
        c = G.dev(rng.uniform(-1.0, 1.0, (batch, T, WIDTH)).astype(np.float32)).to(dtype)
        idx = G.dev(ids) if offsets is not None else G.dev(ids).view(T, batch, hot)
        want_out, want, scale, walk, run_len = mean_reference(tables, batch, ids, offsets, hot, c)
        bound = mean_gradient_bound(kind, want, scale, walk, run_len)
        distinct = np.unique(G.global_problem(C.ROWS, batch, ids, offsets, hot)[0]).size
        for sparse_grad in (False, True, "padded"):
            flat = torch.nn.Parameter(torch.cat(tables))
            group = ce.TableGroup.from_flat(flat, C.ROWS)
            out = pyt.cuemb_embedding_grouped_trainable(group, idx, G.dev(offsets), sparse_grad=sparse_grad, mode="mean")
            assert out.requires_grad
            check_mean_out(kind, out, want_out, tables, batch, ids, offsets, hot)
            (out * c).sum().backward()
            grad = flat.grad
            if sparse_grad is False:
                assert grad.layout == torch.strided
            else:
                assert grad.layout == torch.sparse_coo
                assert grad._nnz() == (distinct if sparse_grad is True else min(ids.size, TOTAL))
                grad = grad.to_dense()
            err = np.abs(grad.double().cpu().numpy() - want)
            assert np.all(err <= bound), (name, sparse_grad, float((err - bound).max()))


@pytest.mark.parametrize("batch", [5, 1023])
def test_mean_on_separate_tensors_only_the_tables_that_require_grad(ce, pyt, batch):
    kind, dtype = "f16", torch.float16
    tables = values(dtype)
    for k, (name, ids, offsets, hot, _) in enumerate(C.layouts(batch)):
        rng = np.random.default_rng(7 * batch + k)
        c = G.dev(rng.uniform(-1.0, 1.0, (batch, T, WIDTH)).astype(np.float32)).to(dtype)
        idx = G.dev(ids) if offsets is not None else G.dev(ids).view(T, batch, hot)
        _, want, scale, walk, run_len = mean_reference(tables, batch, ids, offsets, hot, c)
        bound = mean_gradient_bound(kind, want, scale, walk, run_len)
        for sparse_grad in (False, True):
            params = [t.clone() for t in tables]
            params[0].requires_grad_(True)
            params[2].requires_grad_(True)
            group = ce.TableGroup(params)
            out = pyt.cuemb_embedding_grouped_trainable(group, idx, G.dev(offsets), sparse_grad=sparse_grad, mode="mean")
            (out * c).sum().backward()
            assert params[1].grad is None
            for t in (0, 2):
                grad = params[t].grad
                assert tuple(grad.shape) == (C.ROWS[t], WIDTH)
                grad = grad.to_dense() if sparse_grad else grad
                err = np.abs(grad.double().cpu().numpy() - want[BASE[t]:BASE[t + 1]])
                assert np.all(err <= bound[BASE[t]:BASE[t + 1]]), (name, t, sparse_grad)


@pytest.mark.parametrize("kind", ["f32", "f16", "bf16"])
def test_weight_grad_through_autograd_has_the_functional_bits(ce, pyt, kind):
    dtype = G.DTYPES[kind]
    tables = values(dtype)
    for batch in (5, 1023):
        for k, (name, ids, offsets, hot, w) in enumerate(C.layouts(batch)):
            rng = np.random.default_rng(batch + k)
            c = G.dev(rng.uniform(-1.0, 1.0, (batch, T, WIDTH)).astype(np.float32)).to(dtype)
            idx = G.dev(ids) if offsets is not None else G.dev(ids).view(T, batch, hot)
            off = G.dev(offsets)
            want = ce.embedding_weight_grad_grouped(ce.TableGroup(tables), c, idx, off, num_hots=hot)
            # the tables are trained too: their gradient is that of the call without the weight gradient
            weights = G.dev(w).to(dtype).view(idx.shape).requires_grad_(True)
            flat = torch.nn.Parameter(torch.cat(tables))
            out = pyt.cuemb_embedding_grouped_trainable(ce.TableGroup.from_flat(flat, C.ROWS), idx, off, weights,
                                                        weight_grad=True)
            (out * c).sum().backward()
            assert weights.grad.shape == weights.shape and torch.equal(ibits(weights.grad), ibits(want)), name
            plain = torch.nn.Parameter(torch.cat(tables))
            out2 = pyt.cuemb_embedding_grouped_trainable(ce.TableGroup.from_flat(plain, C.ROWS), idx, off, weights.detach())
            (out2 * c).sum().backward()
            assert torch.equal(ibits(out), ibits(out2)), name
            if batch == 5:        # (at B = 1,023 the float atomics of long runs may arrive in another order)
                assert torch.equal(ibits(flat.grad), ibits(plain.grad)), name
            # no table requires grad: the call still goes through autograd, and only the weight gradient is computed
            weights = G.dev(w).to(dtype).view(idx.shape).requires_grad_(True)
            out = pyt.cuemb_embedding_grouped_trainable(ce.TableGroup(tables), idx, off, weights, weight_grad=True)
            assert out.requires_grad and torch.equal(ibits(out), ibits(out2))
            (out * c).sum().backward()
            assert torch.equal(ibits(weights.grad), ibits(want)), name
            assert all(t.grad is None for t in tables)


def test_the_module_trains_its_flat_parameter_with_the_mean(ce, pyt):
    kind, dtype, batch = "f32", torch.float32, 5
    tables = values(dtype)
    name, ids, offsets, hot, _ = C.layouts(batch)[3]
    c = G.dev(np.random.default_rng(2).uniform(-1.0, 1.0, (batch, T, WIDTH)).astype(np.float32))
    _, want, scale, walk, run_len = mean_reference(tables, batch, ids, offsets, hot, c)
    flat = torch.nn.Parameter(torch.cat(tables))
    bags = pyt.TrainableEmbeddingBagGroup(ce.TableGroup.from_flat(flat, C.ROWS), sparse_grad=True, mode="mean")
    assert list(bags.parameters())[0] is flat
    (bags(G.dev(ids), G.dev(offsets)) * c).sum().backward()
    grad = flat.grad.to_dense()
    assert np.all(np.abs(grad.double().cpu().numpy() - want) <= mean_gradient_bound(kind, want, scale, walk, run_len))
    before = flat.detach().clone()
    torch.optim.SGD(bags.parameters(), lr=0.5).step()
    assert torch.equal(flat.detach(), before - 0.5 * grad)
    assert not torch.equal(flat.detach(), before)


def test_a_padded_mean_step_under_hip_graph_capture(ce, pyt):
    """One linear stream, no parallel branches: forward + backward of a one-storage group with mode="mean",
    weight_grad=True and sparse_grad="padded" (nothing is read back), captured once at B = 5; the indices are rewritten
    in place between the two replays and the replayed step has the eager bits."""
    batch, dtype = 5, torch.float16
    tables = values(dtype)
    lengths = np.full((T, batch), 9)
    offsets = G.dev(np.concatenate([[0], np.cumsum(lengths.reshape(-1))]))
    idx = G.dev(C.draw_ids(np.random.default_rng(3), C.ROWS, lengths))
    c = G.dev(np.random.default_rng(4).uniform(-1.0, 1.0, (batch, T, WIDTH)).astype(np.float32)).to(dtype)
    weights = G.dev(G.exact_weights(np.random.default_rng(8), idx.numel())).to(dtype)
    flat = torch.nn.Parameter(torch.cat(tables))
    group = ce.TableGroup.from_flat(flat, C.ROWS)
    group.row_base_device                                    # built before the capture
    static = {}

    def step(g, p):
        p.grad = None
        out = pyt.cuemb_embedding_grouped_trainable(g, idx, offsets, weights, sparse_grad="padded", mode="mean",
                                                    weight_grad=True)
        (out * c).sum().backward()
        return out.detach(), p.grad

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step(group, flat)                                    # warm-up outside capture (library / module loading)
        torch.cuda.current_stream().synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            static["out"], static["grad"] = step(group, flat)
    for seed in (5, 6):
        idx.copy_(G.dev(C.draw_ids(np.random.default_rng(seed), C.ROWS, lengths)))
        graph.replay()
        torch.cuda.synchronize()
        eager_flat = torch.nn.Parameter(torch.cat(tables))
        out, grad = step(ce.TableGroup.from_flat(eager_flat, C.ROWS), eager_flat)
        assert torch.equal(ibits(static["out"]), ibits(out)), seed
        assert torch.equal(ibits(static["grad"].to_dense()), ibits(grad.to_dense())), seed
        assert torch.equal(static["grad"]._indices(), grad._indices()), seed
