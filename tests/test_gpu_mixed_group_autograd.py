"""Training a mixed-width group through autograd: TrainableMixedEmbeddingBagGroup / cuemb_embedding_mixed_group_trainable
give every table a coalesced sparse gradient whose dense form equals the single-table cuemb_embedding autograd on that
table's own bags and column slice of grad_y, on exactly representable data -- sum and mean, CSR and fixed hotness.

Mean pooling multiplies grad_y by 1 / length, so the bags of the mean cases have lengths 0, 1, 8 or 64 (and hotness 1 or
8): integer grad_y times a power of two keeps every partial sum exact in fp32, and the comparison stays bit for bit
however the two routes cut a row's lookups into partial sums."""
import numpy as np
import pytest
import torch

import grouped_backward_cases as G
import grouped_cases as C
import mixed_group_backward_reference as R

pytestmark = pytest.mark.gpu

ROWS = R.ROWS
WIDTHS = (128, 16, 64, 32)
T = len(WIDTHS)
COLS = R.column_base(WIDTHS)


@pytest.fixture(scope="module")
def ce():
    import cuembed_amd
    assert torch.cuda.is_available()
    return cuembed_amd


@pytest.fixture(scope="module")
def pyt():
    from cuembed_amd import cuembed_pyt
    return cuembed_pyt


def tables_of(dtype):
    return [torch.from_numpy(C.table_values(t, ROWS[t], w)).cuda().to(dtype) for t, w in enumerate(WIDTHS)]


def power_of_two_layouts(batch):
    """[(name, ids, offsets or None, hot)] with bag lengths in {0, 1, 8, 64}: CSR, and fixed hotness 1 and 8."""
    out = []
    for hot in (1, 8):
        rng = np.random.default_rng(hot)
        out.append(("h%d" % hot, C.draw_ids(rng, ROWS, np.full((T, batch), hot)), None, hot))
    rng = np.random.default_rng(99)
    lengths = rng.choice((0, 1, 8, 64), size=(T, batch))
    offsets = np.concatenate([[0], np.cumsum(lengths.reshape(-1))]).astype(np.int64)
    out.append(("csr", C.draw_ids(rng, ROWS, lengths), offsets, 0))
    return out


def mean_scaled(grad_y32, batch, offsets, hot, weight):
    """grad_y [B, D] (numpy fp32) times each bag's mean factor, by numpy: 1 / (the bag's length times `weight`, the value
    every lookup's weight has; 1 when unweighted), 0 for an empty bag.  Independent of the library's own scale kernel."""
    lengths = np.full(T * batch, hot) if offsets is None else np.diff(offsets)
    denominator = lengths.astype(np.float64) * weight
    factor = np.where(denominator > 0, 1.0 / np.maximum(denominator, 1e-30), 0.0).reshape(T, batch)
    out = grad_y32.astype(np.float64).copy()
    for t in range(T):
        out[:, COLS[t]:COLS[t + 1]] *= factor[t][:, None]
    assert np.array_equal(out, out.astype(np.float32))          # powers of two: exact
    return out.astype(np.float32)


def single_table_grads(pyt, tables, batch, ids, offsets, hot, grad_y, weights=None):
    """The dense gradient of every table from the single-table autograd on its own bags and slice of grad_y."""
    grads = []
    for t, table in enumerate(tables):
        i_t, o_t, w_t = C.table_slice(t, batch, ids, offsets, hot, ids if weights is None else weights)
        if i_t.size == 0:                      # (a table without a lookup: nothing to differentiate)
            grads.append(torch.zeros_like(table))
            continue
        if o_t is None:
            o_t = np.arange(0, batch * hot + 1, hot)
        p = table.clone().requires_grad_(True)
        out = pyt.cuemb_embedding(p, G.dev(i_t), G.dev(o_t), None if weights is None else G.dev(w_t))
        out.backward(grad_y[:, COLS[t]:COLS[t + 1]].contiguous())
        grads.append(p.grad)
    return grads


@pytest.mark.parametrize("batch", [5, 1023])
@pytest.mark.parametrize("kind,mode,weighted", [("f32", "sum", False), ("f16", "sum", False), ("f32", "sum", True),
                                                ("f32", "mean", False), ("f32", "mean", True)])
def test_every_table_gets_the_single_table_gradient(ce, pyt, kind, mode, weighted, batch):
    """weighted: every lookup's weight is 0.5, so a weighted mean's factor stays a power of two.  The mean's reference is
    the single-table SUM autograd on grad_y scaled by numpy (mean_scaled), not by the library's scale launch."""
    dtype = G.DTYPES[kind]
    tables = tables_of(dtype)
    if mode == "sum":
        layouts = [(name, ids, offsets, hot) for name, ids, offsets, hot, _ in C.layouts(batch, rows=ROWS)]
    else:
        layouts = power_of_two_layouts(batch)
    for k, (name, ids, offsets, hot) in enumerate(layouts):
        params = [torch.nn.Parameter(t.clone()) for t in tables]
        bags = pyt.TrainableMixedEmbeddingBagGroup(params, mode=mode)
        assert bags.num_tables == T and bags.embedding_dim == sum(WIDTHS) and len(list(bags.parameters())) == T
        gy32 = R.exact_grad_y(np.random.default_rng(40 + k), batch, WIDTHS, kind)
        grad_y = G.dev(gy32).to(dtype)
        w32 = np.full(ids.size, 0.5, dtype=np.float32) if weighted else None
        w_d = None if w32 is None else G.dev(w32).to(dtype)
        ids_d, off_d = G.dev(ids), G.dev(offsets)
        idx = ids_d if offsets is not None else ids_d.view(T, batch, hot)
        out = bags(idx, off_d, w_d)
        want_out = ce.embedding_forward_mixed_group(tables, ids_d, off_d, w_d, num_hots=hot, mode=mode)
        assert torch.equal(out.detach(), want_out), name
        direct = torch.autograd.grad(out, params, grad_y, retain_graph=True)     # as the backward returns them
        out.backward(grad_y)                                   # (accumulation into .grad drops the is_coalesced flag)
        reference_gy = grad_y if mode == "sum" else G.dev(mean_scaled(gy32, batch, offsets, hot, 0.5 if weighted else 1.0))
        want = single_table_grads(pyt, tables, batch, ids, offsets, hot, reference_gy, w32)
        for t, p in enumerate(params):
            assert direct[t].layout == torch.sparse_coo and direct[t].is_coalesced(), (name, t)
            assert direct[t].values().is_contiguous() and torch.equal(direct[t].to_dense(), want[t]), (name, t)
            assert p.grad.is_sparse and tuple(p.grad.shape) == (ROWS[t], WIDTHS[t]), (name, t)
            i_t = C.table_slice(t, batch, ids, offsets, hot, ids)[0]
            assert p.grad._nnz() == np.unique(i_t).size, (name, t)
            assert torch.equal(p.grad.to_dense(), want[t]), (name, t)


def test_only_the_tables_that_require_grad_get_one_and_weights_may_not(ce, pyt):
    batch, dtype = 5, torch.float32
    tables = tables_of(dtype)
    name, ids, offsets, hot, w32 = C.layouts(batch, rows=ROWS)[3]
    mixed = [torch.nn.Parameter(tables[0].clone()), tables[1], torch.nn.Parameter(tables[2].clone()), tables[3]]
    group = ce.MixedTableGroup(mixed)
    grad_y = G.dev(R.exact_grad_y(np.random.default_rng(1), batch, WIDTHS, "f32"))
    w = G.dev(G.exact_weights(np.random.default_rng(2), ids.size))
    out = pyt.cuemb_embedding_mixed_group_trainable(group, G.dev(ids), G.dev(offsets), w)
    out.backward(grad_y)
    assert mixed[0].grad is not None and mixed[2].grad is not None and mixed[1].grad is None and mixed[3].grad is None
    g = ce.embedding_backward_mixed_group(ce.MixedTableGroup(tables), grad_y, G.dev(ids), G.dev(offsets), w)
    per_table = g.per_table()
    for t in (0, 2):
        assert torch.equal(mixed[t].grad._indices()[0], per_table[t][0].long())
        assert torch.equal(mixed[t].grad._values(), per_table[t][1])
    with pytest.raises(ValueError, match="weight gradient"):
        pyt.cuemb_embedding_mixed_group_trainable(group, G.dev(ids), G.dev(offsets), w.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="mode must be"):
        pyt.cuemb_embedding_mixed_group_trainable(group, G.dev(ids), G.dev(offsets), mode="max")
    with torch.no_grad():                      # grad mode off: just the forward
        plain = pyt.cuemb_embedding_mixed_group_trainable(group, G.dev(ids), G.dev(offsets), w)
    assert not plain.requires_grad and torch.equal(plain, out.detach())
    with pytest.raises(RuntimeError, match="forward only"):        # the plain forward keeps refusing
        ce.embedding_forward_mixed_group(group, G.dev(ids), G.dev(offsets))
