"""embedding_backward_grouped -- one sort and one scatter-add for a group of tables -- against the single-table pipeline
on each table's own bags (grouped_cases.table_slice): bit for bit on exactly representable data and with
reference_sums on arbitrary data; against an fp64 sum under the bound of test_gpu_backward_tolerance.py with the default
arithmetic; and the one-storage group: the same forward bits, one SGD step on group.flat equal to the per-table steps."""
import numpy as np
import pytest
import torch

import grouped_backward_cases as G
import grouped_cases as C

pytestmark = pytest.mark.gpu

WIDTH = 64
T = len(C.ROWS)
TOTAL = sum(C.ROWS)
BASE = np.concatenate([[0], np.cumsum(C.ROWS)])

# tests/test_gpu_backward_tolerance.py, bound (3): the same constants
EPS = {"f16": 2.0 ** -11, "bf16": 2.0 ** -8}
TINY = 2.0 ** -23


def _hip_error_bound(kind, exact, scale, walk, run_len):
    """What fp32 partial sums with 16-bit flushes can be off by (test_gpu_backward_tolerance._hip_error_bound): a run
    inside one workgroup is rounded once; one that crosses workgroups is combined by one 16-bit atomic per workgroup it
    touches (>= 256 lookups each), each rounding a partial sum the size of a random walk over the terms."""
    flushes = 2 + run_len // 256
    return (EPS[kind] * (np.abs(exact) + 4.0 * (np.sqrt(flushes)[:, None] + 1.0) * walk)
            + 1e-5 * scale + TINY)


@pytest.fixture(scope="module")
def ce():
    import cuembed_amd
    assert torch.cuda.is_available()
    return cuembed_amd


def tables_of(dtype, width=WIDTH):
    return [torch.from_numpy(C.table_values(t, rows, width)).cuda().to(dtype) for t, rows in enumerate(C.ROWS)]


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


@pytest.mark.parametrize("batch", C.BATCHES)
@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("kind", ["f32", "f16", "bf16"])
def test_exact_data_equals_the_single_table_calls_bit_for_bit(ce, kind, weighted, batch):
    dtype = G.DTYPES[kind]
    group = ce.TableGroup(tables_of(dtype))
    ce.capacity_overflowed(reset=True)        # (the word is sticky: an earlier test of the process may have raised it)
    for k, (name, ids, offsets, hot, _) in enumerate(C.layouts(batch)):
        rng = np.random.default_rng(1000 * batch + 10 * k + weighted)
        gy32 = G.exact_grad_y(rng, batch, T, WIDTH, kind)
        w32 = G.exact_weights(rng, ids.size) if weighted else None
        keys, sids = G.global_problem(C.ROWS, batch, ids, offsets, hot)
        exact = G.fp64_sums(keys, sids, gy32.reshape(batch * T, WIDTH).astype(np.float64), w32, TOTAL)[0]
        assert G.representable(kind, weighted, exact), name
        grad_y = G.dev(gy32).to(dtype)
        w_d = None if w32 is None else G.dev(w32).to(dtype)
        ids_d, off_d = G.dev(ids), G.dev(offsets)
        dense, views = ce.embedding_backward_grouped(group, grad_y, ids_d, off_d, w_d, num_hots=hot, dense=True)
        assert tuple(dense.shape) == (TOTAL, WIDTH) and dense.dtype == dtype and len(views) == T
        assert np.array_equal(dense.double().cpu().numpy(), exact), name               # ... and the sums are right
        g = ce.embedding_backward_grouped(group, grad_y, ids_d, off_d, w_d, num_hots=hot)
        assert g.capacity == min(ids.size, TOTAL) == g.ids.numel() == g.rows.shape[0] and g.row_base == tuple(BASE)
        assert g.ids.dtype == torch.int32 and g.last_id.numel() == 1
        cuts = g.table_cuts()
        assert int(cuts[-1]) == int(g.last_id) + 1 == np.unique(keys).size
        per_table = g.per_table()
        for t, rows_t in enumerate(C.ROWS):
            assert views[t].data_ptr() == dense[BASE[t]:].data_ptr() and views[t].shape[0] == rows_t
            i_t, o_t, w_t = G.table_problem(t, batch, ids, offsets, hot, w_d)
            grad_t = grad_y[:, t].contiguous()
            want = G.single_table(ce, rows_t, grad_t, i_t, o_t, hot, w_t, compressed=False)
            assert same_bits(views[t], want), (name, t)
            want_ids, want_rows = G.single_table(ce, rows_t, grad_t, i_t, o_t, hot, w_t, compressed=True)
            got_ids, got_rows = per_table[t]
            assert torch.equal(got_ids, want_ids) and same_bits(got_rows, want_rows), (name, t)
    assert not ce.capacity_overflowed()


@pytest.mark.parametrize("batch", [5, 1023])
@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("kind", ["f32", "f16", "bf16"])
def test_reference_sums_on_arbitrary_data_equal_the_single_table_calls(ce, kind, weighted, batch):
    """A rounding chain in nz order is untouched by the grouping: the sort is stable, so inside one table row the
    lookups keep the single-table order."""
    dtype = G.DTYPES[kind]
    group = ce.TableGroup(tables_of(dtype))
    for k, (name, ids, offsets, hot, w32) in enumerate(C.layouts(batch)):
        rng = np.random.default_rng(2000 * batch + 10 * k + weighted)
        grad_y = G.dev(rng.uniform(-1.0, 1.0, (batch, T, WIDTH)).astype(np.float32)).to(dtype)
        w_d = G.dev(w32).to(dtype) if weighted else None
        _, views = ce.embedding_backward_grouped(group, grad_y, G.dev(ids), G.dev(offsets), w_d, num_hots=hot, dense=True,
                                                 reference_sums=True)
        for t, rows_t in enumerate(C.ROWS):
            i_t, o_t, w_t = G.table_problem(t, batch, ids, offsets, hot, w_d)
            want = G.single_table(ce, rows_t, grad_y[:, t].contiguous(), i_t, o_t, hot, w_t, compressed=False,
                                  reference_sums=True)
            assert same_bits(views[t], want), (name, t)


@pytest.mark.parametrize("batch", [5, 1023])
@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("kind", ["f32", "f16", "bf16"])
def test_default_arithmetic_on_arbitrary_data_against_fp64(ce, kind, weighted, batch):
    """The segment cuts of the scatter-add move with the position in the combined stream, so bit equality with the
    per-table call is NOT claimed: the same sums, associated differently.  16-bit gradients: bound (3) of
    test_gpu_backward_tolerance.py; fp32: that file's fp32 criterion, 1e-5 of the summed magnitudes."""
    dtype = G.DTYPES[kind]
    group = ce.TableGroup(tables_of(dtype))
    for k, (name, ids, offsets, hot, w32) in enumerate(C.layouts(batch)):
        rng = np.random.default_rng(3000 * batch + 10 * k + weighted)
        grad_y = G.dev(rng.uniform(-1.0, 1.0, (batch, T, WIDTH)).astype(np.float32)).to(dtype)
        w_d = G.dev(w32).to(dtype) if weighted else None
        keys, sids = G.global_problem(C.ROWS, batch, ids, offsets, hot)
        exact, scale, walk, run_len = G.fp64_sums(keys, sids, grad_y.double().cpu().numpy().reshape(batch * T, WIDTH),
                                                  None if w_d is None else w_d.double().cpu().numpy(), TOTAL)
        bound = 1e-5 * scale + 1e-30 if kind == "f32" else _hip_error_bound(kind, exact, scale, walk, run_len)
        dense, _ = ce.embedding_backward_grouped(group, grad_y, G.dev(ids), G.dev(offsets), w_d, num_hots=hot, dense=True)
        err = np.abs(dense.double().cpu().numpy() - exact)
        print(name, kind, "dense: max error / bound", float((err / bound).max()))
        assert np.all(err <= bound), (name, float((err - bound).max()))
        g = ce.embedding_backward_grouped(group, grad_y, G.dev(ids), G.dev(offsets), w_d, num_hots=hot)
        count = int(g.last_id) + 1
        looked_up = np.unique(keys)
        assert count == looked_up.size and np.array_equal(g.ids[:count].cpu().numpy(), looked_up), name
        err = np.abs(g.rows[:count].double().cpu().numpy() - exact[looked_up])
        print(name, kind, "compressed: max error / bound", float((err / bound[looked_up]).max()))
        assert np.all(err <= bound[looked_up]), (name, float((err - bound[looked_up]).max()))


def test_int64_indices_and_offsets_give_the_same_gradient(ce):
    """The keys are written fresh as int32 whatever the indices' type: the same gradient from int64 and int32 input."""
    batch, dtype = 5, torch.float16
    group = ce.TableGroup(tables_of(dtype))
    for k, (name, ids, offsets, hot, _) in enumerate(C.layouts(batch)):
        grad_y = G.dev(G.exact_grad_y(np.random.default_rng(k), batch, T, WIDTH, "f16")).to(dtype)
        a = ce.embedding_backward_grouped(group, grad_y, G.dev(ids), G.dev(offsets), num_hots=hot)
        b = ce.embedding_backward_grouped(group, grad_y, G.dev(ids.astype(np.int32)),
                                          None if offsets is None else G.dev(offsets.astype(np.int32)), num_hots=hot)
        assert a.ids.dtype == b.ids.dtype == torch.int32 and torch.equal(a.last_id, b.last_id)
        n = int(a.last_id) + 1
        assert torch.equal(a.ids[:n], b.ids[:n]) and same_bits(a.rows[:n], b.rows[:n]), name


def test_an_empty_batch_gives_an_empty_gradient(ce):
    group = ce.TableGroup(tables_of(torch.float32))
    off = torch.zeros(T * 5 + 1, dtype=torch.int64, device="cuda")
    ids = torch.zeros(0, dtype=torch.int64, device="cuda")
    grad_y = torch.ones((5, T, WIDTH), device="cuda")
    dense, views = ce.embedding_backward_grouped(group, grad_y, ids, off, dense=True)
    assert not dense.any() and [v.shape[0] for v in views] == list(C.ROWS)
    g = ce.embedding_backward_grouped(group, grad_y, ids, off)
    assert g.capacity == 0 and int(g.last_id) == -1 and not g.table_cuts().any()
    assert [(i.numel(), r.shape[0]) for i, r in g.per_table()] == [(0, 0)] * T


@pytest.mark.parametrize("kind,width", [("f16", 6), ("f16", 64), ("f32", 64), ("bf16", 36)])
def test_one_storage_forward_equals_separate_tensors(ce, kind, width):
    """Width 6 in fp16: 12-byte rows, so the slices' bases are only 4-byte aligned (table 2 begins 60,204 bytes in) and
    the group runs on 4-byte lanes; 36 bf16: 72-byte rows, 8-byte lanes and bases."""
    dtype = G.DTYPES[kind]
    separate = tables_of(dtype, width)
    group = ce.TableGroup.allocate(C.ROWS, width, dtype=dtype)
    assert group.flat.is_cuda and not group.flat.any()
    for t, table in enumerate(separate):
        group.tables[t].copy_(table)
    assert torch.equal(group.flat, torch.cat(separate))
    if width == 6:
        assert group.lane_bytes() == 4 and ce.TableGroup(separate).lane_bytes() == 4
        assert any(p % 8 for p in group.host_ptrs)
    for batch in (5, 1023):
        for name, ids, offsets, hot, w32 in C.layouts(batch):
            for mode in ("sum", "mean"):
                for w in (None, G.dev(w32).to(dtype)):
                    got = ce.embedding_forward_grouped(group, G.dev(ids), G.dev(offsets), w, num_hots=hot, mode=mode)
                    want = ce.embedding_forward_grouped(separate, G.dev(ids), G.dev(offsets), w, num_hots=hot, mode=mode)
                    assert same_bits(got, want), (name, batch, mode)


@pytest.mark.parametrize("kind", ["f32", "f16", "bf16"])
def test_one_sgd_step_on_the_flat_storage_equals_the_per_table_steps(ce, kind):
    """sparse_row_update on group.flat with the grouped gradient's global ids and device-side count, no read-back:
    every table gets the bits of its own single-table step, and rows that were not looked up are untouched."""
    dtype, batch, lr = G.DTYPES[kind], 1023, 0.125
    separate = tables_of(dtype)
    ce.capacity_overflowed(reset=True)        # (sticky: see above)
    for k, (name, ids, offsets, hot, _) in enumerate(C.layouts(batch)):
        rng = np.random.default_rng(50 + k)
        grad_y = G.dev(G.exact_grad_y(rng, batch, T, WIDTH, kind)).to(dtype)
        w_d = G.dev(G.exact_weights(rng, ids.size)).to(dtype)
        group = ce.TableGroup.from_flat(torch.cat(separate), C.ROWS)
        before = group.flat.clone()
        g = ce.embedding_backward_grouped(group, grad_y, G.dev(ids), G.dev(offsets), w_d, num_hots=hot)
        ce.sparse_row_update(group.flat, g.ids, g.rows, rule="sgd", lr=lr, last_id=g.last_id)
        keys, _ = G.global_problem(C.ROWS, batch, ids, offsets, hot)
        untouched = np.setdiff1d(np.arange(TOTAL), keys)
        assert untouched.size > 0
        assert same_bits(group.flat[G.dev(untouched)], before[G.dev(untouched)]), name
        for t, rows_t in enumerate(C.ROWS):
            i_t, o_t, w_t = G.table_problem(t, batch, ids, offsets, hot, w_d)
            table = separate[t].clone()
            inv, rows = G.single_table(ce, rows_t, grad_y[:, t].contiguous(), i_t, o_t, hot, w_t, compressed=True)
            if inv.numel():
                ce.sparse_row_update(table, inv, rows, rule="sgd", lr=lr)
                assert not same_bits(table, separate[t])
            assert same_bits(group.tables[t], table), (name, t)
    assert not ce.capacity_overflowed()


def test_adam_on_the_flat_storage_takes_the_grouped_gradient_as_it_is(ce):
    """The rest of the sparse optimizer family applies unchanged: one lazy-Adam step on group.flat equals the per-table
    steps on exact data."""
    dtype, batch = torch.float32, 5
    separate = tables_of(dtype)
    name, ids, offsets, hot, _ = C.layouts(batch)[3]
    rng = np.random.default_rng(9)
    grad_y = G.dev(G.exact_grad_y(rng, batch, T, WIDTH, "f32"))
    group = ce.TableGroup.from_flat(torch.cat(separate), C.ROWS)
    m, v = torch.zeros_like(group.flat), torch.zeros_like(group.flat)
    g = ce.embedding_backward_grouped(group, grad_y, G.dev(ids), G.dev(offsets))
    ce.sparse_row_adam(group.flat, g.ids, g.rows, exp_avg=m, exp_avg_sq=v, lr=0.01, last_id=g.last_id)
    for t, rows_t in enumerate(C.ROWS):
        i_t, o_t, _ = G.table_problem(t, batch, ids, offsets, hot)
        table = separate[t].clone()
        inv, rows = G.single_table(ce, rows_t, grad_y[:, t].contiguous(), i_t, o_t, hot, None, compressed=True)
        if inv.numel():
            ce.sparse_row_adam(table, inv, rows, exp_avg=torch.zeros_like(table), exp_avg_sq=torch.zeros_like(table), lr=0.01)
        assert same_bits(group.tables[t], table), t
