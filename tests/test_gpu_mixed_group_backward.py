"""embedding_backward_mixed_group -- one sort and one scatter-add for a group of tables of DIFFERENT widths -- against T
single-table compressed chains on the contiguous column slices of grad_y (bit for bit on exactly representable data),
against embedding_backward_grouped on same-width groups, against fp64 sums on arbitrary data under the project's bound,
and mixed_group_mean_scale against T grouped_mean_scale calls on one-table groups.

What is new in the kernel is the source address and the active lanes PER LOOKUP; the shapes below are the smallest at
which each can go wrong: tables of 5,000, 17, 300 and 64 rows, B in {1, 5, 1,023}; with segment_len = 8 every segment
near a table boundary holds runs of two widths, and the 17-row table at B = 1,023 has runs of ~1,500 lookups that cross
several workgroups (the chain and the atomics).  Columns >= W_t of an entry are unspecified and never compared."""
import numpy as np
import pytest
import torch

import grouped_backward_cases as G
import grouped_cases as C
import mixed_group_backward_reference as R

pytestmark = pytest.mark.gpu

ROWS = R.ROWS
MIXED = [(128, 16, 64, 32), (36, 4, 128), (6, 2, 10)]
INT_PAIRS = [(np.int32, np.int32), (np.int64, np.int64), (np.int32, np.int64), (np.int64, np.int32)]   # (ids, offsets)


@pytest.fixture(scope="module")
def ce():
    import cuembed_amd
    assert torch.cuda.is_available()
    return cuembed_amd


def ident(widths):
    return "w" + "_".join(map(str, widths))


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


_TABLES = {}


def group_of(ce, dtype, widths):
    """A MixedTableGroup made once per (dtype, widths) and never changed (the backward reads no table value)."""
    key = (dtype, widths)
    if key not in _TABLES:
        _TABLES[key] = ce.MixedTableGroup([torch.zeros(ROWS[t], w, dtype=dtype, device="cuda") for t, w in enumerate(widths)])
    return _TABLES[key]


def exact_sums(widths, rows, batch, ids, offsets, hot, weights, grad_y):
    """The fp64 sums of the padded gradient by sort and segmented sum: (global ids [count], sums [count, W_max])."""
    T, w_max = len(widths), max(widths)
    cols = R.column_base(widths)
    keys, sids = G.global_problem(rows, batch, ids, offsets, hot)
    order = np.argsort(keys, kind="stable")
    keys, sids = keys[order], sids[order]
    t, b = sids % T, sids // T
    padded = np.zeros((batch * T, w_max))
    for k, w in enumerate(widths):
        padded[k::T, :w] = grad_y[:, cols[k]:cols[k + 1]]
    terms = padded[b * T + t] * (1.0 if weights is None else weights[order][:, None])
    if keys.size == 0:
        return keys, np.zeros((0, w_max))
    starts = np.concatenate([[0], np.flatnonzero(np.diff(keys)) + 1])
    return keys[starts], np.add.reduceat(terms, starts, axis=0)


def single_table_chains(ce, widths, rows, batch, ids, offsets, hot, w_d, grad_y, index_dtype):
    """T single-table compressed chains on the contiguous slices of grad_y, laid end to end: (global ids, [rows_t])."""
    base, cols = R.row_base(rows), R.column_base(widths)
    all_ids, all_rows = [], []
    for t, w in enumerate(widths):
        i_t, o_t, w_t = G.table_problem(t, batch, ids, offsets, hot, w_d, index_dtype=index_dtype)
        inv, r = G.single_table(ce, rows[t], grad_y[:, cols[t]:cols[t + 1]].contiguous(), i_t, o_t, hot, w_t, compressed=True)
        all_ids.append(inv.to(torch.int64) + int(base[t]))
        all_rows.append(r)
    return torch.cat(all_ids), all_rows


def check_against_chains(g, want_ids, want_rows, widths, where):
    count = int(g.last_id) + 1
    assert count == want_ids.numel(), where
    assert torch.equal(g.ids[:count].to(torch.int64), want_ids), where
    k = 0
    for t, r in enumerate(want_rows):
        n = r.shape[0]
        assert same_bits(g.rows[k:k + n, :widths[t]], r), (where, t)
        k += n
    assert k == count


def tunings(ce, dtype, widths, nnz):
    """None (default) and segment_len = 8 with every column-slice count out of 1 / 2 / 4 that the lane count allows."""
    lanes = ce.mixed_group_backward_launch_shape(dtype, widths, max(nnz, 1))
    row_lanes = lanes["lanes"] * lanes["column_slices"]
    xcds = ce.device_shape()["xcds"]
    return [None] + [(8, s) for s in (1, 2, 4) if row_lanes % s == 0 and xcds % s == 0]


# ---- 1. bits on exact data ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("batch", C.BATCHES)
@pytest.mark.parametrize("kind", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("widths", MIXED, ids=ident)
def test_exact_data_equals_the_single_table_chains_bit_for_bit(ce, widths, kind, batch):
    dtype = G.DTYPES[kind]
    rows, T = ROWS[:len(widths)], len(widths)
    group = group_of(ce, dtype, widths)
    ce.capacity_overflowed(reset=True)        # (the word is sticky: an earlier test of the process may have raised it)
    try:
        for weighted in (False, True):
            for k, (name, ids, offsets, hot, _) in enumerate(C.layouts(batch, rows=rows)):
                rng = np.random.default_rng(1000 * batch + 10 * k + weighted)
                gy32 = R.exact_grad_y(rng, batch, widths, kind)
                w32 = G.exact_weights(rng, ids.size) if weighted else None
                looked_up, exact = exact_sums(widths, rows, batch, ids, offsets, hot, w32, gy32)
                assert G.representable(kind, weighted, exact), name
                it, ot = INT_PAIRS[(k + weighted) % 4]
                grad_y = G.dev(gy32).to(dtype)
                w_d = None if w32 is None else G.dev(w32).to(dtype)
                ids_d, off_d = G.dev(ids.astype(it)), None if offsets is None else G.dev(offsets.astype(ot))
                ce.set_backward_tuning(segment_len=0, column_slices=0)
                want_ids, want_rows = single_table_chains(ce, widths, rows, batch, ids, offsets, hot, w_d, grad_y, it)
                assert np.array_equal(want_ids.cpu().numpy(), looked_up), name
                for tuning in tunings(ce, dtype, widths, ids.size):
                    if tuning is not None:
                        ce.set_backward_tuning(segment_len=tuning[0], column_slices=tuning[1])
                        shape = ce.mixed_group_backward_launch_shape(dtype, widths, max(ids.size, 1), weighted)
                        assert (shape["segment_len"], shape["column_slices"]) == tuning
                    where = (name, weighted, tuning)
                    g = ce.embedding_backward_mixed_group(group, grad_y, ids_d, off_d, w_d, num_hots=hot)
                    assert g.capacity == min(ids.size, sum(rows)) == g.ids.numel() == g.rows.shape[0], where
                    assert g.rows.shape[1] == max(widths) and g.rows.dtype == dtype and g.ids.dtype == torch.int32
                    assert g.widths == tuple(widths) and g.row_base == tuple(R.row_base(rows)) and g.last_id.numel() == 1
                    check_against_chains(g, want_ids, want_rows, widths, where)
                    count = int(g.last_id) + 1                                  # ... and the sums are right
                    got = g.rows[:count].double().cpu().numpy()
                    table = np.searchsorted(R.row_base(rows), looked_up, side="right") - 1
                    mask = np.arange(max(widths))[None, :] < np.asarray(widths)[table][:, None]
                    assert np.array_equal(got[mask], exact[mask]), where
                    # padding columns: untouched or zero -- whatever they hold, per_table() never shows them
                    per_table = g.per_table()
                    assert [r.shape[1] for _, r in per_table] == list(widths)
                    assert sum(i.numel() for i, _ in per_table) == count
                    assert int(g.table_cuts()[-1]) == count
    finally:
        ce.set_backward_tuning(segment_len=0, column_slices=0)
    assert not ce.capacity_overflowed()


def test_mean_mode_is_the_sum_mode_on_the_scaled_grad_y(ce):
    """mode="mean" = mixed_group_mean_scale in front of the sum pipeline.  A run that crosses workgroups is combined by
    float atomics, whose order is not fixed, so the comparison is made where no order matters: fp32, integer grad_y, bag
    lengths 0 / 1 / 8 / 64 and weights of 0.5 -- every mean factor a power of two, every partial sum exact."""
    widths, batch, dtype = (128, 16, 64, 32), 1023, torch.float32
    T = len(widths)
    group = group_of(ce, dtype, widths)
    layouts = []
    for hot in (1, 8):
        layouts.append(("h%d" % hot, C.draw_ids(np.random.default_rng(hot), ROWS, np.full((T, batch), hot)), None, hot))
    rng = np.random.default_rng(99)
    lengths = rng.choice((0, 1, 8, 64), size=(T, batch))
    layouts.append(("csr", C.draw_ids(rng, ROWS, lengths),
                    np.concatenate([[0], np.cumsum(lengths.reshape(-1))]).astype(np.int64), 0))
    for weighted in (False, True):
        for k, (name, ids, offsets, hot) in enumerate(layouts):
            grad_y = G.dev(R.exact_grad_y(np.random.default_rng(k), batch, widths, "f32"))
            w_d = torch.full((ids.size,), 0.5, device="cuda") if weighted else None
            a = ce.embedding_backward_mixed_group(group, grad_y, G.dev(ids), G.dev(offsets), w_d, num_hots=hot, mode="mean")
            scaled = ce.mixed_group_mean_scale(group, grad_y, G.dev(offsets), w_d, num_hots=hot)
            assert not torch.equal(scaled, grad_y) or hot == 1
            b = ce.embedding_backward_mixed_group(group, scaled, G.dev(ids), G.dev(offsets), w_d, num_hots=hot)
            count = int(a.last_id) + 1
            assert count == int(b.last_id) + 1 and torch.equal(a.ids[:count], b.ids[:count]), name
            looked_up, exact = exact_sums(widths, ROWS, batch, ids, offsets, hot,
                                          None if w_d is None else w_d.double().cpu().numpy(), scaled.double().cpu().numpy())
            for t, ((ia, ra), (ib, rb)) in enumerate(zip(a.per_table(), b.per_table())):
                assert torch.equal(ia, ib) and same_bits(ra, rb), (name, weighted, t)
                mine = (looked_up >= R.row_base(ROWS)[t]) & (looked_up < R.row_base(ROWS)[t + 1])
                assert np.array_equal(ra.double().cpu().numpy(), exact[mine][:, :widths[t]]), (name, weighted, t)


# ---- 2. same-width groups ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("widths", [(36, 36, 36), (128,)], ids=ident)
def test_a_same_width_group_equals_the_grouped_backward(ce, widths, kind):
    dtype = G.DTYPES[kind]
    rows, T, W = ROWS[:len(widths)], len(widths), widths[0]
    mixed = group_of(ce, dtype, widths)
    same = ce.TableGroup(list(mixed.tables))
    for batch in C.BATCHES:
        for weighted in (False, True):
            for k, (name, ids, offsets, hot, _) in enumerate(C.layouts(batch, rows=rows)):
                rng = np.random.default_rng(7000 * batch + 10 * k + weighted)
                gy32 = R.exact_grad_y(rng, batch, widths, kind)
                w32 = G.exact_weights(rng, ids.size) if weighted else None
                assert G.representable(kind, weighted, exact_sums(widths, rows, batch, ids, offsets, hot, w32, gy32)[1])
                grad_y = G.dev(gy32).to(dtype)
                w_d = None if w32 is None else G.dev(w32).to(dtype)
                got = ce.embedding_backward_mixed_group(mixed, grad_y, G.dev(ids), G.dev(offsets), w_d, num_hots=hot)
                want = ce.embedding_backward_grouped(same, grad_y.view(batch, T, W), G.dev(ids), G.dev(offsets), w_d,
                                                     num_hots=hot, dense=False)
                assert torch.equal(got.last_id, want.last_id), (name, batch)          # the count word
                count = int(want.last_id) + 1
                assert got.capacity == want.capacity and torch.equal(got.ids[:count], want.ids[:count]), (name, batch)
                assert same_bits(got.rows[:count], want.rows[:count]), (name, batch, weighted)


# ---- 3. a table without a lookup, no lookups at all, B = 1 -----------------------------------------------------------

def test_a_table_without_a_single_lookup_between_two_others(ce):
    widths, batch, dtype = (128, 16, 64, 32), 5, torch.float16
    group = group_of(ce, dtype, widths)
    name, ids, offsets, hot, _ = [c for c in C.layouts(batch, rows=ROWS) if c[0] == "csr_empty_table"][0]
    assert offsets[batch] == offsets[2 * batch]                 # every bag of table 1 is empty
    grad_y = G.dev(R.exact_grad_y(np.random.default_rng(3), batch, widths, "f16")).to(dtype)
    g = ce.embedding_backward_mixed_group(group, grad_y, G.dev(ids), G.dev(offsets))
    cuts = g.table_cuts().tolist()
    assert cuts[1] == cuts[2] and cuts[0] == 0 and cuts[-1] == int(g.last_id) + 1 > 0
    per_table = g.per_table()
    assert per_table[1][0].numel() == 0 and tuple(per_table[1][1].shape) == (0, 16)
    want_ids, want_rows = single_table_chains(ce, widths, ROWS, batch, ids, offsets, hot, None, grad_y, np.int64)
    check_against_chains(g, want_ids, want_rows, widths, name)


def test_no_lookups_launch_nothing_and_count_zero(ce):
    widths, batch = (128, 16, 64, 32), 5
    group = group_of(ce, torch.float32, widths)
    off = torch.zeros(len(widths) * batch + 1, dtype=torch.int64, device="cuda")
    ids = torch.zeros(0, dtype=torch.int64, device="cuda")
    for mode in ("sum", "mean"):
        g = ce.embedding_backward_mixed_group(group, torch.ones((batch, sum(widths)), device="cuda"), ids, off, mode=mode)
        assert g.capacity == 0 and int(g.last_id) == -1 and int(g.last_id) + 1 == 0 and not g.table_cuts().any()
        assert [(i.numel(), tuple(r.shape)) for i, r in g.per_table()] == [(0, (0, w)) for w in widths]


def test_the_capacity_check_writes_nothing_and_raises_the_word(ce):
    widths, batch, dtype = (128, 16, 64, 32), 5, torch.float16
    group = group_of(ce, dtype, widths)
    name, ids, offsets, hot, _ = C.layouts(batch, rows=ROWS)[1]
    grad_y = G.dev(R.exact_grad_y(np.random.default_rng(4), batch, widths, "f16")).to(dtype)
    ce.capacity_overflowed(reset=True)
    full = ce.embedding_backward_mixed_group(group, grad_y, G.dev(ids), num_hots=hot)
    count = int(full.last_id) + 1
    exact_fit = ce.embedding_backward_mixed_group(group, grad_y, G.dev(ids), num_hots=hot, capacity=count)
    assert exact_fit.capacity == count and not exact_fit.capacity_overflowed()
    assert torch.equal(exact_fit.ids, full.ids[:count])
    small = ce.embedding_backward_mixed_group(group, grad_y, G.dev(ids), num_hots=hot, capacity=count - 1)
    assert small.capacity == count - 1 and int(small.last_id) + 1 == count
    assert small.capacity_overflowed(reset=True) and not ce.capacity_overflowed()
    assert not small.table_cuts().any()            # (a count above the capacity: all-zero cuts, nothing to apply)


# ---- 4. arbitrary data against fp64 ----------------------------------------------------------------------------------

@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("kind", ["f16", "bf16", "f32"])
def test_default_arithmetic_on_arbitrary_data_against_fp64(ce, kind, weighted):
    """The same sums as the single-table chains, associated differently: every VALID element within the bound of
    tests/test_gpu_backward_tolerance.py::_hip_error_bound (mixed_group_backward_reference.hip_error_bound) of the fp64
    sum for 16-bit gradients; fp32 within 1e-5 of the summed magnitudes, the criterion that
    test_fp32_gradients_random_data_within_1e3 asserts (100 times tighter than the 1e-3 its name carries)."""
    widths, batch, dtype = (128, 16, 64, 32), 1023, G.DTYPES[kind]
    group = group_of(ce, dtype, widths)
    for k, (name, ids, offsets, hot, _) in enumerate(C.layouts(batch, rows=ROWS)):
        rng = np.random.default_rng(3000 + 10 * k + weighted)
        grad_y = G.dev(rng.uniform(-1.0, 1.0, (batch, sum(widths))).astype(np.float32)).to(dtype)
        w_d = G.dev(rng.uniform(0.0, 1.0, ids.size).astype(np.float32)).to(dtype) if weighted else None
        exact, scale, walk, run_len, valid = R.fp64_sums(widths, ROWS, batch, ids, offsets, hot,
                                                         None if w_d is None else w_d.double().cpu().numpy(),
                                                         grad_y.double().cpu().numpy())
        shape = ce.mixed_group_backward_launch_shape(dtype, widths, ids.size, weighted)
        bound = (1e-5 * scale + 1e-30 if kind == "f32"
                 else R.hip_error_bound(kind, exact, scale, walk, run_len, shape["lookups_per_block"]))
        g = ce.embedding_backward_mixed_group(group, grad_y, G.dev(ids), G.dev(offsets), w_d, num_hots=hot)
        count = int(g.last_id) + 1
        looked_up = np.flatnonzero(run_len)
        assert count == looked_up.size and np.array_equal(g.ids[:count].cpu().numpy(), looked_up), name
        err = np.abs(g.rows[:count].double().cpu().numpy() - exact[looked_up])
        ok = valid[looked_up]
        print(name, kind, "max error / bound", float((err[ok] / bound[looked_up][ok]).max()))
        assert np.all(err[ok] <= bound[looked_up][ok]), (name, float((err[ok] - bound[looked_up][ok]).max()))


# ---- 5. the mean's scale -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("widths", MIXED, ids=ident)
def test_mean_scale_equals_the_one_table_grouped_mean_scales(ce, widths, kind):
    dtype = G.DTYPES[kind]
    rows, T = ROWS[:len(widths)], len(widths)
    cols = R.column_base(widths)
    group = group_of(ce, dtype, widths)
    ones = [ce.TableGroup([t]) for t in group.tables]
    for batch in (5, 1023):
        for k, (name, ids, offsets, hot, w32) in enumerate(C.layouts(batch, rows=rows)):
            rng = np.random.default_rng(500 * batch + k)
            grad_y = G.dev(rng.uniform(-1.0, 1.0, (batch, sum(widths))).astype(np.float32)).to(dtype)
            w32 = w32.copy()
            if offsets is not None and batch >= 3:          # a bag whose weights sum to zero: the factor is 0
                w32[int(offsets[1]):int(offsets[2])] = 0.0
            w_all = G.dev(w32).to(dtype)
            for weighted in (False, True):
                w_d = w_all if weighted else None
                off_d = G.dev(offsets)
                got = ce.mixed_group_mean_scale(group, grad_y, off_d, w_d, num_hots=hot)
                per_table = []
                for t in range(T):
                    _, o_t, w_t = G.table_problem(t, batch, ids, offsets, hot, w_d, index_dtype=np.int64)
                    slice_t = grad_y[:, cols[t]:cols[t + 1]].contiguous().view(batch, 1, widths[t])
                    per_table.append(ce.grouped_mean_scale(ones[t], slice_t, o_t, w_t, num_hots=hot).view(batch, widths[t]))
                want = torch.cat(per_table, dim=1)
                assert same_bits(got, want), (name, batch, weighted)
                if offsets is not None and weighted and batch >= 3:
                    assert not got[1, :widths[0]].any() and grad_y[1, :widths[0]].any()     # the zero weight sum
                if name == "csr_ragged" and batch >= 3:
                    assert not got[0].any()                                                 # empty bags
                in_place = grad_y.clone()
                assert ce.mixed_group_mean_scale(group, in_place, off_d, w_d, num_hots=hot, out=in_place) is in_place
                assert same_bits(in_place, want), (name, batch, weighted, "in place")


# ---- 6. misalignment -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["f16", "f32"])
def test_a_misaligned_grad_y_narrows_the_lanes_and_keeps_the_bits(ce, kind):
    widths, batch, dtype = (128, 16, 64, 32), 1023, G.DTYPES[kind]
    group = group_of(ce, dtype, widths)
    D, size = sum(widths), dtype.itemsize
    name, ids, offsets, hot, w32 = C.layouts(batch, rows=ROWS)[3]
    rng = np.random.default_rng(77)
    gy = G.dev(R.exact_grad_y(rng, batch, widths, kind)).to(dtype)
    w_d = G.dev(G.exact_weights(rng, ids.size)).to(dtype)
    want = ce.embedding_backward_mixed_group(group, gy, G.dev(ids), G.dev(offsets), w_d)
    assert ce.mixed_group_backward_launch_shape(dtype, widths, ids.size, True, pointer_bits=gy.data_ptr())["elems_per_lane"] \
        == 16 // size
    count = int(want.last_id) + 1
    buffer = torch.zeros(batch * D + 16, dtype=dtype, device="cuda")
    for shift_bytes, lane in ((8, 8), (4, 4)):
        view = buffer[shift_bytes // size:shift_bytes // size + batch * D].view(batch, D)
        view.copy_(gy)
        assert view.data_ptr() % 16 == shift_bytes and view.is_contiguous()
        shape = ce.mixed_group_backward_launch_shape(dtype, widths, ids.size, True, pointer_bits=view.data_ptr())
        assert shape["elems_per_lane"] == lane // size
        got = ce.embedding_backward_mixed_group(group, view, G.dev(ids), G.dev(offsets), w_d)
        assert int(got.last_id) + 1 == count and torch.equal(got.ids[:count], want.ids[:count])
        for (ia, ra), (ib, rb) in zip(got.per_table(), want.per_table()):
            assert torch.equal(ia, ib) and same_bits(ra, rb), shift_bytes


# ---- 7. capture --------------------------------------------------------------------------------------------------------

def test_a_captured_mean_backward_replays_to_the_eager_bits(ce):
    """(fp32, integer grad_y and bag lengths 0 / 1 / 8 / 64: the mean factors are powers of two and every partial sum is
    exact, so the bits do not depend on the order in which the atomics of a long run land.)"""
    widths, batch, dtype = (128, 16, 64, 32), 1023, torch.float32
    T = len(widths)
    group = group_of(ce, dtype, widths)
    rng = np.random.default_rng(123)
    lengths = rng.choice((0, 1, 8, 64), size=(T, batch))
    ids_d = G.dev(C.draw_ids(rng, ROWS, lengths))
    off_d = G.dev(np.concatenate([[0], np.cumsum(lengths.reshape(-1))]).astype(np.int64))
    grad_y = G.dev(R.exact_grad_y(rng, batch, widths, "f32"))
    static = {}

    def step():
        return ce.embedding_backward_mixed_group(group, grad_y, ids_d, off_d, mode="mean")

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()                                    # warm call: the group's device arrays, the overflow word, code loading
        torch.cuda.current_stream().synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            static["g"] = step()
    torch.cuda.synchronize()
    for seed in (1, 2):
        grad_y.copy_(G.dev(R.exact_grad_y(np.random.default_rng(seed), batch, widths, "f32")))
        graph.replay()
        torch.cuda.synchronize()
        eager = step()
        g = static["g"]
        count = int(eager.last_id) + 1
        assert int(g.last_id) + 1 == count and torch.equal(g.ids[:count], eager.ids[:count])
        for (ia, ra), (ib, rb) in zip(g.per_table(), eager.per_table()):
            assert torch.equal(ia, ib) and same_bits(ra, rb) and ra.any(), seed
