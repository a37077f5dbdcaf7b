"""Every backward route on non-finite and signed-zero gradients, against backward_edge_model.py: a planted +Inf, -Inf or
NaN element must reach exactly the (row, column) pairs that look it up, a sum of zeros is +0, untouched memory keeps its
pattern, and rows that may hold anything (those of the exchange's padding ids) leave no trace.

    default backward     every exact case of backward_bits_cases.py under its forced launch shape, through
                         test_gpu_backward_bits.launch_case, on edge_build's planted data: gradient, inverse mapping and
                         overflow word against the model;
    reference_sums       the run lengths of the long-run test on U(-1, 1) data with dedicated poisoned samples around and
                         inside the long runs, against the CPU oracle;
    group                grouped_mean_scale and embedding_backward_grouped (sum / mean, dense / compressed) on the group of
                         grouped_cases.py with exactly summable data;
    weight gradient      embedding_weight_grad and embedding_weight_grad_grouped on tables and gradients that hold
                         non-finite elements;
    exchange             the owner's merge with hashed bit patterns in the rows of padding ids, and the pack as a copy of
                         raw bytes.

Comparison rule (backward_edge_model.compare): where the model is NaN the device is NaN; everywhere else the bits are
identical.  test_backward_edges_host.py asserts, without a GPU, that the data puts the planted elements where they can leak.
"""
import numpy as np
import pytest
import torch

import backward_bits_cases as C
import backward_edge_model as M
import grouped_cases as GC
import grouped_train_reference as R
import test_gpu_backward_bits as P
from test_backward_edges_host import EXACT_CASES, ORACLE_VIEW, group_model
from test_gpu_exchange_native import _backends, _cuts, _merge_expected, _pack_expected

pytestmark = pytest.mark.gpu

TORCH = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
T = len(M.GROUP_ROWS)
BASE = np.concatenate([[0], np.cumsum(M.GROUP_ROWS)]).astype(np.int64)


@pytest.fixture(scope="module")
def ce():
    import cuembed_amd
    assert torch.cuda.is_available()
    return cuembed_amd


def on_device(bits, kind):
    """Bit patterns -> a device tensor of the kind's type."""
    a = np.ascontiguousarray(bits)
    return torch.from_numpy(a.view(np.int16 if a.dtype.itemsize == 2 else np.int32)).cuda().view(TORCH[kind])


def device_bits(t):
    t = t.detach().contiguous()
    wide = t.element_size() == 4
    return t.view(torch.int32 if wide else torch.int16).cpu().numpy().view(np.uint32 if wide else np.uint16)


def dev(a, dtype=None):
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


# ---- the default backward ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", EXACT_CASES)
def test_default_backward_on_planted_data(ce, request, name):
    request.addfinalizer(lambda: ce.set_backward_tuning(0, 0))
    case = C.CASES[name]
    kind = case.kind
    full = P.planned_shape(ce, case)
    d = M.edge_build(case, full["segment_len"], full["segments_per_block"])
    w = None if d["weights_bits"] is None else on_device(d["weights_bits"], kind)
    grad, inverse, overflowed, _ = P.launch_case(ce, case, d, on_device(d["grad_y_bits"], kind), w)
    pattern = M.to_bits(kind, np.array([0.0 if case.out == "skip" else C.PATTERN], dtype=np.float32))[0]
    want, want_inverse, want_overflow, sums = M.default_backward_expected(case, d, P.EXTRA_ROWS, pattern, C.INVERSE_PATTERN)
    assert overflowed == want_overflow
    by_bits, by_class = M.compare(kind, device_bits(grad), want, name)
    assert (by_class > 0) == (case.out != "small")
    if want_inverse is not None:
        assert np.array_equal(inverse.cpu().numpy().astype(np.int64), want_inverse), "inverse_mapping"


# ---- reference_sums ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("kind,width", M.REFERENCE_SHAPES)
def test_reference_sums_on_planted_data(ce, oracle, kind, width, weighted):
    """The doc promises the oracle's bits "for ANY data": poisoned samples just before and after every long run, at the
    clamp target nnz - 1, in the middle of a long run and of a short run between two long ones; full and compressed; a
    pre-filled buffer with rows of -0.0 and of infinities."""
    p = M.reference_sums_problem(kind, width, weighted)
    ti, ts = p["ti"], p["ts"]
    as_oracle = lambda bits: None if bits is None else bits.view(ORACLE_VIEW[kind])
    gy_o, w_o = as_oracle(p["grad_y_bits"]), as_oracle(p["weights_bits"])
    gy_d = on_device(p["grad_y_bits"], kind)
    w_d = None if p["weights_bits"] is None else on_device(p["weights_bits"], kind)
    for compressed in (False, True):
        remap = oracle.compute_compressed_grad_indices(ti) if compressed else None
        rows = int(remap[-1]) + 1 if compressed else p["ncat"]
        want, want_inverse = oracle.embedding_backward(gy_o, width, rows, ti, ts, remap, w_o)
        got, inverse = ce.embedding_backward(gy_d, rows, dev(ti), dev(ts), dev(remap), w_d, reference_sums=True)
        _, by_class = M.compare(kind, device_bits(got), np.ascontiguousarray(want).view(M.BITS[kind]), (kind, width, compressed))
        assert by_class > 0
        if compressed:
            assert np.array_equal(inverse.cpu().numpy(), want_inverse)
    start = p["start"]
    want, _ = oracle.embedding_backward(gy_o, width, p["ncat"], ti, ts, None, w_o, skip_grad_init=True,
                                        grad_embedding=as_oracle(start.copy()))
    got, _ = ce.embedding_backward(gy_d, p["ncat"], dev(ti), dev(ts), None, w_d, skip_grad_init=True,
                                   grad_embedding=on_device(start, kind), reference_sums=True)
    M.compare(kind, device_bits(got), np.ascontiguousarray(want).view(M.BITS[kind]), (kind, width, "pre-filled"))
    untouched = np.setdiff1d(np.arange(p["ncat"]), p["row_ids"])
    assert np.array_equal(device_bits(got)[untouched], start[untouched])


# ---- the group -----------------------------------------------------------------------------------------------------------
def group_of(ce, kind, width):
    return ce.TableGroup([on_device(bits, kind) for _, bits in M.group_tables(kind, width)])


@pytest.mark.parametrize("width", M.GROUP_WIDTHS)
@pytest.mark.parametrize("batch", M.GROUP_BATCHES)
@pytest.mark.parametrize("kind", ["f32", "f16", "bf16"])
def test_grouped_mean_scale_on_planted_data(ce, kind, batch, width):
    """Inf * 0 = NaN and -x * 0 = -0 in bags that are empty or whose weights sum to 0: the model's bits, out of place
    and in place."""
    group = group_of(ce, kind, width)
    for layout in M.GROUP_LAYOUTS:
        p = M.group_problem(kind, batch, width, layout)
        grad_y, offsets = on_device(p["grad_y_bits"], kind), dev(p["offsets"])
        for weighted in (False, True):
            w32 = p["weights"] if weighted else None
            w_d = on_device(p["weights_bits"], kind) if weighted else None
            with np.errstate(all="ignore"):
                want = M.to_bits(kind, R.mean_scale(kind, p["grad_y"], R.mean_factor(T, batch, p["offsets"], p["hot"], w32)))
            got = ce.grouped_mean_scale(group, grad_y, offsets, w_d, num_hots=p["hot"])
            assert got.data_ptr() != grad_y.data_ptr()
            _, by_class = M.compare(kind, device_bits(got), want, (layout, weighted))
            assert by_class > 0
            assert np.array_equal(device_bits(grad_y), p["grad_y_bits"])          # the source is left alone
            work = grad_y.clone()
            back = ce.grouped_mean_scale(group, work, offsets, w_d, num_hots=p["hot"], out=work)
            assert back is work
            M.compare(kind, device_bits(work), want, (layout, weighted, "in place"))


@pytest.mark.parametrize("width", M.GROUP_WIDTHS)
@pytest.mark.parametrize("batch", M.GROUP_BATCHES)
@pytest.mark.parametrize("kind", ["f32", "f16", "bf16"])
def test_grouped_backward_on_planted_data(ce, kind, batch, width):
    group = group_of(ce, kind, width)
    ce.capacity_overflowed(reset=True)
    for layout in M.GROUP_LAYOUTS:
        p = M.group_problem(kind, batch, width, layout)
        grad_y, offsets, ids = on_device(p["grad_y_bits"], kind), dev(p["offsets"]), dev(p["ids"])
        keys = np.unique(M.group_keys(batch, p)[0])
        for weighted in (False, True):
            w_d = on_device(p["weights_bits"], kind) if weighted else None
            for mode in ("sum", "mean"):
                want = M.to_bits(kind, group_model(kind, batch, width, layout, mode, weighted)[2].value)
                label = (layout, weighted, mode)
                got, views = ce.embedding_backward_grouped(group, grad_y, ids, offsets, w_d, num_hots=p["hot"], dense=True,
                                                           mode=mode)
                M.compare(kind, device_bits(got), want, label + ("dense",))
                assert len(views) == T and views[2].data_ptr() == got[int(BASE[2]):].data_ptr()
                g = ce.embedding_backward_grouped(group, grad_y, ids, offsets, w_d, num_hots=p["hot"], mode=mode)
                count = int(g.last_id.item()) + 1
                assert count == keys.size and np.array_equal(g.ids[:count].cpu().numpy(), keys), label
                M.compare(kind, device_bits(g.rows[:count]), want[keys], label + ("compressed",))
                assert np.array_equal(device_bits(grad_y), p["grad_y_bits"])
    assert not ce.capacity_overflowed(reset=True)


@pytest.mark.parametrize("width", M.GROUP_WIDTHS)
@pytest.mark.parametrize("kind", ["f32", "f16", "bf16"])
def test_weight_gradient_on_planted_data(ce, kind, width):
    """0 * Inf wherever a table row holds a zero; lookups of clean rows in clean samples stay finite and exact."""
    tables = M.group_tables(kind, width)
    flat = np.concatenate([values for values, _ in tables])
    device_tables = [on_device(bits, kind) for _, bits in tables]
    group = ce.TableGroup(device_tables)
    for batch, layout in M.WEIGHT_GRAD_CASES:
        p = M.group_problem(kind, batch, width, layout)
        keys, samples, table_of, _ = M.group_keys(batch, p)
        value, _, _ = M.weight_grad(flat, keys, p["grad_y"].reshape(-1, width), samples)
        want = M.to_bits(kind, value)
        grad_y = on_device(p["grad_y_bits"], kind)
        got = ce.embedding_weight_grad_grouped(group, grad_y, dev(p["ids"]), dev(p["offsets"]), num_hots=p["hot"])
        _, by_class = M.compare(kind, device_bits(got), want, (batch, layout, "grouped"))
        assert by_class > 0
        for t in range(T):
            position = np.arange(p["ids"].size, dtype=np.float32)
            ids_t, offsets_t, at = GC.table_slice(t, batch, p["ids"], p["offsets"], p["hot"], position)
            if ids_t.size == 0:
                continue
            one = ce.embedding_weight_grad(device_tables[t], dev(ids_t), grad_y[:, t, :].contiguous(), dev(offsets_t),
                                           batch_size=batch, num_hots=p["hot"])
            lo = int(at[0])
            assert np.all(table_of[lo:lo + ids_t.size] == t)
            M.compare(kind, device_bits(one), want[lo:lo + ids_t.size], (batch, layout, "table %d" % t))


# ---- the exchange ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", ["c_abi", "torch_op"])
@pytest.mark.parametrize("kind,width", [("f16", 256), ("f32", 33), ("bf16", 64)])
def test_owner_merge_with_anything_in_the_padding_rows(backend, kind, width):
    """The rows that padding ids carry hold what an earlier step left there -- NaNs, infinities, -0.0, huge values.  The
    merge sums them into the padding run's row and FinishOwnerPiece zeroes it: every row from the count on is +0, and
    the real rows hold exactly what their own lookups sum to."""
    _, merge = _backends()[backend]
    rng = np.random.default_rng(29 + width)
    pad_lo, pad_len = 1234, 777
    for n, distinct, padding, capacity in M.MERGE_CASES:
        ids, bits = M.merge_problem(kind, width, n, distinct, padding, capacity)
        case = (n, distinct, padding, capacity)
        before_ids = rng.integers(0, M.MERGE_CATEGORIES, size=capacity + 1).astype(np.int64)
        before_rows = rng.integers(-2, 3, size=(capacity + 1, width)).astype(np.float32)
        out_ids = dev(before_ids)
        out_rows = dev(before_rows, TORCH[kind])
        tail = torch.full((capacity + 2,), -5, dtype=torch.int64, device="cuda")
        flag = torch.zeros((1,), dtype=torch.int64, device="cuda")
        count = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        merge(dev(ids), on_device(bits, kind), M.MERGE_CATEGORIES, pad_lo, pad_len, out_ids, out_rows, tail, flag, count)
        torch.cuda.synchronize()
        real = ids < M.MERGE_CATEGORIES
        values = M.from_bits(kind, bits)
        with np.errstate(all="ignore"):
            e_ids, _, k, e_flag = _merge_expected(ids, np.where(real[:, None], values, 0), M.MERGE_CATEGORIES, capacity,
                                                  pad_lo, pad_len, before_ids, before_rows)
        assert e_flag == 0 and int(count.item()) == k and int(flag.item()) == 0, case
        assert np.array_equal(out_ids.cpu().numpy(), e_ids), case
        want = np.full((capacity + 1, width), M.special(kind, "+0"), dtype=M.BITS[kind])
        if k:
            _, inverse = np.unique(ids[real], return_inverse=True)
            want[:k] = M.to_bits(kind, M.scatter_add(inverse, np.flatnonzero(real), values, None, k, chunk=width,
                                                     reasons=False).value)
        got = device_bits(out_rows)
        assert not got[k:].any(), "%r: a row at or past the count is not +0" % (case,)
        M.compare(kind, got, want, case)
        t = tail.cpu().numpy()
        assert np.array_equal(t[:capacity], e_ids[:capacity]) and t[capacity] == k and t[capacity + 1] == 0, case


@pytest.mark.parametrize("backend", ["c_abi", "torch_op"])
@pytest.mark.parametrize("kind,width", [("f16", 256), ("f16", 33), ("f32", 7), ("bf16", 64)])
def test_pack_is_a_copy_of_raw_bytes(backend, kind, width):
    """Rows with NaN payloads of either sign, infinities and -0.0 arrive byte for byte; rows behind a slot's ids keep
    theirs."""
    pack, _ = _backends()[backend]
    rng = np.random.default_rng(17 + width)
    num_categories = 100_000
    for world, n, slot, count in [(3, 5000, 2500, 4100), (8, 3000, 300, None), (4, 1, 16, None), (64, 4000, 90, 3999)]:
        ids = np.sort(rng.choice(num_categories, size=n, replace=False)).astype(np.int64)
        bits = M.hashed_patterns(kind, (n, width), world)
        assert n * width < 64 or (M.is_nan_bits(kind, bits).any() and (bits == M.special(kind, "-0")).any())
        cuts = _cuts(num_categories, world)
        before = M.hashed_patterns(kind, (world * slot, width), 1000 + world)
        send_ids = torch.full((world * slot,), -7, dtype=torch.int64, device="cuda")
        send_rows = on_device(before, kind)
        starts = torch.full((world + 1,), -1, dtype=torch.int64, device="cuda")
        flag = torch.zeros((1,), dtype=torch.int64, device="cuda")
        d_count = None if count is None else torch.tensor([count], dtype=torch.int64, device="cuda")
        pack(dev(ids), on_device(bits, kind), d_count, dev(cuts), slot, 0, num_categories, send_ids, send_rows, starts, flag)
        torch.cuda.synchronize()
        e_ids, e_rows, written, e_starts, e_flag = _pack_expected(ids, bits, count, cuts, slot, 0, num_categories)
        case = (world, n, slot, count)
        assert np.array_equal(starts.cpu().numpy(), e_starts) and np.array_equal(send_ids.cpu().numpy(), e_ids), case
        assert int(flag.item()) == e_flag, case
        got = device_bits(send_rows)
        assert np.array_equal(got[written], e_rows[written]), case
        assert np.array_equal(got[~written], before[~written]), case
