"""The mixed-width grouped backward as torch ops (cuembed_pyt::cuembed_embedding_backward_mixed_group and
cuembed_pyt::cuembed_mixed_group_mean_scale): they exist with the documented schemas, give the same tensors as the Python
calls, their fake implementations give the right shapes and dtypes, and they reject what the functions reject."""
import numpy as np
import pytest
import torch

import grouped_backward_cases as G
import grouped_cases as C
import mixed_group_backward_reference as R

pytestmark = pytest.mark.gpu

ROWS = (5000, 17, 300)
WIDTHS = (36, 4, 128)
BATCH = 5


@pytest.fixture(scope="module")
def ce():
    import cuembed_amd
    assert torch.cuda.is_available()
    return cuembed_amd


@pytest.fixture(scope="module")
def pyt():
    from cuembed_amd import cuembed_pyt
    return cuembed_pyt


@pytest.fixture(scope="module")
def group(ce):
    return ce.MixedTableGroup([torch.zeros(ROWS[t], w, dtype=torch.float16, device="cuda") for t, w in enumerate(WIDTHS)])


def sorted_lookups(ce, group, ids, off, hot, weights):
    T, total = group.num_tables, group.total_rows
    keys, sids = torch.ops.cuembed_pyt.cuembed_grouped_backward_keys(ids, off, group.row_base_device, T, BATCH, hot, True)
    return ce.transpose(sids, keys, weights, num_categories=total, remapped=True)


def test_the_ops_exist_with_their_schemas(pyt):
    ops = torch.ops.cuembed_pyt
    scatter = str(ops.cuembed_embedding_backward_mixed_group.default._schema)
    assert "int[] widths" in scatter and "Tensor table_columns" in scatter and "int capacity" in scatter
    assert "Tensor? transpose_weights" in scatter and scatter.endswith("-> (Tensor, Tensor, Tensor)")
    scale = str(ops.cuembed_mixed_group_mean_scale.default._schema)
    assert "int[] widths" in scale and "Tensor? offsets" in scale and "int hotness" in scale and scale.endswith("-> Tensor")


def test_the_ops_agree_with_the_functions(ce, pyt, group):
    ops = torch.ops.cuembed_pyt
    for k, (name, ids, offsets, hot, w32) in enumerate(C.layouts(BATCH, ROWS)):
        rng = np.random.default_rng(k)
        grad_y = G.dev(R.exact_grad_y(rng, BATCH, WIDTHS, "f16")).half()
        ids_d, off_d = G.dev(ids), G.dev(offsets)
        for weights in (None, G.dev(G.exact_weights(rng, ids.size)).half()):
            want = ce.embedding_backward_mixed_group(group, grad_y, ids_d, off_d, weights, num_hots=hot)
            t_keys, t_sids, t_w, remap = sorted_lookups(ce, group, ids_d, off_d, hot, weights)
            rows, inv, overflow = ops.cuembed_embedding_backward_mixed_group(
                grad_y, list(WIDTHS), group.table_columns_device, t_keys, t_sids, remap, t_w, want.capacity)
            count = int(remap[-1]) + 1
            assert count == int(want.last_id) + 1 and int(overflow) == 0
            assert rows.shape == want.rows.shape and rows.dtype == want.rows.dtype and inv.dtype == want.ids.dtype
            assert torch.equal(inv[:count], want.ids[:count]), name
            cuts = want.table_cuts().tolist()
            for t, w in enumerate(WIDTHS):
                assert torch.equal(rows[cuts[t]:cuts[t + 1], :w], want.rows[cuts[t]:cuts[t + 1], :w]), (name, t)
            # a capacity below the count: nothing is written, the op's own word says so
            small = ops.cuembed_embedding_backward_mixed_group(grad_y, list(WIDTHS), group.table_columns_device, t_keys,
                                                               t_sids, remap, t_w, count - 1)
            assert int(small[2]) == 1 and small[0].shape[0] == count - 1
        for weights in (None, G.dev(w32).half()):
            want = ce.mixed_group_mean_scale(group, grad_y, off_d, weights, num_hots=hot)
            got = ops.cuembed_mixed_group_mean_scale(grad_y, list(WIDTHS), group.table_columns_device, off_d, weights, hot)
            assert got.dtype == want.dtype and torch.equal(got, want), name


def test_the_ops_reject_what_the_functions_reject(ce, pyt, group):
    ops = torch.ops.cuembed_pyt
    name, ids, offsets, hot, _ = C.layouts(BATCH, ROWS)[3]
    ids_d, off_d = G.dev(ids), G.dev(offsets)
    grad_y = torch.zeros((BATCH, sum(WIDTHS)), dtype=torch.float16, device="cuda")
    t_keys, t_sids, _, remap = sorted_lookups(ce, group, ids_d, off_d, hot, None)
    columns, widths = group.table_columns_device, list(WIDTHS)
    scatter, scale = ops.cuembed_embedding_backward_mixed_group, ops.cuembed_mixed_group_mean_scale
    with pytest.raises(RuntimeError):     # y_grad of another width
        scatter(grad_y[:, :-2].contiguous(), widths, columns, t_keys, t_sids, remap, None, 10)
    with pytest.raises(RuntimeError):     # one (column, width) pair per table
        scatter(grad_y, widths, columns[:2].contiguous(), t_keys, t_sids, remap, None, 10)
    with pytest.raises(RuntimeError):     # the columns as int64
        scatter(grad_y, widths, columns.long(), t_keys, t_sids, remap, None, 10)
    with pytest.raises(RuntimeError):     # sample ids of another length
        scatter(grad_y, widths, columns, t_keys, t_sids[:-1], remap, None, 10)
    with pytest.raises(RuntimeError):     # remapped ids of another dtype
        scatter(grad_y, widths, columns, t_keys, t_sids, remap.long(), None, 10)
    with pytest.raises(RuntimeError):     # weights of another dtype
        scatter(grad_y, widths, columns, t_keys, t_sids, remap, torch.ones(ids.size, device="cuda"), 10)
    with pytest.raises(RuntimeError):     # a negative capacity
        scatter(grad_y, widths, columns, t_keys, t_sids, remap, None, -1)
    with pytest.raises(RuntimeError):     # a row that is no multiple of 4 bytes
        scatter(grad_y, [35, 5, 128], columns, t_keys, t_sids, remap, None, 10)
    with pytest.raises(RuntimeError):     # offsets of a length that is not num_tables * batch + 1
        scale(grad_y, widths, columns, off_d[:-1], None, 0)
    with pytest.raises(RuntimeError):     # neither CSR nor a hotness
        scale(grad_y, widths, columns, None, None, 0)
    with pytest.raises(RuntimeError):     # weights of another dtype
        scale(grad_y, widths, columns, off_d, torch.ones(ids.size, device="cuda"), 0)
    with pytest.raises(RuntimeError):     # a tensor on the CPU
        scale(grad_y.cpu(), widths, columns, off_d, None, 0)


def test_the_scatter_op_raises_on_a_table_of_more_than_1024_lanes(ce, pyt):
    """fp16 rows of 2,050 elements are 4,100 bytes: 4-byte lanes, 1,025 of them.  The op takes its lane from the library
    and must RAISE on the limit, before any launch (the sorted lookups below are never read), as the function does."""
    T, B, H = 2, 3, 2
    widths = [2050, 8]
    group = ce.MixedTableGroup([torch.zeros(5, w, dtype=torch.float16, device="cuda") for w in widths])
    assert group.lane_bytes() == 4
    grad_y = torch.zeros((B, sum(widths)), dtype=torch.float16, device="cuda")
    keys = torch.arange(T * B * H, dtype=torch.int32, device="cuda") % 10
    keys, _ = torch.sort(keys)
    sids = torch.zeros_like(keys)
    remap = torch.unique_consecutive(keys, return_inverse=True)[1].to(torch.int32)
    scatter = torch.ops.cuembed_pyt.cuembed_embedding_backward_mixed_group
    with pytest.raises(RuntimeError, match="the widest table is more than 1024 lanes"):
        scatter(grad_y, widths, group.table_columns_device, keys, sids, remap, None, T * B * H)
    idx = torch.zeros(T, B, H, dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError, match="1024 lanes"):
        ce.embedding_backward_mixed_group(group, grad_y, idx, num_hots=H)
    # without lookups, or without room, the op launches nothing and does not get as far as the limit
    empty = keys[:0]
    rows, ids, overflow = scatter(grad_y, widths, group.table_columns_device, empty, empty, empty, None, 4)
    assert rows.shape == (4, 2050) and ids.shape == (4,) and int(overflow) == 0


def test_fake_implementations_give_shapes_and_dtypes(pyt):
    from torch._subclasses.fake_tensor import FakeTensorMode
    T, D = len(WIDTHS), sum(WIDTHS)
    with FakeTensorMode():
        grad_y = torch.empty((BATCH, D), dtype=torch.float16, device="cuda")
        columns = torch.empty((T, 2), dtype=torch.int32, device="cuda")
        lookups = [torch.empty((40,), dtype=torch.int32, device="cuda") for _ in range(3)]
        rows, ids, overflow = torch.ops.cuembed_pyt.cuembed_embedding_backward_mixed_group(grad_y, list(WIDTHS), columns,
                                                                                           *lookups, None, 33)
        assert tuple(rows.shape) == (33, max(WIDTHS)) and rows.dtype == torch.float16 and rows.device.type == "cuda"
        assert tuple(ids.shape) == (33,) and ids.dtype == torch.int32
        assert tuple(overflow.shape) == (1,) and overflow.dtype == torch.int32
        off = torch.empty((T * BATCH + 1,), dtype=torch.int64, device="cuda")
        out = torch.ops.cuembed_pyt.cuembed_mixed_group_mean_scale(grad_y, list(WIDTHS), columns, off, None, 0)
        assert tuple(out.shape) == (BATCH, D) and out.dtype == torch.float16
