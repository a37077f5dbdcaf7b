"""The mixed-width grouped forward as a torch op (cuembed_pyt::cuemb_embedding_mixed_group): it exists, gives the same
tensor as the Python call, its fake implementation gives the right shape and dtype, it rejects what the function rejects
-- and the same-width op cuemb_embedding_grouped still refuses mixed widths."""
import numpy as np
import pytest
import torch

import grouped_cases as C

pytestmark = pytest.mark.gpu

ROWS = (5000, 17, 300)
WIDTHS = (36, 4, 128)


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
def problem():
    batch = 5
    tables = [torch.from_numpy(C.table_values(t, ROWS[t], w).astype(np.float16)).cuda() for t, w in enumerate(WIDTHS)]
    layouts = {name: (torch.from_numpy(ids).cuda(), None if off is None else torch.from_numpy(off).cuda(), hot,
                      torch.from_numpy(w.astype(np.float16)).cuda())
               for name, ids, off, hot, w in C.layouts(batch, ROWS)}
    return batch, tables, layouts


def test_the_op_exists_and_agrees_with_the_function(ce, pyt, problem):
    batch, tables, layouts = problem
    assert hasattr(torch.ops.cuembed_pyt, "cuemb_embedding_mixed_group")
    group = ce.MixedTableGroup(tables)
    lane = group.lane_bytes()
    assert lane == 8
    for name, (ids, off, hot, w) in layouts.items():
        idx = ids if off is not None else ids.view(len(tables), batch, hot)
        for mode in ("sum", "mean"):
            for weights in (None, w):
                want = ce.embedding_forward_mixed_group(group, ids, off, weights, num_hots=hot, mode=mode)
                got = pyt.cuemb_embedding_mixed_group(group, idx, off, weights, mode=mode)
                assert got.dtype == want.dtype and got.shape == (batch, sum(WIDTHS)) and torch.equal(got, want), (name, mode)
                raw = torch.ops.cuembed_pyt.cuemb_embedding_mixed_group(tables, group.table_ptrs,
                                                                        group.descriptor(batch, lane), lane, idx, off,
                                                                        weights, mode)
                assert torch.equal(raw, want), (name, mode)


def test_the_op_rejects_what_the_function_rejects(ce, pyt, problem):
    batch, tables, layouts = problem
    group = ce.MixedTableGroup(tables)
    lane = group.lane_bytes()
    descriptor = group.descriptor(batch, lane)
    ids, off, _, _ = layouts["csr_ragged"]
    op = torch.ops.cuembed_pyt.cuemb_embedding_mixed_group
    with pytest.raises(RuntimeError):
        op(tables, group.table_ptrs, descriptor, lane, ids, off, None, "concat")
    with pytest.raises(RuntimeError):     # offsets of a length that is not num_tables * batch + 1
        op(tables, group.table_ptrs, descriptor, lane, ids, off[:-1], None, "sum")
    with pytest.raises(RuntimeError):     # one pointer per table
        op(tables, group.table_ptrs[:2].contiguous(), descriptor, lane, ids, off, None, "sum")
    with pytest.raises(RuntimeError):     # a descriptor of the wrong size
        op(tables, group.table_ptrs, descriptor[:-4].contiguous(), lane, ids, off, None, "sum")
    with pytest.raises(RuntimeError):     # a descriptor filled for another lane width
        op(tables, group.table_ptrs, group.descriptor(batch, 4), 4, ids, off, None, "sum")
    with pytest.raises(RuntimeError):     # weights of another dtype
        op(tables, group.table_ptrs, descriptor, lane, ids, off, torch.ones(ids.numel(), device="cuda"), "sum")
    needs_grad = [t.clone().requires_grad_(True) for t in tables]
    with pytest.raises(RuntimeError):     # forward only
        pyt.cuemb_embedding_mixed_group(ce.MixedTableGroup(needs_grad), ids, off)
    with pytest.raises(RuntimeError):
        ce.embedding_forward_mixed_group(needs_grad, ids, off)
    with torch.no_grad():
        assert torch.equal(pyt.cuemb_embedding_mixed_group(ce.MixedTableGroup(needs_grad), ids, off),
                           ce.embedding_forward_mixed_group(group, ids, off))


def test_the_op_names_its_own_table_rule_and_the_shared_batch_rules(ce):
    """The op's checks are the same-width op's in two parts: the table part with the mixed-width rule and message, the
    batch part as it is.  Two tables of widths (4, 8), 3 bags of 2 lookups each."""
    T, B, H = 2, 3, 2

    def fp16(rows, width):
        return torch.zeros(rows, width, dtype=torch.float16, device="cuda")

    tables = [fp16(5, 4), fp16(7, 8)]
    group = ce.MixedTableGroup(tables)
    lane = group.lane_bytes()
    descriptor = group.descriptor(B, lane)
    idx = torch.zeros(T, B, H, dtype=torch.int64, device="cuda")
    off = torch.arange(0, T * B * H + 1, H, dtype=torch.int64, device="cuda")
    op = torch.ops.cuembed_pyt.cuemb_embedding_mixed_group

    def call(tables=tables, idx=idx, off=None, weights=None):
        ptrs = torch.tensor([t.data_ptr() for t in tables], dtype=torch.int64, device="cuda")
        return op(tables, ptrs, descriptor, lane, idx, off, weights, "sum")

    assert call().shape == (B, 12) and call(idx=idx.view(-1), off=off).shape == (B, 12)      # mixed widths are in order
    mixed_rule = "mixed-width group must be contiguous .* of one dtype and device, every row a multiple of 4 bytes"
    for bad in (fp16(7, 7),                       # 14-byte rows
                fp16(7, 8).float(),               # another dtype
                fp16(7, 16)[:, :8],               # not contiguous
                fp16(7 * 8, 1).view(-1)):         # not [rows, width]
        with pytest.raises(RuntimeError, match=mixed_rule):
            call(tables=[tables[0], bad])
    with pytest.raises(RuntimeError, match=r"offsets must hold num_tables \* batch_size \+ 1 entries"):
        call(idx=idx.view(-1), off=off[:-1])
    with pytest.raises(RuntimeError, match=r"without offsets, indices must be \[num_tables, batch, hotness\]"):
        call(idx=idx.view(-1))
    with pytest.raises(RuntimeError, match="weights have the wrong dtype"):
        call(weights=torch.ones(T * B * H, device="cuda"))
    with pytest.raises(RuntimeError, match="weights must have one entry per index"):
        call(weights=torch.ones(T * B * H - 1, dtype=torch.float16, device="cuda"))
    with pytest.raises(RuntimeError, match="indices must be int32 or int64"):
        call(idx=idx.float())


def test_the_same_width_op_still_refuses_mixed_widths(ce, problem):
    batch, tables, layouts = problem
    ids, off, _, _ = layouts["csr_ragged"]
    ptrs = torch.tensor([t.data_ptr() for t in tables], dtype=torch.int64, device="cuda")
    with pytest.raises(RuntimeError, match="one dtype, width and device"):
        torch.ops.cuembed_pyt.cuemb_embedding_grouped(tables, ptrs, ids, off, None, "sum")
    with pytest.raises(ValueError, match="one width per group"):
        ce.TableGroup(tables)
    with pytest.raises(ValueError, match="one width per group"):
        ce.embedding_forward_grouped(tables, ids, off)


def test_fake_implementation_gives_shape_and_dtype(ce, pyt, problem):
    from torch._subclasses.fake_tensor import FakeTensorMode
    batch, tables, layouts = problem
    T = len(WIDTHS)
    with FakeTensorMode():
        f_tables = [torch.empty((rows, w), dtype=torch.float16, device="cuda") for rows, w in zip(ROWS, WIDTHS)]
        ptrs = torch.empty((T,), dtype=torch.int64, device="cuda")
        descriptor = torch.empty(((T + 1) * 4,), dtype=torch.int32, device="cuda")
        ids = torch.empty((40,), dtype=torch.int32, device="cuda")
        off = torch.empty((T * batch + 1,), dtype=torch.int64, device="cuda")
        fixed = torch.empty((T, batch, 7), dtype=torch.int32, device="cuda")
        for idx, o in ((ids, off), (fixed, None)):
            out = torch.ops.cuembed_pyt.cuemb_embedding_mixed_group(f_tables, ptrs, descriptor, 8, idx, o, None, "sum")
            assert tuple(out.shape) == (batch, sum(WIDTHS)) and out.dtype == torch.float16 and out.device.type == "cuda"
