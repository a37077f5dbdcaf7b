"""The grouped backward without a GPU: row bases, one-storage groups on CPU tensors, and every argument error of the new
entry points raised before a device check.  The old grouped entry points stay forward only."""
import pytest
import torch

import grouped_cases as C


@pytest.fixture(scope="module")
def ce():
    import cuembed_amd
    return cuembed_amd


@pytest.fixture(scope="module")
def pyt():
    from cuembed_amd import cuembed_pyt
    return cuembed_pyt


def cpu_tables(width=8, dtype=torch.float32):
    return [torch.from_numpy(C.table_values(t, rows, width)).to(dtype) for t, rows in enumerate(C.ROWS)]


def test_row_base_is_the_exclusive_prefix_sum(ce):
    group = ce.TableGroup(cpu_tables())
    assert group.row_counts == C.ROWS and isinstance(group.row_counts, tuple)
    assert group.row_base == (0, 5000, 5017, 5317) and isinstance(group.row_base, tuple)
    assert group.total_rows == 5317 and group.flat is None
    dev = group.row_base_device
    assert dev.dtype == torch.int64 and dev.tolist() == list(group.row_base)
    assert group.row_base_device is dev                       # built once
    one = ce.TableGroup(cpu_tables()[1:2])
    assert one.row_base == (0, 17)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
def test_allocate_and_from_flat_share_one_storage(ce, dtype):
    width = 6
    group = ce.TableGroup.allocate(C.ROWS, width, dtype=dtype, device="cpu")
    assert tuple(group.flat.shape) == (sum(C.ROWS), width) and group.flat.dtype == dtype
    assert group.row_counts == C.ROWS and group.num_tables == 3 and not group.quantized
    itemsize = group.flat.element_size()
    for t, rows in enumerate(C.ROWS):
        assert tuple(group.tables[t].shape) == (rows, width)
        assert group.host_ptrs[t] == group.flat.data_ptr() + group.row_base[t] * width * itemsize
        if t:
            assert group.host_ptrs[t] - group.host_ptrs[t - 1] == C.ROWS[t - 1] * width * itemsize
    group.flat[5000 + 3, 2] = 7                               # row 3 of table 1
    assert group.tables[1][3, 2] == 7
    group.tables[2][0, 0] = -2
    assert group.flat[5017, 0] == -2
    # a parameter the caller owns: the views are detached, the parameter is kept
    param = torch.nn.Parameter(torch.zeros(sum(C.ROWS), width, dtype=dtype))
    owned = ce.TableGroup.from_flat(param, C.ROWS)
    assert owned.flat is param and not any(t.requires_grad for t in owned.tables)
    assert owned.host_ptrs[0] == param.data_ptr()
    # fp16 rows of 12 bytes: the second base is only 4-byte aligned, and lane_bytes follows the least aligned pointer
    if dtype == torch.float16:
        assert group.lane_bytes() == 4


def test_one_storage_groups_reject_what_they_cannot_hold(ce):
    with pytest.raises(ValueError):
        ce.TableGroup.from_flat(torch.zeros(10, 4), (3, 3))            # the counts do not add up
    with pytest.raises(ValueError):
        ce.TableGroup.from_flat(torch.zeros(10, 4), (11, -1))
    with pytest.raises(ValueError):
        ce.TableGroup.from_flat(torch.zeros(10, 8)[:, :4], (10,))      # not contiguous
    with pytest.raises(TypeError):
        ce.TableGroup.from_flat(torch.zeros(10, 12, dtype=torch.uint8), (10,))     # quantized
    with pytest.raises(TypeError):
        ce.TableGroup.allocate((10,), 12, dtype=torch.uint8, device="cpu")
    with pytest.raises(ValueError):
        ce.TableGroup.allocate((), 4, device="cpu")


def problem(batch=5, width=8, dtype=torch.float32):
    name, ids, off, hot, w = C.layouts(batch)[3]
    assert name == "csr_ragged"
    grad_y = torch.zeros(batch, len(C.ROWS), width, dtype=dtype)
    return torch.from_numpy(ids), torch.from_numpy(off), grad_y


def test_argument_errors_come_before_any_device_check(ce, pyt):
    """Everything below runs on CPU tensors: a device check would raise RuntimeError("... no CPU fallback ...")."""
    tables = cpu_tables()
    group = ce.TableGroup(tables)
    ids, off, grad_y = problem()
    # int32 keys with 2^31 rows or more: the row counts are faked, nothing that large is allocated
    huge = ce.TableGroup(tables)
    huge.row_counts = (2 ** 31 - 17, 17, 300)
    assert huge.row_base[-1] == 2 ** 31 + 300
    with pytest.raises(ValueError, match="int32 keys"):
        ce.grouped_backward_keys(huge, ids, off, key_dtype=torch.int32)
    edge = ce.TableGroup(tables)
    edge.row_counts = (2 ** 31 - 17, 17, 0)                   # exactly 2^31 rows
    with pytest.raises(ValueError, match="int32 keys"):
        ce.grouped_backward_keys(edge, ids, off, key_dtype=torch.int32)
    with pytest.raises(TypeError):
        ce.grouped_backward_keys(group, ids, off, key_dtype=torch.int16)
    # a quantized group
    qgroup = ce.TableGroup([torch.zeros(rows, 16, dtype=torch.uint8) for rows in C.ROWS])
    with pytest.raises(TypeError, match="8-bit"):
        ce.grouped_backward_keys(qgroup, ids, off)
    with pytest.raises(TypeError, match="8-bit"):
        ce.embedding_backward_grouped(qgroup, grad_y, ids, off)
    with pytest.raises(TypeError, match="8-bit"):
        pyt.cuemb_embedding_grouped_trainable(qgroup, ids, off)
    # grad_y of the wrong shape or dtype
    with pytest.raises(ValueError, match="grad_y"):
        ce.embedding_backward_grouped(group, grad_y[:, :2].contiguous(), ids, off)
    with pytest.raises(ValueError, match="grad_y"):
        ce.embedding_backward_grouped(group, grad_y.view(5 * 3, 8), ids, off)
    with pytest.raises(ValueError, match="contiguous"):
        ce.embedding_backward_grouped(group, torch.zeros(3, 5, 8).transpose(0, 1), ids, off)
    with pytest.raises(TypeError, match="grad_y"):
        ce.embedding_backward_grouped(group, grad_y.half(), ids, off)
    # reference_sums without dense
    with pytest.raises(ValueError, match="reference_sums"):
        ce.embedding_backward_grouped(group, grad_y, ids, off, reference_sums=True)
    # the layout
    with pytest.raises(ValueError):
        ce.grouped_backward_keys(group, ids, off[:-1])
    with pytest.raises(ValueError):
        ce.grouped_backward_keys(group, ids, off, num_hots=3)
    with pytest.raises(ValueError):
        ce.grouped_backward_keys(group, ids)
    with pytest.raises(TypeError):
        ce.grouped_backward_keys(group, ids.float(), off)
    with pytest.raises(TypeError):
        ce.embedding_backward_grouped(group, grad_y, ids, off, weights=torch.zeros(ids.numel(), dtype=torch.float16))
    with pytest.raises(ValueError):
        ce.grouped_backward_keys(group, ids, off, out=(torch.zeros(3, dtype=torch.int32),) * 2)
    # the autograd surface
    needs_grad = [t.clone().requires_grad_(True) for t in tables]
    with pytest.raises(ValueError, match="padded"):
        pyt.cuemb_embedding_grouped_trainable(ce.TableGroup(needs_grad), ids, off, sparse_grad="padded")
    with pytest.raises(ValueError, match="padded"):
        pyt.TrainableEmbeddingBagGroup(ce.TableGroup(needs_grad), sparse_grad="padded")
    weights = torch.ones(ids.numel(), requires_grad=True)
    with pytest.raises(ValueError, match="weight gradient"):
        pyt.cuemb_embedding_grouped_trainable(ce.TableGroup(needs_grad), ids, off, weights)
    for bad in ("blocked", "fastest", 1, None):
        with pytest.raises(ValueError, match="sparse_grad"):
            pyt.cuemb_embedding_grouped_trainable(ce.TableGroup(needs_grad), ids, off, sparse_grad=bad)
    # table cuts
    base = group.row_base_device
    with pytest.raises(ValueError):
        ce.grouped_table_cuts(ids, base, count=3, last_id=ids[:1])
    with pytest.raises(ValueError):
        ce.grouped_table_cuts(ids, base, count=ids.numel() + 1)
    with pytest.raises(TypeError):
        ce.grouped_table_cuts(ids, base, last_id=ids[:1].int())
    with pytest.raises(TypeError):
        ce.grouped_table_cuts(ids, base.int())
    # ... and a call that is in order reaches the device check
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ce.grouped_backward_keys(group, ids, off)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ce.embedding_backward_grouped(group, grad_y, ids, off)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ce.grouped_table_cuts(ids, base)


def test_the_old_entry_points_stay_forward_only(ce, pyt):
    needs_grad = [t.clone().requires_grad_(True) for t in cpu_tables()]
    ids, off, _ = problem()
    with pytest.raises(RuntimeError, match="forward only"):
        ce.embedding_forward_grouped(needs_grad, ids, off)
    with pytest.raises(RuntimeError, match="forward only"):
        pyt.cuemb_embedding_grouped(ce.TableGroup(needs_grad), ids, off)
    with pytest.raises(RuntimeError, match="forward only"):
        ce.EmbeddingBagGroup(needs_grad)(ids, off)


def test_the_trainable_module_registers_its_parameters(ce, pyt):
    param = torch.nn.Parameter(torch.zeros(sum(C.ROWS), 8))
    bags = pyt.TrainableEmbeddingBagGroup(ce.TableGroup.from_flat(param, C.ROWS), sparse_grad="padded")
    assert [p is param for p in bags.parameters()] == [True]
    assert bags.num_tables == 3 and bags.embedding_dim == 8
    tables = [torch.nn.Parameter(t) for t in cpu_tables()]
    tables[1].requires_grad_(False)
    separate = pyt.TrainableEmbeddingBagGroup(ce.TableGroup(tables))
    assert len(list(separate.parameters())) == 3


def test_the_new_unit_and_symbols_are_declared(ce):
    from cuembed_amd import build
    assert "c_api_grouped_backward.hip" in build.UNITS
    lib = ce._lib.lib()
    assert hasattr(lib, "cuembed_grouped_backward_keys") and hasattr(lib, "cuembed_grouped_table_cuts")
