"""The mixed-width optimizer step without a GPU: what it refuses and with which words, its launch shape against values
worked out by hand, and the exported names."""
import pytest
import torch

import cuembed_amd as ce
from cuembed_amd import optim

ROWS, WIDTHS = (3, 1, 1, 64, 2), (16, 8, 520, 8, 32)


def group(dtype=torch.float16, rows=ROWS, widths=WIDTHS):
    return ce.MixedTableGroup([torch.zeros((n, w), dtype=dtype) for n, w in zip(rows, widths)])


def gradient(g, n=4, width=None):
    return torch.zeros(n, dtype=torch.int32), torch.zeros((n, width or max(g.widths)), dtype=g.dtype)


def test_stochastic_rounding_is_refused_by_name():
    g = group()
    ids, rows = gradient(g)
    for call in (lambda: ce.sparse_row_update_mixed_group(g, ids, rows, rule="sgd", lr=0.1, stochastic_rounding=True),
                 lambda: ce.sparse_row_adam_mixed_group(g, ids, rows, exp_avg=[], exp_avg_sq=[], lr=0.1, stochastic_rounding=True),
                 lambda: optim.MixedGroupSparseUpdater(g, "sgd", 0.1, stochastic_rounding=True),
                 lambda: optim.MixedGroupSparseAdamUpdater(g, 0.1, stochastic_rounding=True)):
        with pytest.raises(ValueError, match="mixed-width group rounds to nearest: stochastic rounding is not available"):
            call()
    with pytest.raises(ValueError, match="takes one piece: count= or last_id=, not counts="):
        ce.sparse_row_update_mixed_group(g, ids, rows, rule="sgd", lr=0.1, counts=torch.zeros(2, dtype=torch.int32))


@pytest.mark.parametrize("rule, rowwise", [("adagrad", False), ("rowwise_adagrad", True)])
def test_wrong_state_shapes(rule, rowwise):
    g = group()
    ids, rows = gradient(g)
    good = [torch.zeros((n,) if rowwise else (n, w)) for n, w in zip(ROWS, WIDTHS)]
    padded = list(good)
    padded[1] = torch.zeros((2,) if rowwise else (1, 520))      # (a state padded to the widest table is not taken)
    with pytest.raises(ValueError, match=r"states\[1\] must have shape \(1,%s\)" % ("" if rowwise else " 8")):
        ce.sparse_row_update_mixed_group(g, ids, rows, rule=rule, lr=0.1, states=padded)
    with pytest.raises(ValueError, match="states must hold one tensor per table: the group has 5 tables, got 4"):
        ce.sparse_row_update_mixed_group(g, ids, rows, rule=rule, lr=0.1, states=good[:4])
    with pytest.raises(ValueError, match=r"exp_avg_sq\[0\] must have shape \(3, 16\), got \(3,\)"):
        ce.sparse_row_adam_mixed_group(g, ids, rows, exp_avg=[torch.zeros(n, w) for n, w in zip(ROWS, WIDTHS)],
                                       exp_avg_sq=[torch.zeros(n) for n in ROWS], lr=0.1)


def test_rows_must_be_padded_to_the_widest_table():
    g = group()
    ids, rows = gradient(g, width=32)
    with pytest.raises(ValueError, match=r"rows must be \[entries, W_max = 520\], padded to the widest table"):
        ce.sparse_row_update_mixed_group(g, ids, rows, rule="sgd", lr=0.1)
    with pytest.raises(TypeError, match="rows must have the tables' dtype"):
        ce.sparse_row_update_mixed_group(g, ids, gradient(g)[1].float(), rule="sgd", lr=0.1)


def test_the_updaters_take_each_other_s_gradients_no_more_than_before():
    g = group()
    ids, rows = gradient(g)
    last = torch.zeros(1, dtype=torch.int32)
    plain = ce.GroupedGrad(ids, rows, last, g.row_base, None)
    mixed = ce.MixedGroupedGrad(ids, rows, last, g.row_base, None, g.widths)
    with pytest.raises(TypeError, match="apply takes the MixedGroupedGrad of embedding_backward_mixed_group, got GroupedGrad"):
        optim.MixedGroupSparseUpdater(g, "sgd", 0.1).apply(plain)
    with pytest.raises(TypeError, match="apply takes the MixedGroupedGrad of embedding_backward_mixed_group, got GroupedGrad"):
        optim.MixedGroupSparseAdamUpdater(g, 0.1).apply(plain)
    same = ce.TableGroup([torch.zeros((n, 8), dtype=torch.float16) for n in ROWS])
    with pytest.raises(TypeError, match=r"apply takes the GroupedGrad of embedding_backward_grouped\(dense=False\), got "
                                        "MixedGroupedGrad"):
        optim.GroupSparseUpdater(same, "sgd", 0.1).apply(mixed)


def test_more_tables_than_the_staged_words_hold():
    many = ce.MixedTableGroup([torch.zeros((1, 2 + 2 * (t % 2)), dtype=torch.float16) for t in range(1024)])
    ids, rows = gradient(many)
    with pytest.raises(ValueError, match="a grouped step takes at most 1023 tables, the group has 1024"):
        ce.sparse_row_update_mixed_group(many, ids, rows, rule="sgd", lr=0.1)
    with pytest.raises(ValueError, match="a grouped step takes 1 to 1023 tables, got 1024"):
        ce.mixed_group_update_launch_shape(torch.float16, many.widths, 10)


@pytest.mark.parametrize("dtype, widths, rule, entries, want", [
    # fp16 at 16-byte lanes: 8 / 128 / 16 elements are 1 / 16 / 2 lanes; 76 entries are 2 tiles: one workgroup;
    # LDS: 8 * (4 + 3) + 4 * 3 = 68 bytes for SGD
    (torch.float16, (8, 128, 16), "sgd", 76,
     dict(elems_per_lane=8, grid=1, lds_bytes=68, lanes_per_entry=[1, 16, 2], entries_per_pass=[64, 4, 32])),
    # 520 elements are 65 lanes: the whole wavefront on one entry; Adam stages two state tensors: 8 * (6 + 5 * 3) + 20
    (torch.float16, (16, 8, 520, 8, 32), "adam", 71,
     dict(elems_per_lane=8, grid=1, lds_bytes=188, lanes_per_entry=[2, 1, 64, 1, 4], entries_per_pass=[32, 64, 1, 64, 16])),
    # fp32: 260 elements are 65 lanes of 4; one state tensor: 8 * (6 + 5 * 2) + 20
    (torch.float32, (8, 4, 260, 4, 16), "rowwise_adagrad", 1 << 20,
     dict(elems_per_lane=4, grid=2048, lds_bytes=148, lanes_per_entry=[2, 1, 64, 1, 4], entries_per_pass=[32, 64, 1, 64, 16])),
    # a 4-byte row narrows every table to 4-byte lanes: 2 / 130 / 38 bf16 elements are 1 / 65 / 19 lanes (group 32);
    # 257 entries are 5 tiles: two workgroups
    (torch.bfloat16, (2, 130, 38), "adagrad", 257,
     dict(elems_per_lane=2, grid=2, lds_bytes=8 * (4 + 3 * 2) + 12, lanes_per_entry=[1, 64, 32], entries_per_pass=[64, 1, 2])),
])
def test_launch_shape(dtype, widths, rule, entries, want):
    assert ce.mixed_group_update_launch_shape(dtype, widths, entries, rule=rule) == want


def test_launch_shape_follows_the_least_aligned_pointer():
    shape = ce.mixed_group_update_launch_shape(torch.float16, (8, 128, 16), 76, rule="adagrad", pointer_bits=4)
    assert shape["elems_per_lane"] == 2 and shape["lanes_per_entry"] == [4, 64, 8]
    # per-element fp32 state 8 bytes off: 16-byte lanes (8 elements, packs of 16 bytes) and 8-byte lanes (4 elements,
    # packs of 16 bytes) are out, 4-byte lanes (2 elements, packs of 8 bytes) fit
    shape = ce.mixed_group_update_launch_shape(torch.float16, (8, 128, 16), 76, rule="adagrad", state_pointer_bits=8)
    assert shape["elems_per_lane"] == 2


def test_exported_names():
    for name in ("sparse_row_update_mixed_group", "sparse_row_adam_mixed_group", "mixed_group_update_launch_shape"):
        assert callable(getattr(ce, name))
    for name in ("MixedGroupSparseUpdater", "MixedGroupSparseAdamUpdater"):
        assert isinstance(getattr(optim, name), type)
