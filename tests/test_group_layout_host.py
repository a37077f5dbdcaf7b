"""The host layer that the entry points on a group of tables share (cuembed_amd.group_layout), without a GPU: the lane
rule of a mixed-width group against BOTH launch-shape functions of the C ABI, one table of bad bag layouts against every
entry point that takes a layout (the messages below are written out here, not taken from the helper), and the common
base of TableGroup and MixedTableGroup."""
import pytest
import torch

DTYPES = (torch.float32, torch.float16, torch.bfloat16)
DEVICE = dict(compute_units=256, xcds=8)
T, B, H, WIDTHS = 2, 3, 2, (4, 8)
ROWS = (5, 7)


@pytest.fixture(scope="module")
def ce():
    import cuembed_amd
    return cuembed_amd


# ---- the lane rule: one truth ------------------------------------------------------------------------------------------

LANE_WIDTHS = [(36, 4, 128), (6, 2, 10), (514,), (128,), (2,), (128, 16, 64, 32), (8, 8),
               tuple(4 * (1 + t % 5) for t in range(65))]


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("widths", LANE_WIDTHS, ids=lambda w: "T%d_w%s" % (len(w), "_".join(map(str, w[:4]))))
def test_the_python_lane_rule_is_the_one_of_both_launch_shape_functions(ce, dtype, widths):
    from cuembed_amd.group_layout import mixed_lane_bytes
    from cuembed_amd.mixed_group_backward import _lane_bytes
    size = dtype.itemsize
    group = ce.MixedTableGroup([torch.zeros(3, w, dtype=dtype) for w in widths])
    seen = set()
    for r0 in (0, 4, 8, 12):
        for r1 in (0, 4, 8, 12):
            p0, p1 = 0x7F0000001000 + r0, 0x7F0000400000 + r1
            lane = mixed_lane_bytes(widths, size, (("a", p0), ("b", p1)))
            seen.add(lane)
            fwd = ce.mixed_group_launch_shape(dtype, torch.int32, widths, B, num_hots=H, pointer_bits=p0 | p1)
            bwd = ce.mixed_group_backward_launch_shape(dtype, widths, 100, pointer_bits=p0 | p1, **DEVICE)
            assert lane == fwd["elems_per_lane"] * size == bwd["elems_per_lane"] * size, (r0, r1)
            assert lane == _lane_bytes(group, ("grad_y", p0), ("rows", p1))
            assert lane in (16, 8, 4) and (p0 | p1) % lane == 0 and all((w * size) % lane == 0 for w in widths)
    assert 4 in seen and max(seen) == mixed_lane_bytes(widths, size)
    # the group's own pointers: lane_bytes is the same function on the tables' bases and `out`
    named = [("tables[%d]" % k, p) for k, p in enumerate(group.host_ptrs)]
    for out_ptr in (0, 0x7F0000001008, 0x7F0000001004):
        assert group.lane_bytes(out_ptr) == mixed_lane_bytes(widths, size, named + [("out", out_ptr)])


def test_the_lane_rule_on_the_cases_the_kernels_split_on(ce):
    from cuembed_amd.group_layout import mixed_lane_bytes
    assert mixed_lane_bytes((36, 4, 128), 2) == 8          # 72-byte rows: c_1 * 2 = 72 is 8 past a 16-byte boundary
    assert mixed_lane_bytes((6, 2, 10), 2) == 4
    assert mixed_lane_bytes((6, 2, 10), 4) == 8
    assert mixed_lane_bytes((514,), 4) == 8
    assert mixed_lane_bytes((128, 16, 64, 32), 2) == 16
    assert mixed_lane_bytes((128,), 4, (("out", 0x1008),)) == 8
    with pytest.raises(ValueError, match="out must be 4-byte aligned: its data pointer is 2 bytes past"):
        mixed_lane_bytes((128,), 4, (("out", 0x1002),))
    with pytest.raises(ValueError, match=r"tables\[1\] must be 4-byte aligned"):
        mixed_lane_bytes((128,), 4, (("tables[0]", 0x1000), ("tables[1]", 0x1003)))


# ---- the bag-layout check: one truth -----------------------------------------------------------------------------------

def meta(n, dtype=torch.int64):   # a tensor of n entries that occupies no memory: the layout checks read size and dtype
    return torch.empty(n, dtype=dtype, device="meta")


IDX = torch.zeros(T * B * H, dtype=torch.int64)
OFF = torch.arange(0, T * B * H + 1, H, dtype=torch.int64)
CSR_XOR = r"either CSR \(offsets given, num_hots == 0\) or fixed hotness \(offsets None, num_hots > 0\)"
BIG = 2 ** 30      # T * BIG = 2^31: one more than fits

# (name, indices, offsets, batch_size, num_hots, exception, message): what every entry point raised before there was one check
BAD_LAYOUTS = [
    ("both", IDX, OFF, None, H, ValueError, CSR_XOR),
    ("neither", IDX, None, None, 0, ValueError, CSR_XOR),
    ("offsets_short", IDX, OFF[:-1], B, 0, ValueError,
     r"offsets must hold num_tables \* batch_size \+ 1 = 7 entries, got 6"),
    ("offsets_long", IDX, torch.zeros(T * B + 2, dtype=torch.int64), B, 0, ValueError,
     r"offsets must hold num_tables \* batch_size \+ 1 = 7 entries, got 8"),
    ("offsets_not_a_multiple", IDX, OFF[:-1], None, 0, ValueError,
     r"offsets must hold num_tables \* batch_size \+ 1 entries: 6 - 1 is not a multiple of 2 tables"),
    ("offsets_empty", IDX, OFF[:0], None, 0, ValueError, r"offsets must hold num_tables \* batch_size \+ 1 entries: 0 - 1"),
    ("offsets_float", IDX, OFF.float(), None, 0, TypeError, "offsets must be int32 or int64, got torch.float32"),
    ("offsets_no_tensor", IDX, OFF.tolist(), None, 0, TypeError, "offsets must be a torch.Tensor"),
    ("indices_not_a_multiple", IDX[:-1], None, None, H, ValueError,
     r"indices.numel\(\) is not a multiple of num_tables \* num_hots"),
    ("indices_short", IDX[:-4], None, B, H, ValueError, r"indices must hold num_tables \* batch_size \* num_hots entries"),
    ("indices_float", IDX.float(), None, None, H, TypeError, "indices must be int32 or int64, got torch.float32"),
    ("indices_no_tensor", IDX.tolist(), None, None, H, TypeError, "indices must be a torch.Tensor"),
    ("bags_past_int_max_csr", IDX, meta(T * BIG + 1), BIG, 0, ValueError,
     r"num_tables \* batch_size = 2147483648 does not fit a 32-bit int"),
    ("bags_past_int_max_fixed", meta(T * BIG), None, BIG, 1, ValueError,
     r"num_tables \* batch_size = 2147483648 does not fit a 32-bit int"),
]
BAD_WEIGHTS = [
    ("weights_dtype", torch.zeros(T * B * H, dtype=torch.float16), TypeError, "weights must be torch.float32, got torch.float16"),
    ("weights_short", torch.zeros(T * B * H - 1), ValueError, "weights must have one entry per index"),
    ("weights_no_tensor", [0.0] * (T * B * H), TypeError, "weights must be a torch.Tensor"),
]


def entry_points(ce):
    """name -> (call(indices, offsets, batch_size, num_hots, weights), takes weights)."""
    same = ce.TableGroup([torch.zeros(rows, 8) for rows in ROWS])
    mixed = ce.MixedTableGroup([torch.zeros(rows, w) for rows, w in zip(ROWS, WIDTHS)])
    gy_same, gy_mixed = torch.zeros(B, T, 8), torch.zeros(B, sum(WIDTHS))
    return {
        "forward_grouped": (lambda i, o, b, h, w=None: ce.embedding_forward_grouped(same, i, o, w, b, h), True),
        "forward_mixed": (lambda i, o, b, h, w=None: ce.embedding_forward_mixed_group(mixed, i, o, w, b, h), True),
        "backward_keys": (lambda i, o, b, h, w=None: ce.grouped_backward_keys(same, i, o, b, h), False),
        "backward_grouped": (lambda i, o, b, h, w=None: ce.embedding_backward_grouped(same, gy_same, i, o, w, b, h), True),
        "backward_mixed": (lambda i, o, b, h, w=None: ce.embedding_backward_mixed_group(mixed, gy_mixed, i, o, w, b, h), True),
        "weight_grad_grouped": (lambda i, o, b, h, w=None: ce.embedding_weight_grad_grouped(same, gy_same, i, o, b, h),
                                False),
    }


ENTRY_POINTS = ("forward_grouped", "forward_mixed", "backward_keys", "backward_grouped", "backward_mixed",
                "weight_grad_grouped")


@pytest.mark.parametrize("entry", ENTRY_POINTS)
def test_every_entry_point_refuses_every_bad_layout_with_the_same_words(ce, entry):
    call, weighted = entry_points(ce)[entry]
    with torch.no_grad():
        for offsets, hot in ((OFF, 0), (None, H)):      # a layout in order gets as far as the device check
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                call(IDX, offsets, None, hot)
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                call(IDX, offsets, B, hot)
        for _, indices, offsets, batch_size, hot, error, message in BAD_LAYOUTS:
            with pytest.raises(error, match=message):
                call(indices, offsets, batch_size, hot)
        if weighted:
            for _, weights, error, message in BAD_WEIGHTS:
                for offsets, hot in ((OFF, 0), (None, H)):
                    with pytest.raises(error, match=message):
                        call(IDX, offsets, None, hot, weights)


def test_the_backward_pipeline_bounds_its_lookups_and_the_forward_does_not(ce):
    calls = entry_points(ce)
    for entry in ("backward_keys", "backward_grouped", "backward_mixed", "weight_grad_grouped"):
        with pytest.raises(ValueError, match=r"2147483648 lookups: the backward pipeline takes at most 2\^31 - 1"):
            calls[entry][0](meta(2 ** 31), meta(T * B + 1), None, 0)
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):
        calls["forward_grouped"][0](meta(2 ** 31), meta(T * B + 1), None, 0)


def test_the_mean_scales_share_the_offsets_part(ce):
    same = ce.TableGroup([torch.zeros(rows, 8) for rows in ROWS])
    mixed = ce.MixedTableGroup([torch.zeros(rows, w) for rows, w in zip(ROWS, WIDTHS)])
    for scale, group, gy in ((ce.grouped_mean_scale, same, torch.zeros(B, T, 8)),
                             (ce.mixed_group_mean_scale, mixed, torch.zeros(B, sum(WIDTHS)))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            scale(group, gy, OFF)
        with pytest.raises(ValueError, match=CSR_XOR):
            scale(group, gy)
        with pytest.raises(ValueError, match=CSR_XOR):
            scale(group, gy, OFF, num_hots=H)
        with pytest.raises(ValueError, match=r"offsets must hold num_tables \* batch_size \+ 1 = 7 entries, got 6"):
            scale(group, gy, OFF[:-1])
        with pytest.raises(TypeError, match="offsets must be int32 or int64"):
            scale(group, gy, OFF.float())
        with pytest.raises(TypeError, match="weights must be torch.float32, got torch.float16"):
            scale(group, gy, weights=torch.zeros(T * B * H, dtype=torch.float16), num_hots=H)
        with pytest.raises(ValueError, match="weights must have one entry per index"):
            scale(group, gy, weights=torch.zeros(T * B * H - 1), num_hots=H)


# ---- one base for both groups ------------------------------------------------------------------------------------------

def test_both_groups_share_their_row_arithmetic_and_neither_is_the_other(ce):
    rows = (5, 0, 7, 300)
    same = ce.TableGroup([torch.zeros(n, 8, dtype=torch.float16) for n in rows])
    mixed = ce.MixedTableGroup([torch.zeros(n, 2 * (k + 1), dtype=torch.float16) for k, n in enumerate(rows)])
    assert same.row_counts == mixed.row_counts == rows
    assert same.row_base == mixed.row_base == (0, 5, 5, 12, 312) and isinstance(mixed.row_base, tuple)
    assert same.total_rows == mixed.total_rows == 312
    assert same.num_tables == mixed.num_tables == len(same) == len(mixed) == 4
    assert same.row_base is same.row_base                     # computed once, not per access
    assert same.row_base_device.tolist() == mixed.row_base_device.tolist() == [0, 5, 5, 12, 312]
    assert same.row_base_device is same.row_base_device and same.row_base_device.dtype == torch.int64
    assert not isinstance(mixed, ce.TableGroup) and not isinstance(same, ce.MixedTableGroup)
    assert type(same).__mro__[1] is type(mixed).__mro__[1]    # ... but one base
    for group in (same, mixed):
        assert group.host_ptrs == tuple(t.data_ptr() for t in group.tables) and group.dtype == torch.float16
        assert group.table_ptrs.tolist() == list(group.host_ptrs) and group.table_ptrs.dtype == torch.int64
        with pytest.raises(ValueError, match="table_ptrs must be the contiguous int64 tensor"):
            type(group)(group.tables, table_ptrs=group.table_ptrs[:-1])
    with pytest.raises(ValueError, match="a TableGroup needs at least one table"):
        ce.TableGroup([])
    with pytest.raises(ValueError, match="a MixedTableGroup needs at least one table"):
        ce.MixedTableGroup([])


def test_the_group_modules_share_their_checks(ce):
    tables = [torch.zeros(rows, 8) for rows in ROWS]
    for make in (ce.EmbeddingBagGroup, ce.MixedEmbeddingBagGroup,
                 lambda t, **kw: ce.QuantizedEmbeddingBagGroup([torch.zeros(4, 16, dtype=torch.uint8)], **kw)):
        with pytest.raises(ValueError, match="mode must be 'sum' or 'mean'"):
            make(tables, mode="max")
        with pytest.raises(ValueError, match="bounds_check must be None, 'raise' or 'repair'"):
            make(tables, bounds_check="clamp")
        bags = make(tables, mode="mean")
        assert bags.mode == "mean" and bags.bounds_check is None and bags.last_check is None
        assert bags.num_tables == bags.group.num_tables
        with pytest.raises(ValueError, match=r"without offsets, idx must be \[num_tables, batch, hotness\]"):
            bags(torch.zeros(4, dtype=torch.int64))
    import inspect
    assert list(inspect.signature(ce.EmbeddingBagGroup.__call__).parameters) == \
        ["self", "idx", "offsets", "weights", "sample_order", "out"]
    assert list(inspect.signature(ce.QuantizedEmbeddingBagGroup.__call__).parameters) == \
        ["self", "idx", "offsets", "weights", "sample_order", "out"]
    assert list(inspect.signature(ce.MixedEmbeddingBagGroup.__call__).parameters) == ["self", "idx", "offsets", "weights", "out"]
    with pytest.raises(TypeError, match="sample_order"):      # refused by the signature, before any check is launched
        ce.MixedEmbeddingBagGroup(tables)(torch.zeros(2, 3, 2, dtype=torch.int64), sample_order=None)


def test_the_grouped_step_still_refuses_the_padded_gradient_of_a_mixed_group(ce):
    """MixedGroupedGrad is a GroupedGrad now; its rows are padded to the widest table, which the grouped step does not
    read: the updaters refuse it as they did, even where the row counts and the width would agree."""
    from cuembed_amd import optim
    same = ce.TableGroup([torch.zeros(rows, 8) for rows in ROWS])
    ids, rows, last = torch.zeros(0, dtype=torch.int32), torch.zeros(0, 8), torch.full((1,), -1, dtype=torch.int32)
    padded = ce.MixedGroupedGrad(ids, rows, last, same.row_base, None, (8, 8))
    assert isinstance(padded, ce.GroupedGrad) and padded.row_base == same.row_base and padded.widths == (8, 8)
    for updater in (optim.GroupSparseUpdater(same, "sgd", 0.1), optim.GroupSparseAdamUpdater(same, 0.1)):
        with pytest.raises(TypeError, match="apply takes the GroupedGrad of embedding_backward_grouped.*MixedGroupedGrad"):
            updater.apply(padded)
        with pytest.raises(ValueError, match="other row counts"):     # a GroupedGrad itself gets as far as the next check
            updater.apply(ce.GroupedGrad(ids, rows, last, (0, 1, 2), None))


def test_the_autograd_batch_of_a_group_keeps_its_own_words(ce):
    from cuembed_amd import cuembed_pyt as P
    from cuembed_amd.group_layout import csr_batch_size
    assert csr_batch_size(2, 7) == 3 and csr_batch_size(2, 1) == 0 and csr_batch_size(2, 6) is None
    assert csr_batch_size(2, 0) is None
    assert P._grouped_batch(T, IDX, OFF) == (B, 0) and P._grouped_batch(T, IDX.view(T, B, H), None) == (B, H)
    with pytest.raises(ValueError, match=r"offsets must hold num_tables \* batch \+ 1 entries$"):
        P._grouped_batch(T, IDX, OFF[:-1])
    with pytest.raises(ValueError, match=r"without offsets, idx must be \[num_tables, batch, hotness\]"):
        P._grouped_batch(T, IDX, None)
