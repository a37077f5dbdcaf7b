"""The mixed-width grouped backward without a GPU: the numpy model of the padded gradient against the CPU oracle's
single-table backward, table by table; every refusal of a call raised before any launch (the tensors here live on the
CPU: a call that got as far as the device check raises RuntimeError "no CPU fallback"); the launch-shape arithmetic
against the single-table plan at W_max; and the names at every layer."""
import os
import re

import numpy as np
import pytest
import torch

import grouped_cases as C
import mixed_group_backward_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = (torch.float32, torch.float16, torch.bfloat16)
DEVICE = dict(compute_units=256, xcds=8)


@pytest.fixture(scope="module")
def ce():
    import cuembed_amd
    return cuembed_amd


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as O
    O.build(ref=False)
    return O


def cpu_group(ce, widths, dtype=torch.float32):
    return ce.MixedTableGroup([torch.zeros(R.ROWS[t], w, dtype=dtype) for t, w in enumerate(widths)])


# ---- the model ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("widths", [(128, 16, 64, 32), (6, 2, 10), (128,)], ids=lambda w: "w" + "_".join(map(str, w)))
@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
def test_the_model_equals_the_oracles_single_table_backward_on_exact_data(oracle, widths, weighted):
    import grouped_backward_cases as G
    rows, batch = R.ROWS[:len(widths)], 5
    base, cols = R.row_base(rows), R.column_base(widths)
    for k, (name, ids, offsets, hot, _) in enumerate(C.layouts(batch, rows=rows)):
        rng = np.random.default_rng(10 * k + weighted)
        gy = R.exact_grad_y(rng, batch, widths, "f32")
        w = G.exact_weights(rng, ids.size) if weighted else None
        got_ids, count, got_rows, valid = R.padded_gradient(widths, rows, batch, ids, offsets, hot, w, gy)
        assert count == got_ids.size == got_rows.shape[0] and got_rows.shape[1] == max(widths) == valid.shape[1]
        assert np.all(np.diff(got_ids) > 0)
        seen = 0
        for t, width in enumerate(widths):
            i_t, o_t, w_t = C.table_slice(t, batch, ids, offsets, hot, np.zeros(ids.size, np.float32) if w is None else w)
            mine = (got_ids >= base[t]) & (got_ids < base[t + 1])
            assert np.array_equal(valid[mine], np.tile(np.arange(max(widths)) < width, (int(mine.sum()), 1)))
            assert not got_rows[mine][:, width:].any()
            if i_t.size == 0:
                assert not mine.any(), (name, t)
                continue
            sid = (oracle.extract_row_ids_from_fixed(batch, hot) if o_t is None
                   else oracle.extract_row_ids_from_csr(o_t.astype(np.int32)))
            ti, ts, tw = oracle.transpose(sid, i_t.astype(np.int32), w_t if weighted else None)
            remap = oracle.compute_compressed_grad_indices(ti)
            unique = int(remap[-1]) + 1
            want, inv = oracle.embedding_backward(np.ascontiguousarray(gy[:, cols[t]:cols[t + 1]]), width, unique, ti, ts,
                                                  remap, tw)
            assert np.array_equal(got_ids[mine] - base[t], inv), (name, t)
            assert np.array_equal(got_rows[mine][:, :width], want.astype(np.float64)), (name, t)
            seen += unique
        assert seen == count, name


# ---- refusals, all before any launch -----------------------------------------------------------------------------------

def test_every_layout_and_dtype_error_is_raised_on_cpu_tensors(ce):
    widths, B = (128, 16, 64, 32), 5
    T, D = len(widths), sum(widths)
    group = cpu_group(ce, widths, torch.float16)
    idx = torch.zeros(T * B * 2, dtype=torch.int64)
    gy = torch.zeros(B, D, dtype=torch.float16)
    call = ce.embedding_backward_mixed_group
    with pytest.raises(RuntimeError, match="no CPU fallback"):       # a call in order gets as far as the device check
        call(group, gy, idx, num_hots=2)
    with pytest.raises(ValueError, match=r"\[batch_size, embedding_dim\]"):
        call(group, gy[:, :-2].contiguous(), idx, num_hots=2)
    with pytest.raises(ValueError, match=r"\[batch_size, embedding_dim\]"):
        call(group, gy.view(B, T, D // T), idx, num_hots=2)
    with pytest.raises(ValueError, match="contiguous"):
        call(group, torch.zeros(D, B, dtype=torch.float16).t(), idx, num_hots=2)
    with pytest.raises(TypeError, match="tables' dtype"):
        call(group, gy.float(), idx, num_hots=2)
    with pytest.raises(TypeError, match="grad_y must be a torch.Tensor"):
        call(group, gy.numpy(), idx, num_hots=2)
    with pytest.raises(ValueError, match="mode must be 'sum' or 'mean'"):
        call(group, gy, idx, num_hots=2, mode="max")
    with pytest.raises(ValueError, match="either CSR"):
        call(group, gy, idx)
    with pytest.raises(ValueError, match="either CSR"):
        call(group, gy, idx, torch.zeros(T * B + 1, dtype=torch.int64), num_hots=2)
    with pytest.raises(ValueError, match=r"num_tables \* batch_size \+ 1"):
        call(group, gy, idx, torch.zeros(T * B, dtype=torch.int64), batch_size=B)
    with pytest.raises(ValueError, match="num_tables . batch_size . num_hots|multiple of"):
        call(group, gy, idx[:-1], num_hots=2)
    with pytest.raises(TypeError, match="int32 or int64"):
        call(group, gy, idx.float(), num_hots=2)
    with pytest.raises(TypeError, match="weights must be torch.float16"):
        call(group, gy, idx, weights=torch.zeros(idx.numel()), num_hots=2)
    with pytest.raises(ValueError, match="one entry per index"):
        call(group, gy, idx, weights=torch.zeros(3, dtype=torch.float16), num_hots=2)
    for bad in (-1, 1.5, True):
        with pytest.raises(ValueError, match="capacity"):
            call(group, gy, idx, num_hots=2, capacity=bad)
    with pytest.raises(TypeError):
        call(ce.TableGroup([torch.zeros(4, 8)]), torch.zeros(1, 8), idx[:1], num_hots=1)
    # the mean scale
    scale = ce.mixed_group_mean_scale
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        scale(group, gy, num_hots=2)
    with pytest.raises(ValueError, match=r"\[batch_size, embedding_dim\]"):
        scale(group, gy.view(B, T, D // T), num_hots=2)
    with pytest.raises(TypeError, match="tables' dtype"):
        scale(group, gy.float(), num_hots=2)
    with pytest.raises(ValueError, match="either CSR"):
        scale(group, gy)
    with pytest.raises(ValueError, match=r"num_tables \* batch_size \+ 1"):
        scale(group, gy, torch.zeros(3, dtype=torch.int32))
    with pytest.raises(TypeError, match="weights must be"):
        scale(group, gy, weights=torch.zeros(T * B * 2), num_hots=2)
    with pytest.raises(ValueError, match="out must be"):
        scale(group, gy, num_hots=2, out=torch.zeros(B, D - 2, dtype=torch.float16))


def test_the_2_to_the_31_limits(ce):
    from cuembed_amd import mixed_group_backward as M
    call = ce.embedding_backward_mixed_group
    group = cpu_group(ce, (2, 2, 2, 2), torch.float16)
    gy = torch.zeros(1, 8, dtype=torch.float16)

    def meta(n):      # a tensor of n entries that occupies no memory: the layout checks read its size and dtype only
        return torch.empty(n, dtype=torch.int32, device="meta")

    with pytest.raises(ValueError, match="does not fit a 32-bit int"):        # T * B: four tables of 2^29 bags each
        call(group, gy, meta(8), meta(4 * 2 ** 29 + 1))
    with pytest.raises(ValueError, match="does not fit a 32-bit int"):
        call(group, gy, meta(4 * 2 ** 29), num_hots=1)
    with pytest.raises(ValueError, match="at most 2\\^31 - 1"):                 # nnz
        call(group, gy, meta(2 ** 31), meta(4 + 1))
    # the staged source offset: B * D * itemsize / lane bytes must stay below 2^31
    wide = cpu_group(ce, (128,), torch.float16)           # 16-byte lanes: 16 lanes per row of grad_y
    M._check_limits(wide, 2 ** 27 - 1, 16)
    with pytest.raises(ValueError, match="31 bits"):
        M._check_limits(wide, 2 ** 27, 16)
    with pytest.raises(ValueError, match="31 bits"):
        M._check_limits(wide, 2 ** 25, 4)                 # the same group behind a 4-byte aligned grad_y: 64 lanes
    with pytest.raises(ValueError, match="31 bits"):      # ... and through the call, before any launch
        call(wide, torch.empty(2 ** 27, 128, dtype=torch.float16, device="meta"), meta(2 ** 27), num_hots=1)
    # W_max: at most 1,024 lanes
    M._check_limits(cpu_group(ce, (8192,), torch.float16), 1, 16)
    with pytest.raises(ValueError, match="1024 lanes"):
        M._check_limits(cpu_group(ce, (8192 + 8,), torch.float16), 1, 16)
    with pytest.raises(ValueError, match="1024 lanes"):
        ce.mixed_group_backward_launch_shape(torch.float32, (4100, 4), 100, **DEVICE)
    with pytest.raises(ValueError, match="nnz"):
        ce.mixed_group_backward_launch_shape(torch.float32, (4,), 2 ** 31, **DEVICE)


# ---- the launch shape --------------------------------------------------------------------------------------------------

def lane_bytes_model(widths, itemsize, pointer_bits=0):
    bits, column = pointer_bits, 0
    for w in widths:
        column += w * itemsize
        bits |= (w * itemsize) | column
    return 16 if bits % 16 == 0 else (8 if bits % 8 == 0 else 4)


@pytest.mark.parametrize("widths", list(R.GROUPS) + [(512, 8), (256, 64, 128)], ids=lambda w: "w" + "_".join(map(str, w)))
def test_the_launch_shape_is_the_single_table_plan_at_the_widest_table(ce, widths):
    for dtype in DTYPES:
        for nnz in (1, 100, 4096, 150_000, 1 << 20, 1 << 22):
            for weighted in (False, True):
                for bits in (0, 8, 4):
                    lane = lane_bytes_model(widths, dtype.itemsize, bits)
                    n = lane // dtype.itemsize
                    s = ce.mixed_group_backward_launch_shape(dtype, widths, nnz, weighted, pointer_bits=bits, **DEVICE)
                    assert s["elems_per_lane"] == n and s["max_width"] == max(widths) and s["embedding_dim"] == sum(widths)
                    assert s["lanes"] * s["column_slices"] == max(widths) // n
                    assert s["lookups_per_block"] == s["segments_per_block"] * s["segment_len"]
                    assert s["segment_len"] % 8 == 0
                    segments = -(-nnz // s["segment_len"])
                    assert s["grid"] >= -(-segments // s["segments_per_block"]) * s["column_slices"]
                    if lane != lane_bytes_model((max(widths),), dtype.itemsize):
                        continue        # (the single-table plan would take wider lanes than the group allows)
                    one = ce.backward_launch_shape(dtype, torch.int32, max(widths), nnz, weighted, **DEVICE)
                    for key in ("column_slices", "lanes", "segments_per_block", "segment_len", "grid"):
                        assert s[key] == one[key], (key, dtype, nnz)
                    # ... plus the lane counts: one uint16 per staged lookup, every segment padded by 4, whole 16 bytes
                    extra = s["segments_per_block"] * (s["segment_len"] + 4) * 2
                    assert s["lds_bytes"] == one["lds_bytes"] + (extra + 15) // 16 * 16
                    assert s["lds_bytes"] <= 64 * 1024


def test_the_launch_shape_obeys_the_backward_tuning(ce):
    try:
        ce.set_backward_tuning(segment_len=8, column_slices=2)
        s = ce.mixed_group_backward_launch_shape(torch.float16, (128, 16, 64, 32), 5000, **DEVICE)
        assert s["segment_len"] == 8 and s["column_slices"] == 2 and s["lanes"] == 8
        s = ce.mixed_group_backward_launch_shape(torch.float16, (36, 4, 128), 5000, **DEVICE)   # 32 lanes of 8 bytes
        assert s["segment_len"] == 8 and s["column_slices"] == 2 and s["lanes"] == 16
    finally:
        ce.set_backward_tuning(segment_len=0, column_slices=0)


# ---- the names ---------------------------------------------------------------------------------------------------------

def test_the_unit_is_built_and_the_names_exist(ce):
    from cuembed_amd import build
    assert "c_api_mixed_group_backward.hip" in build.UNITS
    assert callable(build.build_mixed_group_backward_test)
    cmake = open(os.path.join(ROOT, "CMakeLists.txt")).read()
    assert "c_api_mixed_group_backward.hip" in cmake and "mixed_group_backward_kat" in cmake
    header = open(os.path.join(ROOT, "include", "cuembed_amd.h")).read()
    for name in ("cuembed_embedding_backward_mixed_group", "cuembed_mixed_group_mean_scale",
                 "cuembed_mixed_group_backward_launch_shape"):
        assert re.search(r"\b%s\(" % name, header), name
    for name in ("embedding_backward_mixed_group", "MixedGroupedGrad", "mixed_group_mean_scale",
                 "mixed_group_backward_launch_shape"):
        assert hasattr(ce, name), name
    kernels = open(os.path.join(ROOT, "cuembed_amd", "csrc", "cuembed", "include", "mixed_group_scatter_kernels.hpp")).read()
    assert "MixedGroupScatterAddKernel" in kernels and "MixedGroupMeanScaleKernel" in kernels
    group = cpu_group(ce, (128, 16, 64, 32))
    assert group.table_columns_device.tolist() == [[0, 128], [128, 16], [144, 64], [208, 32]]
    assert group.table_columns_device.dtype == torch.int32


def test_the_forward_still_refuses_tensors_that_require_grad(ce):
    tables = [torch.zeros(4, 8, requires_grad=True), torch.zeros(4, 4)]
    with pytest.raises(RuntimeError, match="forward only"):
        ce.embedding_forward_mixed_group(tables, torch.zeros(2, 1, 1, dtype=torch.int64), num_hots=1)
