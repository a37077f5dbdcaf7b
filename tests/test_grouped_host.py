"""Host side of the grouped forward (no GPU): misuse raises a Python exception before any launch, and
grouped_forward_launch_shape is the single-table plan at batch T * B."""
import numpy as np
import pytest
import torch

import grouped_cases as C


@pytest.fixture(scope="module")
def ce():
    import cuembed_amd
    return cuembed_amd


def cpu_tables(width=8, dtype=torch.float32, rows=C.ROWS):
    return [torch.zeros((r, width), dtype=dtype) for r in rows]


def test_a_group_holds_its_tables_and_their_pointers(ce):
    tables = cpu_tables()
    group = ce.TableGroup(tables)
    assert len(group) == group.num_tables == 3 and group.width == 8 and not group.quantized
    assert group.table_ptrs.dtype == torch.int64 and group.table_ptrs.tolist() == [t.data_ptr() for t in tables]
    assert group.host_ptrs == tuple(t.data_ptr() for t in tables)
    q = ce.TableGroup([torch.zeros((r, 16 + 8), dtype=torch.uint8) for r in C.ROWS])
    assert q.quantized and q.width == 16


def test_mismatched_tables_are_refused(ce):
    with pytest.raises(ValueError):
        ce.TableGroup([])
    with pytest.raises(TypeError):
        ce.TableGroup([np.zeros((4, 8), dtype=np.float32)])
    with pytest.raises(ValueError):                                     # widths
        ce.TableGroup(cpu_tables(8)[:2] + cpu_tables(12)[:1])
    with pytest.raises(TypeError):                                      # dtypes
        ce.TableGroup(cpu_tables(8)[:2] + cpu_tables(8, torch.float16)[:1])
    with pytest.raises(TypeError):                                      # plain and fused tables
        ce.TableGroup(cpu_tables(8)[:1] + [torch.zeros((4, 16), dtype=torch.uint8)])
    with pytest.raises(TypeError):
        ce.TableGroup([torch.zeros((4, 8), dtype=torch.int32)])
    with pytest.raises(ValueError):                                     # devices
        ce.TableGroup(cpu_tables(8)[:1] + [torch.empty((4, 8), device="meta")])
    with pytest.raises(ValueError):                                     # contiguity
        ce.TableGroup([torch.zeros((4, 16))[:, ::2]])
    with pytest.raises(ValueError):                                     # a fused row of 6 codes
        ce.TableGroup([torch.zeros((4, 14), dtype=torch.uint8)])
    with pytest.raises(ValueError):                                     # one pointer per table
        ce.TableGroup(cpu_tables(), table_ptrs=torch.zeros((2,), dtype=torch.int64))


@pytest.mark.parametrize("quantized", [False, True], ids=["plain", "quantized"])
def test_misuse_raises_before_any_launch(ce, quantized):
    """(the tables are on the CPU: a call that got as far as the device check would raise RuntimeError instead)"""
    T, B = 3, 4
    if quantized:
        group = ce.TableGroup([torch.zeros((r, 16 + 8), dtype=torch.uint8) for r in C.ROWS])
        fn, w = ce.embedding_forward_quantized_grouped, torch.zeros((24,), dtype=torch.float16)
    else:
        group = ce.TableGroup(cpu_tables())
        fn, w = ce.embedding_forward_grouped, torch.zeros((24,))
    ids = torch.zeros((24,), dtype=torch.int32)
    offsets = torch.arange(0, 2 * (T * B + 1), 2, dtype=torch.int64)
    for mode in ("concat", "max", 2):
        with pytest.raises(ValueError):
            fn(group, ids, offsets, mode=mode)
    with pytest.raises(ValueError):
        fn(group, ids, offsets, row_loads_device=torch.zeros((4,), dtype=torch.int32))
    with pytest.raises(ValueError):
        fn(group, ids, offsets, row_loads="nt")
    with pytest.raises(ValueError):                                     # offsets: T * B + 1 entries
        fn(group, ids, offsets[:-1])
    with pytest.raises(ValueError):
        fn(group, ids, offsets, batch_size=B + 1)
    with pytest.raises(ValueError):                                     # CSR or fixed hotness, not both, not neither
        fn(group, ids, offsets, num_hots=2)
    with pytest.raises(ValueError):
        fn(group, ids)
    with pytest.raises(ValueError):                                     # indices [T, B, H]
        fn(group, ids, num_hots=5)
    with pytest.raises(ValueError):                                     # sample_order is a CSR hint
        fn(group, ids, num_hots=2, sample_order=torch.zeros((12,), dtype=torch.int32))
    with pytest.raises(TypeError):
        fn(group, ids.float(), offsets)
    with pytest.raises(TypeError):                                      # weights of the wrong dtype
        fn(group, ids, offsets, w.double())
    with pytest.raises(ValueError):                                     # one weight per index
        fn(group, ids, offsets, w[:-1])
    with pytest.raises(TypeError):                                      # the other kind of group
        (ce.embedding_forward_grouped if quantized else ce.embedding_forward_quantized_grouped)(group, ids, offsets)
    # T * B past INT_MAX: offsets of 2^31 + 1 entries for a group of one table (a meta tensor: no memory behind it)
    one = ce.TableGroup(group.tables[:1])
    huge = torch.empty((2 ** 31 + 1,), dtype=torch.int64, device="meta")
    with pytest.raises(ValueError, match="32-bit"):
        fn(one, ids, huge)
    # ... and everything in order reaches the device check
    with pytest.raises(RuntimeError, match="GPU"):
        fn(group, ids, offsets)


def test_a_table_that_requires_grad_is_refused_in_grad_mode(ce):
    tables = [t.requires_grad_(True) for t in cpu_tables()]
    ids, offsets = torch.zeros((24,), dtype=torch.int32), torch.arange(0, 26, 2, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="forward only"):
        ce.embedding_forward_grouped(tables, ids, offsets)
    with torch.no_grad(), pytest.raises(RuntimeError, match="GPU"):
        ce.embedding_forward_grouped(tables, ids, offsets)


ELEMS = {torch.float32: 4, torch.float16: 2, torch.bfloat16: 2}


def expected_source(staged, lanes):
    return "lds_staged" if staged else ("wave_shuffle" if lanes <= 64 and 64 % lanes == 0 else "global")


@pytest.mark.parametrize("batch", C.BATCHES, ids=lambda b: "b%d" % b)
@pytest.mark.parametrize("width", [4, 36, 128, 512, 514])
@pytest.mark.parametrize("elem", list(ELEMS), ids=["f32", "f16", "bf16"])
def test_launch_shape_is_the_single_table_plan_at_batch_T_times_B(ce, elem, width, batch):
    T = len(C.ROWS)
    for index in (torch.int32, torch.int64):
        for hot, csr in [(h, False) for h in C.FIXED_HOTS + (4100,)] + [(0, True)]:
            for weighted in (False, True):
                s = ce.grouped_forward_launch_shape(elem, index, width, T, batch, hot, is_csr=csr, is_weighted=weighted)
                row_bytes = width * ELEMS[elem]
                lane = 16 if row_bytes % 16 == 0 else (8 if row_bytes % 8 == 0 else 4)
                assert s["elems_per_lane"] == lane // ELEMS[elem] and s["lanes_per_row"] == row_bytes // lane
                assert s["grid"] == -(-T * batch // s["samples_per_block"])
                per_sample = hot * ((4 if index == torch.int32 else 8) + (ELEMS[elem] if weighted else 0))
                assert s["staged"] == (not csr and per_sample <= 16 * 1024)
                assert s["lds_bytes"] == (s["samples_per_block"] * per_sample if s["staged"] else 0)
                assert s["index_source"] == expected_source(s["staged"], s["lanes_per_row"])
                if csr and s["index_source"] == "wave_shuffle":
                    assert s["samples_per_block"] == 64 // s["lanes_per_row"]       # one wavefront per workgroup
                # the plan of ONE table with T * B samples, minus the kernels the grouped path never takes
                one = ce.forward_launch_shape(elem, index, width, T * batch, hot, is_csr=csr, is_weighted=weighted)
                if not one["wide_load"]:
                    assert (s["samples_per_block"], s["grid"], s["lds_bytes"], s["staged"]) == \
                        (one["samples_per_block"], one["grid"], one["lds_bytes"], one["staged"])


@pytest.mark.parametrize("width,codes", [(4, 4), (8, 8), (40, 8), (256, 16)])
def test_quantized_launch_shape(ce, width, codes):
    T = len(C.ROWS)
    for batch in C.BATCHES:
        for out in (torch.float16, torch.float32):
            for hot, csr in [(7, False), (26, False), (0, True)]:
                s = ce.grouped_forward_launch_shape(out, torch.int32, width, T, batch, hot, is_csr=csr, quantized=True)
                one = ce.quantized_forward_launch_shape(torch.int32, out, width, T * batch, hot, is_csr=csr)
                assert s["elems_per_lane"] == codes == one["codes_per_lane"]
                assert s["grid"] == -(-T * batch // s["samples_per_block"]) == one["grid"]
                assert (s["lanes_per_row"], s["samples_per_block"], s["lds_bytes"], s["staged"]) == \
                    (one["lanes_per_row"], one["samples_per_block"], one["lds_bytes"], one["staged"])
                assert s["index_source"] == expected_source(s["staged"], s["lanes_per_row"])


def test_launch_shape_refuses_what_the_library_would_abort_on(ce):
    with pytest.raises(ValueError):
        ce.grouped_forward_launch_shape(torch.float16, torch.int32, 128, 2, 2 ** 30 + 1, 0, is_csr=True)
    with pytest.raises(ValueError):
        ce.grouped_forward_launch_shape(torch.float16, torch.int32, 128, 0, 8, 0, is_csr=True)
    with pytest.raises(ValueError):
        ce.grouped_forward_launch_shape(torch.float16, torch.int32, 3, 2, 8, 0, is_csr=True)
    with pytest.raises(TypeError):
        ce.grouped_forward_launch_shape(torch.float64, torch.int32, 128, 2, 8, 0, is_csr=True)
    with pytest.raises(TypeError):
        ce.grouped_forward_launch_shape(torch.float16, torch.int16, 128, 2, 8, 0, is_csr=True)
    with pytest.raises(TypeError):
        ce.grouped_forward_launch_shape(torch.bfloat16, torch.int32, 128, 2, 8, 0, is_csr=True, quantized=True)
