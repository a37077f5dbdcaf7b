"""GPU parity of the grouped forward on fused 8-bit tables: bit-identical to T calls of embedding_forward_quantized (whose
bits tests/test_gpu_quantized_forward_bits.py pins) stacked on dim 1, and within the derived bound of
tests/quantized_reference.py::pooled64 (worst_ratio <= 1).  Same tables, batch sizes and bags as
tests/test_gpu_grouped_forward.py; W = 4, 8, 40, 256: 4, 8, 8 and 16 codes per lane."""
import numpy as np
import pytest
import torch

import grouped_cases as C
import quantized_reference as R

pytestmark = pytest.mark.gpu

WIDTHS = (4, 8, 40, 256)
OUTS = {"f16": (torch.float16, np.float16), "f32": (torch.float32, np.float32)}


@pytest.fixture(scope="module")
def ce():
    import cuembed_amd
    assert torch.cuda.is_available()
    return cuembed_amd


_TABLES = {}


def tables_of(width):
    """(fused numpy tables, the same on the device), made once per width and never changed."""
    if width not in _TABLES:
        host = [R.quantize(C.table_values(t, rows, width)) for t, rows in enumerate(C.ROWS)]
        _TABLES[width] = (host, [torch.from_numpy(q).cuda() for q in host])
    return _TABLES[width]


def ibits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


@pytest.mark.parametrize("batch", C.BATCHES, ids=lambda b: "b%d" % b)
@pytest.mark.parametrize("width", WIDTHS, ids=lambda w: "w%d" % w)
@pytest.mark.parametrize("out", list(OUTS))
def test_grouped_quantized_forward_equals_single_table_calls_and_keeps_the_bound(ce, out, width, batch):
    host, dev = tables_of(width)
    group = ce.TableGroup(dev)
    T = len(dev)
    codes = ce.grouped_forward_launch_shape(OUTS[out][0], torch.int32, width, T, batch, 0, is_csr=True,
                                            quantized=True)["elems_per_lane"]
    assert codes == {4: 4, 8: 8, 40: 8, 256: 16}[width]
    for n, (name, ids, offsets, hot, w32) in enumerate(C.layouts(batch)):
        w_host = w32.astype(OUTS[out][1])
        w_dev = torch.from_numpy(w_host).cuda()
        idx_t = (torch.int32, torch.int64)[n % 2]
        off_t = (torch.int64, torch.int32)[(n // 2) % 2]
        d_ids = torch.from_numpy(ids).cuda().to(idx_t)
        d_off = None if offsets is None else torch.from_numpy(offsets).cuda().to(off_t)
        for mode, weighted in C.MODES:
            got = ce.embedding_forward_quantized_grouped(group, d_ids, d_off, w_dev if weighted else None, num_hots=hot,
                                                         mode=mode, out_dtype=OUTS[out][0])
            assert got.shape == (batch, T, width) and got.dtype == OUTS[out][0]
            got_host = got.cpu().numpy()
            for t in range(T):
                i, o, w = C.table_slice(t, batch, ids, offsets, hot, w_host)
                lo = t * batch * hot if offsets is None else int(offsets[t * batch])
                one = ce.embedding_forward_quantized(
                    dev[t], d_ids[lo:lo + i.size].contiguous(),
                    None if o is None else torch.from_numpy(np.ascontiguousarray(o)).cuda().to(off_t),
                    w_dev[lo:lo + i.size].contiguous() if weighted else None, batch_size=batch, num_hots=hot, mode=mode,
                    out_dtype=OUTS[out][0])
                assert torch.equal(ibits(got[:, t]), ibits(one)), (name, mode, weighted, t)
                exact, bound = R.pooled64(host[t], i, o, hot, w if weighted else None, mode=mode, out=out)
                assert R.worst_ratio(got_host[:, t], exact, bound) <= 1.0, (name, mode, weighted, t)
            for hint in (dict(row_loads="streaming"),
                         dict(sample_order=ce.bag_order_by_length(d_off)) if d_off is not None else None):
                if hint is not None:
                    again = ce.embedding_forward_quantized_grouped(group, d_ids, d_off, w_dev if weighted else None,
                                                                   num_hots=hot, mode=mode, out_dtype=OUTS[out][0], **hint)
                    assert torch.equal(ibits(again), ibits(got)), (name, mode, weighted, hint.keys())


@pytest.mark.parametrize("width", [8, 256])
def test_a_4_byte_aligned_table_narrows_the_group(ce, width):
    """One fused table viewed 4 bytes past a 16-byte boundary: 4 codes per lane for the whole group, the same bits."""
    _, dev = tables_of(width)
    t1 = dev[1]
    flat = torch.zeros((t1.numel() + 32,), dtype=torch.uint8, device="cuda")
    first = (4 - flat.data_ptr()) % 16
    moved = flat[first:first + t1.numel()].view(t1.shape)
    moved.copy_(t1)
    assert moved.data_ptr() % 16 == 4
    aligned, narrowed = ce.TableGroup(dev), ce.TableGroup([dev[0], moved, dev[2]])
    assert aligned.lane_bytes() == 8 and narrowed.lane_bytes() == 4
    for batch in (5, 1023):
        for name, ids, offsets, hot, w32 in C.layouts(batch):
            d_ids = torch.from_numpy(ids).cuda()
            d_off = None if offsets is None else torch.from_numpy(offsets).cuda()
            w = torch.from_numpy(w32.astype(np.float16)).cuda()
            for mode, weighted in C.MODES:
                a = ce.embedding_forward_quantized_grouped(aligned, d_ids, d_off, w if weighted else None, num_hots=hot, mode=mode)
                b = ce.embedding_forward_quantized_grouped(narrowed, d_ids, d_off, w if weighted else None, num_hots=hot, mode=mode)
                assert torch.equal(ibits(a), ibits(b)), (batch, name, mode, weighted)
                for t in range(len(dev)):       # ... and those are the bits of the single-table calls
                    i, o, _ = C.table_slice(t, batch, ids, offsets, hot, ids)
                    lo = t * batch * hot if offsets is None else int(offsets[t * batch])
                    one = ce.embedding_forward_quantized(
                        dev[t], d_ids[lo:lo + i.size].contiguous(),
                        None if o is None else torch.from_numpy(np.ascontiguousarray(o)).cuda(),
                        w[lo:lo + i.size].contiguous() if weighted else None, batch_size=batch, num_hots=hot, mode=mode)
                    assert torch.equal(ibits(b[:, t]), ibits(one)), (batch, name, mode, weighted, t)
