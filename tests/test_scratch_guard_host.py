"""The guard harness of tests/scratch_guard.py can fail: on CPU tensors, fake numpy "kernels" that write one byte before
their buffer, one byte past it, or whose result depends on what the buffer held are each reported; a well-behaved one
passes.  No GPU."""
import numpy as np
import pytest
import torch

import scratch_guard as G


def whole_allocation(view):
    """(numpy bytes of the flat allocation behind a guarded view, offset of the view in it)."""
    flat = torch.empty(0, dtype=torch.uint8).set_(view.untyped_storage())
    return flat.numpy(), view.storage_offset() * view.element_size()


def sum_kernel(view, data, before=0, after=0, lazy=False):
    """A fake kernel: a running sum of `data` through `view` as scratch.  lazy: trusts the scratch to start at zero."""
    raw, at = whole_allocation(view)
    scratch = raw[at:at + view.numel() * view.element_size()].view(np.int64)
    if not lazy:
        scratch[:] = 0
    scratch[:data.size] += data
    if before:
        raw[at - before] = 0
    if after:
        raw[at + view.numel() * view.element_size() + after - 1] = 0
    return np.cumsum(scratch[:data.size])


DATA = np.arange(1, 33, dtype=np.int64)


def run(fill, **fault):
    work, check = G.guarded_bytes(8 * DATA.size, fill=fill, device="cpu")
    out = sum_kernel(work, DATA, **fault)
    check("work")
    return (out,)


def test_a_well_behaved_kernel_passes():
    got = G.same_for_every_fill(lambda fill: run(fill))
    assert np.array_equal(got[0], np.cumsum(DATA))


def test_one_byte_before_the_view_is_reported():
    with pytest.raises(AssertionError, match="byte 1 BEFORE the start"):
        run("zeros", before=1)
    with pytest.raises(AssertionError, match="byte 3 BEFORE the start"):
        run("ones", before=3)


def test_one_byte_past_the_view_is_reported():
    with pytest.raises(AssertionError, match="byte 0 PAST the end"):
        run("zeros", after=1)
    with pytest.raises(AssertionError, match="byte %d PAST the end" % (G.GUARD_BYTES - 1)):
        run("random", after=G.GUARD_BYTES)


def test_a_result_that_depends_on_the_fill_is_reported():
    assert np.array_equal(run("zeros", lazy=True)[0], np.cumsum(DATA))      # (right on a fresh allocation)
    with pytest.raises(AssertionError, match="depends on what the workspace held"):
        G.same_for_every_fill(lambda fill: run(fill, lazy=True))


@pytest.mark.parametrize("nbytes", [1, 8, 4096 * 8 + 24])
def test_the_view_has_the_asked_size_alignment_and_fill(nbytes):
    for align in (1, 4, 8, 16):
        for fill, byte in (("zeros", 0), ("ones", 0xFF)):
            view, check = G.guarded_bytes(nbytes, align=align, fill=fill, device="cpu")
            assert view.numel() == nbytes and view.dtype == torch.uint8
            assert view.data_ptr() % align == 0 and view.data_ptr() % (2 * align) != 0    # this alignment and no better
            assert bool((view == byte).all())
            raw, at = whole_allocation(view)
            assert at >= G.GUARD_BYTES and raw.size - at - nbytes >= G.GUARD_BYTES
            assert (raw[:at] == G.SENTINEL).all() and (raw[at + nbytes:] == G.SENTINEL).all()
            check()
    a, _ = G.guarded_bytes(nbytes, fill="random", device="cpu", seed=3)
    b, _ = G.guarded_bytes(nbytes, fill="random", device="cpu", seed=3)
    assert torch.equal(a, b)


def test_typed_outputs():
    out, check = G.guarded_like((5, 3), torch.int64, device="cpu")
    assert out.shape == (5, 3) and out.dtype == torch.int64 and out.data_ptr() % 8 == 0 and out.data_ptr() % 16 != 0
    out[:] = 7
    check("out")
    raw, at = whole_allocation(out)
    raw[at + 5 * 3 * 8] = 1
    with pytest.raises(AssertionError, match="out: byte 0 PAST the end of its 120 bytes"):
        check("out")
    half, check = G.guarded_like(9, torch.float16, device="cpu")
    assert half.numel() == 9 and half.data_ptr() % 4 == 2
    check()
