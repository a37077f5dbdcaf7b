"""Guard bands round scratch buffers and outputs (plain helpers; tests/test_gpu_scratch_confinement.py uses them on the
device, tests/test_scratch_guard_host.py on CPU tensors with fake kernels).

A buffer from guarded_bytes() is a view of EXACTLY the asked size inside one flat allocation.  At least 64 KiB on each
side hold a sentinel byte -- a whole 4,096-key tile of 8-byte keys is 32 KiB, so a kernel that runs one tile past its
plan writes into a guard, not into somebody else's memory -- and check() says where a guard was damaged.  The view
starts at an address that is a multiple of `align` and of nothing larger, so a kernel that assumes a better alignment
than the header promises meets the weakest case.  The view itself holds a fill: zeros, 0xFF or seeded random bytes;
what a call computes must not depend on it (same_for_every_fill)."""
import numpy as np
import torch

GUARD_BYTES = 64 * 1024
SENTINEL = 0xA5
#: the alignment include/cuembed_amd.h promises to accept for `work`: the widest access made to a plan region is one
#: 64-bit word (keys, tile_bits, the state words, the first-flag masks, the row cache's keys and moves)
WORK_ALIGN = 8
FILLS = ("zeros", "ones", "random")
_RANDOM = {}


def fill_bytes(view, fill, seed=0):
    """Overwrite a uint8 view with one of FILLS (random: the same bytes for the same seed and size)."""
    if fill == "zeros":
        view.zero_()
    elif fill == "ones":
        view.fill_(0xFF)
    elif fill == "random":
        key = (seed, str(view.device))
        if key not in _RANDOM:        # (1 MiB of random bytes per seed and device, repeated to the view's length)
            _RANDOM[key] = torch.from_numpy(
                np.random.default_rng(1000 + seed).integers(0, 256, 1 << 20, dtype=np.uint8)).to(view.device)
        pool = _RANDOM[key]
        view.copy_(pool.repeat(-(-view.numel() // pool.numel()))[:view.numel()] if view.numel() > pool.numel()
                   else pool[:view.numel()])
    else:
        raise ValueError("fill must be one of %r, got %r" % (FILLS, fill))
    return view


def _first_damage(guard):
    bad = guard != SENTINEL
    if not bool(bad.any()):
        return None
    return int(torch.nonzero(bad)[0, 0])


def guarded_bytes(nbytes, align=WORK_ALIGN, fill="zeros", device="cuda", seed=0):
    """(view, check): `view` = uint8[nbytes] between two sentinel guards of >= GUARD_BYTES, holding `fill`, at an address
    that is an odd multiple of `align`; check() asserts both guards intact and names the first damaged byte."""
    nbytes = int(nbytes)
    assert nbytes >= 0 and align >= 1 and (align & (align - 1)) == 0
    flat = torch.empty((GUARD_BYTES + 2 * align + nbytes + GUARD_BYTES,), dtype=torch.uint8, device=device)
    flat.fill_(SENTINEL)
    base = flat.data_ptr()
    start = GUARD_BYTES + (align - (base + GUARD_BYTES)) % (2 * align)     # (base + start) % (2 * align) == align
    assert (base + start) % (2 * align) == align % (2 * align) and flat.numel() - (start + nbytes) >= GUARD_BYTES
    view = flat[start:start + nbytes]
    fill_bytes(view, fill, seed)

    def check(what="buffer"):
        front = _first_damage(flat[:start])
        assert front is None, "%s: byte %d BEFORE the start of its %d bytes was written (holds 0x%02x)" % (
            what, start - front, nbytes, int(flat[front]))
        back = _first_damage(flat[start + nbytes:])
        assert back is None, "%s: byte %d PAST the end of its %d bytes was written (holds 0x%02x)" % (
            what, back, nbytes, int(flat[start + nbytes + back]))

    return view, check


def guarded_like(tensor_shape, dtype, device="cuda", fill="random", seed=0):
    """(tensor, check): a typed output of exactly `tensor_shape` elements between two guards, aligned to its element
    size and no better."""
    shape = tuple(int(s) for s in (tensor_shape if isinstance(tensor_shape, (tuple, list, torch.Size)) else (tensor_shape,)))
    item = torch.empty((), dtype=dtype).element_size()
    view, check = guarded_bytes(int(np.prod(shape, dtype=np.int64)) * item, align=item, fill=fill, device=device, seed=seed)
    return view.view(dtype).view(shape), check


def same_for_every_fill(call, fills=FILLS):
    """call(fill) -> tuple of numpy arrays (or None) for every fill; asserts that all fills give the first one's
    arrays bit for bit and returns those."""
    first = None
    for fill in fills:
        got = call(fill)
        if first is None:
            first, first_fill = got, fill
            continue
        assert len(got) == len(first)
        for k, (a, b) in enumerate(zip(first, got)):
            if a is None and b is None:
                continue
            assert a.shape == b.shape and a.dtype == b.dtype
            differ = np.nonzero(a.reshape(-1).view(np.uint8) != b.reshape(-1).view(np.uint8))[0]
            assert differ.size == 0, ("result %d depends on what the workspace held: fill %r and fill %r differ first "
                                      "at byte %d" % (k, first_fill, fill, int(differ[0])))
    return first
