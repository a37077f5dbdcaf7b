"""ops._check_alignment against the three native dispatchers, read off their source (no GPU, integers only).

The rows of the tables below are derived by hand from

  * SplitRow                 cuembed_amd/csrc/cuembed/include/embedding_lookup.hpp:144-163
        bits = p0 | p1 | row_bytes; 16 if bits % 16 == 0, else 8 if bits % 8 == 0, else 4 (:149-153);
        aborts unless p0 % 4 == 0 and p1 % 4 == 0 (:154-155), row_bytes % 4 == 0 (:148) and
        width / (bytes / sizeof(ElemT)) <= kMaxBlockThreads = 1024 (:159; gather_reduce_kernels.hpp:41);
  * UpdateLaneBytes          cuembed_amd/csrc/cuembed/include/sparse_update.hpp:57-74
        the same bits over table | rows | row_bytes (:63-65); per-element fp32 state narrows the lane while
        state % (4 * min(bytes / sizeof(ElemT), 4)) != 0 (:68-70) and aborts if the 4-byte lane still does not fit
        (:71).  No lane limit: PlanUpdate (:84-96) loops over rows wider than its lane group;
  * QuantizedCodesPerLane    cuembed_amd/csrc/cuembed/include/quantized_lookup.hpp:34-38
        8 if width % 8 == 0 and table % 8 == 0, else 4; aborts unless table % 4 == 0 (:36) and width % 4 == 0 (:35);
        DequantizeRows (:177-178) and PlanQuantizedForward (:71-72) abort above 1024 lanes; QuantizeRows (:145-148) loops.
"""
import pytest

from cuembed_amd import ops

BASE = 0x7F0000000000            # a 16-byte (and far more) aligned address

# (element size, width, residues of the data pointers mod 16) -> lane bytes, or None = rejected
SPLIT_ROW = [
    # fp32
    (4, 4, (0, 0), 16), (4, 4, (8, 0), 8), (4, 4, (0, 4), 4), (4, 4, (12, 8), 4),
    (4, 2, (0, 0), 8), (4, 1, (0, 0), 4), (4, 6, (0, 0), 8), (4, 6, (4, 0), 4),
    (4, 64, (0, 0), 16), (4, 64, (8, 8), 8), (4, 64, (4, 8), 4), (4, 64, (12, 12), 4),
    (4, 4096, (0, 0), 16),            # exactly 1024 lanes of 16 bytes: accepted
    (4, 4096, (8, 0), None),          # 2048 lanes of 8 bytes
    (4, 4104, (0, 0), None),          # 1026 lanes of 16 bytes: rejected at any alignment
    (4, 2048, (8, 0), 8),             # exactly 1024 lanes of 8 bytes: accepted
    (4, 2052, (0, 0), 16),            # 513 lanes
    (4, 2052, (8, 0), None),          # 1026 lanes of 8 bytes: rejected
    (4, 1024, (4, 0), 4),             # exactly 1024 lanes of 4 bytes: accepted
    (4, 1028, (0, 0), 16),            # 257 lanes
    (4, 1028, (0, 4), None),          # 1028 lanes of 4 bytes
    (4, 1026, (0, 0), 8),             # 513 lanes
    (4, 1026, (4, 0), None),          # 1026 lanes of 4 bytes: rejected
    (4, 1025, (0, 0), None),          # the row size allows 4-byte lanes only: 1025 lanes at any alignment
    # 16-bit
    (2, 8, (0, 0), 16), (2, 8, (8, 0), 8), (2, 8, (4, 0), 4), (2, 8, (0, 12), 4),
    (2, 4, (0, 0), 8), (2, 2, (0, 0), 4), (2, 6, (0, 0), 4), (2, 12, (0, 0), 8),
    (2, 512, (4, 0), 4),              # 256 lanes of 4 bytes: one sample per workgroup
    (2, 2048, (4, 0), 4),             # exactly 1024 lanes of 4 bytes: accepted
    (2, 2052, (0, 0), 8),             # 4104 bytes: 513 lanes of 8
    (2, 2052, (8, 8), 8),
    (2, 2052, (4, 0), None),          # 1026 lanes of 4 bytes: rejected
    (2, 8192, (0, 0), 16),            # exactly 1024 lanes of 16 bytes
    (2, 8192, (0, 8), None),
    (2, 8, (2, 0), None), (2, 8, (0, 6), None), (2, 8, (10, 0), None), (2, 8, (14, 14), None),   # % 4 == 2: rejected
    (2, 3, (0, 0), None),             # 6-byte rows
    (4, 0, (0, 0), None),
]


@pytest.mark.parametrize("size,width,residues,lane", SPLIT_ROW)
def test_split_row_and_update_lane_bytes(size, width, residues, lane):
    args = ("params", BASE + residues[0], size, width, (("out", BASE + 4096 + residues[1]),))
    if lane is None:
        with pytest.raises(ValueError):
            ops._check_alignment(*args)
    else:
        assert ops._check_alignment(*args) == lane
        assert width * size // lane <= ops.MAX_LANES_PER_ROW == 1024
    # UpdateLaneBytes: the same lane, and no limit on the lanes of a row
    if width > 0 and (width * size) % 4 == 0 and all(r % 4 == 0 for r in residues):
        bits = residues[0] | residues[1] | (width * size)
        want = 16 if bits % 16 == 0 else (8 if bits % 8 == 0 else 4)
        assert ops._check_alignment(*args, max_lanes=None) == want
        assert lane in (None, want)
    else:
        with pytest.raises(ValueError):
            ops._check_alignment(*args, max_lanes=None)


def test_messages_name_the_tensor_and_the_alignment_that_fits():
    with pytest.raises(ValueError, match=r"out must be 4-byte aligned"):
        ops._check_alignment("params", BASE, 2, 8, (("out", BASE + 2),))
    with pytest.raises(ValueError, match=r"1026 lanes of 4 bytes.*8-byte aligned data \(grad_y\)"):
        ops._check_alignment("params", BASE, 2, 2052, (("grad_y", BASE + 4),))
    with pytest.raises(ValueError, match=r"1028 lanes of 4 bytes.*8-byte aligned data \(params\)"):
        ops._check_alignment("params", BASE + 4, 4, 1028, (("out", BASE),))
    with pytest.raises(ValueError, match=r"2048 lanes of 4 bytes.*8-byte aligned data \(qtable\)"):
        ops._check_alignment("qtable", BASE + 4, 1, 8192, codes=True)
    with pytest.raises(ValueError, match="multiple of 4 bytes"):
        ops._check_alignment("params", BASE, 2, 3)


# (element size, width, table residue, rows residue, state residues) -> lane bytes, or None = rejected
UPDATE_STATE = [
    # fp32 table: a lane of N elements moves 4 * N bytes of state
    (4, 8, 0, 0, (0,), 16), (4, 8, 0, 0, (8,), 8), (4, 8, 0, 0, (4,), 4), (4, 8, 0, 0, (12,), 4),
    (4, 8, 8, 0, (0,), 8), (4, 8, 8, 0, (4,), 4), (4, 8, 4, 0, (0,), 4), (4, 8, 0, 0, (0, 8), 8), (4, 8, 0, 0, (8, 4), 4),
    # 16-bit table: 16-byte lanes are 8 elements (16 bytes of state at a time), 8-byte lanes 4 (16), 4-byte lanes 2 (8)
    (2, 8, 0, 0, (0,), 16), (2, 8, 0, 0, (8,), 4), (2, 8, 8, 0, (0,), 8), (2, 8, 8, 0, (8,), 4), (2, 8, 4, 0, (8,), 4),
    (2, 8, 0, 0, (0, 8), 4),
    (2, 8, 0, 0, (4,), None), (2, 8, 0, 0, (12,), None), (2, 8, 4, 4, (4,), None), (2, 8, 0, 0, (0, 4), None),
    # a state cannot narrow a row into rejection: the update kernels loop (fp32 W = 2048 at 4-byte lanes: 2048 lanes)
    (4, 2048, 0, 0, (4,), 4),
]


@pytest.mark.parametrize("size,width,table,rows,state,lane", UPDATE_STATE)
def test_update_lane_bytes_with_per_element_state(size, width, table, rows, state, lane):
    kw = dict(others=(("rows", BASE + 8192 + rows),), state=tuple(("state%d" % k, BASE + 65536 * (k + 1) + r)
                                                                   for k, r in enumerate(state)), max_lanes=None)
    if lane is None:
        with pytest.raises(ValueError, match="state.* must be 8-byte aligned"):
            ops._check_alignment("table", BASE + table, size, width, **kw)
    else:
        assert ops._check_alignment("table", BASE + table, size, width, **kw) == lane


# (width, table residue mod 16) -> codes per lane of the dequantizer / quantizer, or None = rejected
QUANTIZED = [
    (4, 0, 4), (8, 0, 8), (8, 8, 8), (8, 4, 4), (8, 12, 4), (12, 0, 4), (36, 0, 4), (64, 4, 4), (64, 8, 8), (256, 12, 4),
    (4096, 4, 4),                     # exactly 1024 lanes of 4 codes: accepted
    (4100, 0, None),                  # 1025 lanes of 4 codes at any alignment
    (4104, 0, 8), (4104, 4, None),    # 513 lanes of 8; 1026 lanes of 4: rejected
    (8192, 0, 8), (8192, 8, 8),       # exactly 1024 lanes of 8 codes: accepted
    (8192, 4, None), (8192, 12, None),
    (8200, 0, None),
    (8, 2, None), (8, 6, None), (8, 1, None),     # % 4 != 0: rejected
    (6, 0, None),
]


@pytest.mark.parametrize("width,residue,codes", QUANTIZED)
def test_quantized_codes_per_lane(width, residue, codes):
    if codes is None:
        with pytest.raises(ValueError):
            ops._check_alignment("qtable", BASE + residue, 1, width, codes=True)
    else:
        assert ops._check_alignment("qtable", BASE + residue, 1, width, codes=True) == codes
    # the quantizer's lane groups loop over the row: only the 4-byte rules remain
    if width % 4 == 0 and residue % 4 == 0:
        assert ops._check_alignment("out", BASE + residue, 1, width, codes=True, max_lanes=None) == \
            (8 if width % 8 == 0 and residue % 8 == 0 else 4)


def test_every_entry_point_checks_before_it_reaches_the_library():
    """The eight Python entry points that hand a data pointer to one of the three dispatchers call the helper before
    their first _lib.lib() (source order; an entry point that lost its check would abort the process instead)."""
    import inspect
    from cuembed_amd import quantized
    for fn in (ops.embedding_forward, ops.embedding_weight_grad, ops.embedding_backward, ops.sparse_row_update,
               ops.sparse_row_adam, quantized.quantize_rows, quantized.dequantize_rows,
               quantized.embedding_forward_quantized):
        src = inspect.getsource(fn)
        assert "_check_alignment(" in src and "_lib.lib()" in src, fn.__name__
        assert src.index("_check_alignment(") < src.index("_lib.lib()"), fn.__name__
