"""The 4-bit mixed-width forward without a GPU: what a bits=4 group reports, the descriptor and the grid against the same
arithmetic in Python, and every refusal of a call, raised before any launch (the tensors live on the CPU: a call that got
as far as the device check raises RuntimeError "no CPU fallback")."""
import ctypes

import pytest
import torch

import cuembed_amd as ce

BLOCK = 256
ROWS = (7, 1000, 64, 300)
# widths -> codes per lane
GROUPS = {(32, 256, 64, 128): 32, (16, 48, 272): 16, (8, 24, 2056, 40): 8, (8224, 32): 32}


def cpu_group(widths, offset_of=None, offset=0):
    """Fused 4-bit tables of zeros on the CPU, 64-byte aligned, table `offset_of` inside a byte buffer `offset` bytes
    past such a boundary."""
    tables = []
    for t, w in enumerate(widths):
        nbytes = ROWS[t] * (w // 2 + 4)
        buf = torch.zeros(nbytes + 128, dtype=torch.uint8)
        first = (-buf.data_ptr()) % 64 + (offset if t == offset_of else 0)
        tables.append(buf[first:first + nbytes].view(ROWS[t], w // 2 + 4))
    return ce.QuantizedMixedTableGroup(tables, table_ptrs=torch.zeros(len(widths), dtype=torch.int64), bits=4)


def descriptor_model(widths, n, batch):
    words, column, blocks = [], 0, 0
    for w in widths:
        lanes = min(w // n, BLOCK)
        words += [w, column, lanes, blocks]
        column += w
        blocks += -(-batch // (BLOCK // lanes))
    return blocks, words + [0, column, 0, blocks]


@pytest.mark.parametrize("widths", list(GROUPS), ids=lambda w: "w" + "_".join(map(str, w)))
def test_codes_per_lane_descriptor_and_grid(widths):
    group = cpu_group(widths)
    n = group.codes_per_lane()
    assert n == GROUPS[widths] == max(c for c in (32, 16, 8) if all(w % c == 0 for w in widths))
    assert group.bits == 4 and group.widths == widths and group.embedding_dim == sum(widths)
    assert group.column_base == tuple(sum(widths[:t]) for t in range(len(widths) + 1))
    assert cpu_group(widths, offset_of=0, offset=4).codes_per_lane() == n        # alignment never narrows the lane
    L, T = ce._lib.lib(), len(widths)
    w_array = (ctypes.c_int * T)(*widths)
    assert L.cuembed_quantized_mixed_group_codes_per_lane_4bit(group._host_array, w_array, T) == n
    assert L.cuembed_quantized_mixed_group_codes_per_lane_4bit(None, w_array, T) == n
    for batch in (1, 67, 300):
        for lane in (c for c in (32, 16, 8) if c <= n):
            blob = (ctypes.c_int32 * ((T + 1) * 4))()
            grid = L.cuembed_fill_quantized_mixed_group_descriptor_4bit(w_array, T, lane, batch, BLOCK, blob)
            assert (grid, list(blob)) == descriptor_model(widths, lane, batch) == group.descriptor_words(batch, lane)
        shape = ce.quantized_mixed_group_launch_shape(torch.float16, torch.int32, widths, batch, num_hots=9, bits=4)
        most = max(BLOCK // min(w // n, BLOCK) for w in widths)
        assert shape == dict(codes_per_lane=n, block_threads=BLOCK, grid=descriptor_model(widths, n, batch)[0],
                             embedding_dim=sum(widths), lds_bytes=most * 9 * 4, staged=True, max_bags_per_block=most)


def test_every_refusal_is_raised_before_any_launch():
    widths, B = (32, 256, 64, 128), 5
    group = cpu_group(widths)
    idx = torch.zeros(4 * B * 3, dtype=torch.int32)
    off = torch.arange(0, 4 * B * 3 + 1, 3, dtype=torch.int32)
    call = ce.embedding_forward_quantized_mixed_group

    def refused(error, match, g=group, **kw):
        with pytest.raises(error, match=match):
            call(g, idx, off, **kw)

    with pytest.raises(ValueError, match="bits must be 8 or 4"):
        ce.QuantizedMixedTableGroup([torch.zeros(3, 20, dtype=torch.uint8)], bits=2)
    with pytest.raises(TypeError, match=r"fused uint8 rows \[rows, width/2 \+ 4\]"):
        ce.QuantizedMixedTableGroup([torch.zeros(3, 20)], bits=4)
    with pytest.raises(ValueError, match=r"table 1: a fused 4-bit row is whole dwords of codes \(W % 8 == 0\)"):
        ce.QuantizedMixedTableGroup([torch.zeros(3, 20, dtype=torch.uint8), torch.zeros(3, 18, dtype=torch.uint8)], bits=4)
    with pytest.raises(TypeError, match="2-D uint8 tensor"):
        ce.QuantizedMixedTableGroup([torch.zeros(3, 4, 20, dtype=torch.uint8)], bits=4)
    with pytest.raises(ValueError, match="every width must be a multiple of 8"):
        ce.quantized_mixed_group_launch_shape(torch.float16, torch.int32, (32, 12), 5, bits=4)
    with pytest.raises(ValueError, match="codes_per_lane must be 32, 16 or 8"):
        group.descriptor_words(5, 4)
    refused(ValueError, "bits=8, but the group holds 4-bit tables", bits=8)
    refused(ValueError, r"tables\[1\] must be 4-byte aligned", g=cpu_group(widths, offset_of=1, offset=2))
    refused(TypeError, "out_dtype must be torch.float32 or torch.float16", out_dtype=torch.bfloat16)
    refused(TypeError, "weights must be torch.float16", weights=torch.zeros(idx.numel()))
    refused(ValueError, "mode must be 'sum' or 'mean'", mode="concat")
    refused(ValueError, "sample_order is not taken", sample_order=torch.zeros(4 * B, dtype=torch.int32))
    refused(ValueError, "row_loads_device is not taken", row_loads_device=torch.zeros(1, dtype=torch.int32))
    refused(ValueError, r"\[batch_size, embedding_dim\] = \[5, 480\]", out=torch.zeros(B, 479, dtype=torch.float16))
    refused(ValueError, "out must be 16-byte aligned", out=torch.zeros(B * 480 + 8, dtype=torch.float16)[4:-4])
    with pytest.raises(RuntimeError, match="no CPU fallback"):                  # everything in order: now the device
        call(group, idx, off, out=torch.zeros(B, 480, dtype=torch.float16))
    with pytest.raises(RuntimeError, match="no CPU fallback"):                  # a list of tables takes bits=
        call(list(group.tables), idx, off, bits=4)
    bags = ce.QuantizedMixedEmbeddingBagGroup(list(group.tables), mode="mean", out_dtype=torch.float32, bits=4)
    assert (bags.num_tables, bags.embedding_dim, bags.bits) == (4, 480, 4)


def test_the_unit_is_built_and_the_op_has_the_8_bit_schema():
    from cuembed_amd import build, cuembed_pyt  # noqa: F401  (the import defines the ops)
    assert "c_api_quantized_mixed_group_fourbit.hip" in build.UNITS
    name = "cuemb_embedding_quantized_mixed_group"
    schemas = [str(getattr(torch.ops.cuembed_pyt, n).default._schema) for n in (name, name + "_4bit")]
    assert schemas[1] == schemas[0].replace(name, name + "_4bit")
