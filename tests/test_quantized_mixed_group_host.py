"""The quantized mixed-width forward without a GPU: the codes-per-lane rule against a three-line model, the descriptor and
the grid against the same arithmetic in Python, and every refusal of a call, raised before any launch (the tensors live
on the CPU: a call that got as far as the device check raises RuntimeError "no CPU fallback")."""
import ctypes

import pytest
import torch

import cuembed_amd as ce

BLOCK = 256
ROWS = (7, 1000, 64, 300)
# widths -> codes per lane on aligned bases
GROUPS = {(16, 128, 32, 64): 16, (8, 24, 136): 8, (4, 12, 1028, 36): 4, (4112, 16): 16}


def cpu_group(widths, offset_of=None, offset=0):
    """Fused tables of zeros on the CPU, 64-byte aligned, table `offset_of` inside a byte buffer `offset` bytes past
    such a boundary."""
    tables = []
    for t, w in enumerate(widths):
        nbytes = ROWS[t] * (w + 8)
        buf = torch.zeros(nbytes + 128, dtype=torch.uint8)
        first = (-buf.data_ptr()) % 64 + (offset if t == offset_of else 0)
        tables.append(buf[first:first + nbytes].view(ROWS[t], w + 8))
    return ce.QuantizedMixedTableGroup(tables, table_ptrs=torch.zeros(len(widths), dtype=torch.int64))


def codes_model(widths, pointer_bits=0):
    if pointer_bits % 8 or any(w % 8 for w in widths):
        return 4
    return 8 if any(w % 16 for w in widths) else 16


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
    assert n == GROUPS[widths] == codes_model(widths)
    assert group.widths == widths and group.embedding_dim == sum(widths)
    assert group.column_base == tuple(sum(widths[:t]) for t in range(len(widths) + 1))
    assert group.row_counts == ROWS[:len(widths)]
    L, T = ce._lib.lib(), len(widths)
    w_array = (ctypes.c_int * T)(*widths)
    assert L.cuembed_quantized_mixed_group_codes_per_lane(group._host_array, w_array, T) == n
    assert L.cuembed_quantized_mixed_group_codes_per_lane(None, w_array, T) == n
    for batch in (1, 67, 300):
        for lane in (c for c in (16, 8, 4) if c <= n):     # a narrower descriptor is what a misaligned base asks for
            blob = (ctypes.c_int32 * ((T + 1) * 4))()
            grid = L.cuembed_fill_quantized_mixed_group_descriptor(w_array, T, lane, batch, BLOCK, blob)
            assert (grid, list(blob)) == descriptor_model(widths, lane, batch) == group.descriptor_words(batch, lane)
        shape = ce.quantized_mixed_group_launch_shape(torch.float16, torch.int32, widths, batch, num_hots=9)
        most = max(BLOCK // min(w // n, BLOCK) for w in widths)
        assert shape == dict(codes_per_lane=n, block_threads=BLOCK, grid=descriptor_model(widths, n, batch)[0],
                             embedding_dim=sum(widths), lds_bytes=most * 9 * 4, staged=True, max_bags_per_block=most)


def test_one_base_at_a_4_byte_offset_narrows_the_launch_and_staging_follows_the_budget():
    widths = (16, 128, 32, 64)
    assert cpu_group(widths, offset_of=2, offset=8).codes_per_lane() == 16
    group = cpu_group(widths, offset_of=2, offset=4)
    assert group.codes_per_lane() == 4 == codes_model(widths, 4)
    with pytest.raises(ValueError, match="at most what the group allows"):
        group.descriptor_words(5, 16)
    kw = dict(widths=(4, 12, 1028, 36), batch_size=300, num_hots=9)       # one-lane bags: 256 per workgroup
    assert ce.quantized_mixed_group_launch_shape(torch.float16, torch.int32, **kw)["lds_bytes"] == 9216
    assert not ce.quantized_mixed_group_launch_shape(torch.float16, torch.int64, **kw)["staged"]               # 18,432
    assert not ce.quantized_mixed_group_launch_shape(torch.float32, torch.int32, is_weighted=True, **kw)["staged"]


def test_every_refusal_is_raised_before_any_launch():
    widths, B = (16, 128, 32, 64), 5
    group = cpu_group(widths)
    idx = torch.zeros(4 * B * 3, dtype=torch.int32)
    off = torch.arange(0, 4 * B * 3 + 1, 3, dtype=torch.int32)
    call = ce.embedding_forward_quantized_mixed_group

    def refused(error, match, g=group, **kw):
        with pytest.raises(error, match=match):
            call(g, idx, off, **kw)

    with pytest.raises(TypeError, match="fused uint8 rows"):
        ce.QuantizedMixedTableGroup([torch.zeros(3, 24)])
    with pytest.raises(TypeError, match="one dtype per group"):
        ce.QuantizedMixedTableGroup([torch.zeros(3, 24, dtype=torch.uint8), torch.zeros(3, 24)])
    with pytest.raises(ValueError, match="table 1: row size must be a multiple of 4 bytes"):
        ce.QuantizedMixedTableGroup([torch.zeros(3, 24, dtype=torch.uint8), torch.zeros(3, 14, dtype=torch.uint8)])
    with pytest.raises(TypeError, match="float32, float16 or bfloat16"):        # the plain group goes on refusing uint8
        ce.MixedTableGroup([torch.zeros(3, 24, dtype=torch.uint8)])
    refused(ValueError, r"tables\[1\] must be 4-byte aligned", g=cpu_group(widths, offset_of=1, offset=2))
    refused(TypeError, "out_dtype must be torch.float32 or torch.float16", out_dtype=torch.bfloat16)
    refused(TypeError, "weights must be torch.float16", weights=torch.zeros(idx.numel()))
    refused(RuntimeError, "weights require grad", weights=torch.zeros(idx.numel(), dtype=torch.float16, requires_grad=True))
    refused(ValueError, "mode must be 'sum' or 'mean'", mode="concat")
    refused(ValueError, "sample_order is not taken", sample_order=torch.zeros(4 * B, dtype=torch.int32))
    refused(ValueError, "row_loads_device is not taken", row_loads_device=torch.zeros(1, dtype=torch.int32))
    refused(ValueError, "row_loads", row_loads="sometimes")
    refused(ValueError, r"out must be a contiguous torch.float16 tensor \[batch_size, embedding_dim\] = \[5, 240\]",
            out=torch.zeros(B, 240))
    refused(ValueError, r"\[batch_size, embedding_dim\] = \[5, 240\]", out=torch.zeros(B, 239, dtype=torch.float16))
    refused(ValueError, "out must be 16-byte aligned", out=torch.zeros(B * 240 + 8, dtype=torch.float16)[4:-4])
    with pytest.raises(TypeError, match="int32 or int64"):
        call(group, idx.float(), off)
    with pytest.raises(ValueError, match=r"num_tables \* batch_size \+ 1"):
        call(group, idx, off[:-1])
    with pytest.raises(RuntimeError, match="no CPU fallback"):                  # everything in order: now the device
        call(group, idx, off, out=torch.zeros(B, 240, dtype=torch.float16))
    with pytest.raises(ValueError, match="bounds_check"):
        ce.QuantizedMixedEmbeddingBagGroup(group, bounds_check="maybe")
    bags = ce.QuantizedMixedEmbeddingBagGroup(group, mode="mean", out_dtype=torch.float32)
    assert (bags.num_tables, bags.embedding_dim, bags.out_dtype) == (4, 240, torch.float32)
