"""The forward on a group of fused 8-bit (bits=4: 4-bit) row-wise tables of DIFFERENT widths in one launch (an extension:
inference only, sum / mean only).

cuembed_amd.mixed_group pools plain tables of any widths into the concatenated [B, D] layout; cuembed_amd.grouped pools
fused 8-bit tables of ONE width.  A served recommendation model wants both at once -- widths that follow the tables'
cardinality, 8 bits because the tables are what fills the memory -- and gets them here:

    bag g = t * B + b        table t, sample b (the mixed group's input layout)
    CSR                      one indices[nnz], one offsets[T * B + 1], optional weights[nnz]
    fixed hotness            indices [T, B, H] (offsets=None, num_hots=H), the same H for every table
    tables                   uint8 [rows_t, W_t + 8]: W_t codes, fp32 scale, fp32 bias (quantize_rows, or torch's
                             quantized::embedding_bag_byte_prepack); bits=4: uint8 [rows_t, W_t / 2 + 4], two codes a
                             byte, fp16 scale, fp16 bias, W_t % 8 == 0 (quantized::embedding_bag_4bit_prepack)
    out                      [B, D] of out_dtype, D = sum of the widths; bag (t, b) at out[b, c_t : c_t + W_t] --
                             torch.cat([embedding_forward_quantized(qtable_t, ..., bits=bits)], dim=1), with the same bits

    QuantizedMixedTableGroup(qtables, bits=8)             the tables, their pointers (host and device) and widths
    embedding_forward_quantized_mixed_group(group, ...)   embedding_forward_quantized on the group, one launch
    quantized_mixed_group_launch_shape(...)               the launch shape (host arithmetic)
    QuantizedMixedEmbeddingBagGroup                       a group with a mode: bags(idx, offsets, weights)

Every function validates its arguments and raises before any launch; the kernel runs on torch's current stream
(cuembed::EmbeddingForwardQuantizedMixedGroup or, for bits=4, EmbeddingForwardQuantized4BitMixedGroup through the C
ABI).  The kernel reads a small per-table descriptor from device memory; the group builds it once per (batch size, codes per lane) -- one host-to-device copy at the FIRST call of
a shape (or at group.descriptor(B, N)), none afterwards -- so with `out=` given every later call copies nothing,
allocates nothing and can be captured into a HIP graph.  There is no backward, no sample_order and no per-table
row-load decision.  A 4-bit table cannot be told from an 8-bit one by its shape: `bits` is given where the group is built
and the group carries it.  A group of 4-bit tables of ONE width is a bits=4 group too: its [B, T * W] result viewed as
[B, T, W] is the stacked layout of cuembed_amd.grouped.
"""
import ctypes

import torch

from . import _lib
from .group_layout import INT_MAX, BagGroupModule, GroupTables
from .grouped import _grouped_args, _grouped_devices
from .ops import _INDEX, _ROW_LOADS, _check_dev, _ptr, _stream
from .quantized import _check_qtable, _format, _out_code, quantize_rows

BLOCK_THREADS = 256        # cuembed::kMixedGroupBlockThreads


def _codes_per_lane(widths, pointer_bits, bits=8):
    """THE rule (detail::QuantizedMixedGroupCodesPerLaneOfBits on the C++ side): the single-table rule on every table.
    bits=4 (detail::Quantized4BitMixedGroupCodesPerLaneOfBits): the largest of 32, 16 and 8 that divides every width --
    a lane's codes are one load at a 4-byte aligned address, so the pointers never narrow it."""
    if bits == 4:
        return 32 if all(w % 32 == 0 for w in widths) else 16 if all(w % 16 == 0 for w in widths) else 8
    if pointer_bits % 8 == 0 and all(w % 8 == 0 for w in widths):
        return 16 if all(w % 16 == 0 for w in widths) else 8
    return 4


def _native(name, bits):
    """The C entry point `name` of the fused 8-bit layout or its `_4bit` sibling (parameter for parameter the same)."""
    return getattr(_lib.lib(), name if bits == 8 else name + "_4bit")


class QuantizedMixedTableGroup(GroupTables):
    """T >= 1 contiguous fused 8-bit tables, uint8 [rows_t, W_t + 8], of one device; the widths W_t (multiples of 4) and
    the row counts may all differ; every base is at least 4-byte aligned.  bits=4: fused 4-bit tables, uint8 [rows_t,
    W_t / 2 + 4], the widths multiples of 8.  Holds the tensors, their base pointers and
    widths on the host, `table_ptrs` (ONE int64 device tensor of the pointers, which the kernel reads) and the device
    descriptors, one per (batch size, codes per lane), each built at its first use.  A group of CPU tensors can be built
    and inspected; calls need the GPU."""

    quantized = True

    def __init__(self, qtables, table_ptrs=None, bits=8):
        self._fmt = _format(bits)        # (before the tables are looked at: _check_table needs it)
        self.bits = bits
        super().__init__(qtables, table_ptrs)
        self.widths = tuple(self._fmt.width_of(t.shape[1]) for t in self.tables)
        base = [0]
        for w in self.widths:
            base.append(base[-1] + w)
        if base[-1] > INT_MAX:
            raise ValueError("the widths sum to %d, which does not fit a 32-bit int" % base[-1])
        self.column_base = tuple(base)
        self._widths_array = (ctypes.c_int * len(self.tables))(*self.widths)
        self._descriptors = {}

    def _first_table(self, first):
        if first.dtype != torch.uint8:
            raise TypeError("tables must be fused uint8 rows %s (quantize_rows), got %s; plain tables go "
                            "into a MixedTableGroup" % (self._fmt.shape.split(" (")[0], first.dtype))

    def _check_table(self, k, t, first):
        try:
            _check_qtable(t, self.bits)
        except (TypeError, ValueError) as e:
            raise type(e)("table %d: %s" % (k, e)) from None

    @classmethod
    def from_float(cls, tables, bits=8):
        """The group of quantize_rows(table, bits=bits) for fp32 / fp16 / bf16 tables [rows_t, W_t] on the device."""
        return cls([quantize_rows(t.detach(), bits=bits) for t in tables], bits=bits)

    @property
    def embedding_dim(self):
        """D: the columns of a result row, the sum of the widths."""
        return self.column_base[-1]

    def codes_per_lane(self):
        """Codes of a row one lane pools (16, 8 or 4), ONE value for the launch, decided by the least aligned table: 16
        when every width is a multiple of 16 and every base 8-byte aligned, 8 when every width is a multiple of 8 and
        every base 8-byte aligned, else 4.  A 4-bit group: 32, 16 or 8, the largest that divides every width, whatever
        the bases' alignment.  The result (16-byte aligned) never narrows it.  ValueError for a base that is not 4-byte
        aligned, where the library would abort."""
        bits = 0
        for k, p in enumerate(self.host_ptrs):
            if p % 4:
                raise ValueError("tables[%d] must be 4-byte aligned: its data pointer is %d bytes past a 4-byte boundary"
                                 % (k, p % 4))
            bits |= p
        return _codes_per_lane(self.widths, bits, self.bits)

    def descriptor_words(self, batch_size, codes_per_lane):
        """The descriptor of (batch_size, codes_per_lane) on the host (cuembed_fill_quantized_mixed_group_descriptor):
        (grid, list of (num_tables + 1) * 4 ints -- per table width, column base, lanes per bag, first workgroup)."""
        T = self.num_tables
        if batch_size < 0 or T * batch_size > INT_MAX:
            raise ValueError("num_tables * batch_size = %d does not fit a 32-bit int" % (T * batch_size))
        lanes = (16, 8, 4) if self.bits == 8 else (32, 16, 8)
        if codes_per_lane not in lanes or codes_per_lane > self.codes_per_lane():
            raise ValueError("codes_per_lane must be %d, %d or %d and at most what the group allows (%d)"
                             % (lanes + (self.codes_per_lane(),)))
        blob = (ctypes.c_int32 * (_lib.lib().cuembed_mixed_group_descriptor_bytes(T) // 4))()
        fill = _native("cuembed_fill_quantized_mixed_group_descriptor", self.bits)
        grid = fill(self._widths_array, T, int(codes_per_lane), int(batch_size), BLOCK_THREADS, blob)
        return grid, list(blob)

    def descriptor(self, batch_size, codes_per_lane):
        """The device descriptor of (batch_size, codes_per_lane): an int32 tensor, built and copied to the device at the
        first use of the pair and kept.  Call it ahead of a graph capture (or run the call once)."""
        key = (int(batch_size), int(codes_per_lane))
        if key not in self._descriptors:
            _, words = self.descriptor_words(*key)
            self._descriptors[key] = torch.tensor(words, dtype=torch.int32, device=self.device)
        return self._descriptors[key]


def _as_quantized_mixed_group(group, bits=None):
    """`group` itself, or the group of a list of fused tables of `bits` (None: 8).  A group carries its bits: a `bits`
    that contradicts them is refused."""
    if isinstance(group, QuantizedMixedTableGroup):
        if bits is not None and bits != group.bits:
            raise ValueError("bits=%r, but the group holds %d-bit tables: bits is for a list of tables" % (bits, group.bits))
        return group
    return QuantizedMixedTableGroup(group, bits=8 if bits is None else bits)


def embedding_forward_quantized_mixed_group(group, indices, offsets=None, weights=None, batch_size=None, num_hots=0,
                                            mode="sum", out_dtype=torch.float16, row_loads=None, out=None,
                                            sample_order=None, row_loads_device=None, bits=None):
    """out[b, c_t : c_t + W_t] = combine_j weights[.] * value(group.tables[t][indices[.]]) over the lookups of bag
    t * batch_size + b, for all tables of a QuantizedMixedTableGroup (or a list of fused tables: a group is then built,
    with its host-to-device copies) in ONE launch.  Returns [batch_size, D] of out_dtype (float16 or float32) --
    torch.cat([embedding_forward_quantized(qtable_t, ..., bits=group.bits)], dim=1), bit for bit.  `bits` (8 or 4) is
    for a list of tables only; a group has its own.

    CSR: offsets[num_tables * batch_size + 1] over one indices[nnz]; fixed hotness: offsets=None, num_hots=H, indices
    [num_tables, batch_size, H].  mode "sum" | "mean"; weights (optional) in out_dtype; fp32 accumulation in lookup order;
    empty bags give zeros.  row_loads ("default" | "streaming" | None, one value for the group) changes no bit.  `out`,
    when given, is 16-byte aligned.  sample_order and row_loads_device must stay None."""
    group = _as_quantized_mixed_group(group, bits)
    oc = _out_code("out_dtype", out_dtype)
    if sample_order is not None:
        raise ValueError("sample_order is not taken by the quantized mixed-width forward in this version")
    batch_size, m, it, ot = _grouped_args(group, indices, offsets, weights, batch_size, num_hots, mode, row_loads, None,
                                          row_loads_device, out_dtype)
    T, D = group.num_tables, group.embedding_dim
    if out is not None:
        if not isinstance(out, torch.Tensor):
            raise TypeError("out must be a torch.Tensor")
        if out.dtype != out_dtype or out.numel() != batch_size * D or not out.is_contiguous():
            raise ValueError("out must be a contiguous %s tensor [batch_size, embedding_dim] = [%d, %d]"
                             % (out_dtype, batch_size, D))
        if out.data_ptr() % 16:
            raise ValueError("out must be 16-byte aligned")
    codes = group.codes_per_lane()
    dev = _grouped_devices(group, indices, offsets, weights)
    if out is None:
        out = torch.empty((batch_size, D), dtype=out_dtype, device=dev)
    else:
        _check_dev("out", out, dev)
    if batch_size > 0:
        descriptor = group.descriptor(batch_size, codes)
        with torch.cuda.device(dev):   # the launch must happen on the tensors' device
            _native("cuembed_embedding_forward_quantized_mixed_group", group.bits)(
                group._host_array, _ptr(group.table_ptrs), group._widths_array, _ptr(descriptor), T, _ptr(indices), it,
                _ptr(offsets), ot, _ptr(weights), batch_size, num_hots, m, _ptr(out), oc, _ROW_LOADS[row_loads],
                _stream(out))
    return out


def quantized_mixed_group_launch_shape(out_dtype, index_dtype, widths, batch_size, num_hots=0, is_weighted=False,
                                       pointer_bits=0, bits=8):
    """Launch shape of a quantized mixed-width forward (pure host arithmetic).  pointer_bits: the table bases OR-ed (0 =
    aligned buffers).  A workgroup of block_threads serves bags of ONE table: table t takes L_t = min(W_t /
    codes_per_lane, block_threads) lanes per bag and block_threads // L_t bags per workgroup; grid = sum_t ceil(
    batch_size / bags per workgroup of t).  num_hots == 0: CSR.  bits=4: widths that are multiples of 8, lanes of 32 / 16
    / 8 codes."""
    fmt = _format(bits)
    oc = _out_code("out_dtype", out_dtype)
    if index_dtype not in _INDEX:
        raise TypeError("index dtype must be int32 or int64, got %s" % index_dtype)
    widths = [int(w) for w in widths]
    T = len(widths)
    if T < 1 or batch_size < 0 or T * batch_size > INT_MAX or num_hots < 0:
        raise ValueError("num_tables >= 1, batch_size >= 0, num_hots >= 0 and num_tables * batch_size must fit a 32-bit int")
    if any(w <= 0 or w % fmt.multiple for w in widths) or sum(widths) > INT_MAX:
        raise ValueError("every width must be a multiple of %d and the widths must sum to at most 2^31 - 1" % fmt.multiple)
    if pointer_bits % 4:
        raise ValueError("every pointer must be 4-byte aligned")
    out = (ctypes.c_int * 7)()
    _native("cuembed_quantized_mixed_group_launch_shape", bits)((ctypes.c_int * T)(*widths), T, oc, _INDEX[index_dtype],
                                                                int(batch_size), int(num_hots), int(bool(is_weighted)),
                                                                int(pointer_bits), out)
    return dict(codes_per_lane=out[0], block_threads=out[1], grid=out[2], embedding_dim=out[3], lds_bytes=out[4],
                staged=out[5] == 1, max_bags_per_block=out[6])


class QuantizedMixedEmbeddingBagGroup(BagGroupModule):
    """A QuantizedMixedTableGroup with a mode, an output dtype and the call shape of nn.EmbeddingBag: bags(idx, offsets,
    weights) with CSR offsets (num_tables * batch + 1 entries), or bags(idx) with idx [num_tables, batch, hotness].
    Returns [batch, embedding_dim].  Inference only.  bounds_check: None (the batch is trusted), "raise" or "repair"
    (cuembed_amd.check_indices in front of the forward, as in MixedEmbeddingBagGroup); the last check is kept as
    .last_check.  from_float quantizes fp32 / fp16 / bf16 tables on the device.  bits (8 or 4): the layout of a list of
    tables; a QuantizedMixedTableGroup has its own."""

    def __init__(self, qtables, mode="sum", out_dtype=torch.float16, bounds_check=None, bits=None):
        super().__init__(mode, bounds_check)
        _out_code("out_dtype", out_dtype)
        self.group = _as_quantized_mixed_group(qtables, bits)
        self.out_dtype = out_dtype

    @classmethod
    def from_float(cls, tables, mode="sum", out_dtype=torch.float16, bounds_check=None, bits=8):
        return cls(QuantizedMixedTableGroup.from_float(tables, bits=bits), mode=mode, out_dtype=out_dtype,
                   bounds_check=bounds_check)

    @property
    def bits(self):
        return self.group.bits

    @property
    def embedding_dim(self):
        return self.group.embedding_dim

    def __call__(self, idx, offsets=None, weights=None, out=None):
        idx, offsets, hot = self._batch(idx, offsets)
        return embedding_forward_quantized_mixed_group(self.group, idx, offsets, weights, num_hots=hot, mode=self.mode,
                                                       out_dtype=self.out_dtype, out=out)
