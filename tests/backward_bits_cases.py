"""Cases and inputs of the backward's fingerprints (test_gpu_backward_bits.py, test_backward_bits_host.py).  Not a
test module: numpy only, integer arithmetic (a multiplicative hash), no random generator.

A case is one call of cuembed_amd.embedding_backward under a forced launch shape.  Its sorted COO is built here from a
list of run lengths laid out against the launch shape (segment_len lookups per segment, segments_per_block segments per
workgroup), so that where every run starts and ends relative to segments and workgroups is known on the host.

Two kinds of data.  Rows that several workgroups contribute to receive hardware float atomics; three contributions onto
zero, or two onto a stored value, round differently by arrival order.  ARBITRARY data (hashed fp32 values with 24
significant bits, hashed weights in (0, 1)) therefore never has a run longer than one workgroup's lookups, nor -- in
sample blocks after the first -- a run of a row that an earlier block stored crossing a workgroup boundary.  EXACT data
(values -1, 0, 1 and -2, 0, 2, weights 0.5 / 0.25, sample ids that make every aligned triple of a run cancel, so that
every partial sum is representable in bf16 too) may do both and must also equal the CPU oracle.
test_backward_bits_host.py asserts these conditions for every case."""
import collections

import numpy as np

BATCH = 510            # rows of grad_y: a multiple of 3 (the exact data cancels in triples of consecutive samples)
PATTERN = -1.75        # what both output buffers hold before the call (representable in every type)
INVERSE_PATTERN = -5
TILE = 4096            # keys per tile of the sort: sample blocks are whole tiles, inputs of up to 32 tiles are one block
BLOCKED_NNZ = 33 * TILE + 77
MASK = np.uint64(0xFFFFFFFF)

Case = collections.namedtuple("Case", "kind index width weighted segment_len slices data out blocks nnz")
# kind f32 / f16 / bf16; index i32 / i64; data "arb" / "exact"; blocks: sample blocks (1 = a fully sorted COO);
# nnz: None = as long as the layout of runs needs, else exactly that many lookups (the tiny cases);
# out: dense    the dense gradient
#      known    compressed, the row count known on the host
#      fit / over / small   compressed, num_grad_embedding_rows=None: buffers of exactly the rows, five more, one fewer
#      pad      ... 37 more and pad_to_capacity=True
#      skip     compressed, skip_grad_init=True on a zeroed buffer
ELEM_BYTES = {"f32": 4, "f16": 2, "bf16": 2}
WIDTHS = {"f32": (1, 3, 6, 32, 128, 1028), "f16": (2, 6, 12, 64, 256, 2056), "bf16": (2, 6, 12, 64, 256, 2056)}
SEGMENT_LENS = (8, 24, 32, 128)


def case_id(c):
    return "-".join([c.kind, c.index, "W%d" % c.width, "weighted" if c.weighted else "plain", "L%d" % c.segment_len,
                     "S%d" % c.slices, c.data, c.out, "P%d" % c.blocks] + (["n%d" % c.nnz] if c.nnz else []))


def lanes_of(kind, width):
    row_bytes = width * ELEM_BYTES[kind]
    return row_bytes // (16 if row_bytes % 16 == 0 else 8 if row_bytes % 8 == 0 else 4)


def all_cases():
    cases = []
    n = 0
    for kind in ("f32", "f16", "bf16"):
        for width in WIDTHS[kind]:
            sliced = [s for s in (2, 4, 8) if lanes_of(kind, width) % s == 0] or [1]
            for k, (seg, slices) in enumerate(((SEGMENT_LENS[n % 4], 1), (SEGMENT_LENS[(n + 1) % 4], sliced[(n + len(kind)) % len(sliced)]))):
                for data in ("arb", "exact"):
                    cases.append(Case(kind, "i32", width, (n + k) % 2 == 1, seg, slices, data,
                                      "dense" if (n + k) % 3 == 0 else "known", 1, None))
            n += 1
    mid = {"f32": 32, "f16": 64, "bf16": 64}
    for kind in ("f32", "f16", "bf16"):
        for data in ("arb", "exact"):
            cases.append(Case(kind, "i64", mid[kind], data == "arb", 32, 1, data, "known", 1, None))
            cases.append(Case(kind, "i64", mid[kind], data == "exact", 24, 2, data, "dense", 1, None))
    for n, out in enumerate(("fit", "over", "small", "pad", "skip")):
        for kind in ("f16", "f32"):
            cases.append(Case(kind, "i32", mid[kind], n % 2 == 0, (8, 32)[n % 2], (1, 4)[kind == "f16"], "arb", out, 1, None))
        cases.append(Case("bf16", "i64" if out == "fit" else "i32", 64, n % 2 == 1, 24, 1, "exact", out, 1, None))
    for nnz in (1, 3, 7, 8 * 24 + 5):     # one lookup, below either window depth, not a multiple of anything
        cases.append(Case("f32", "i32", 32, False, 24, 1, "arb", "known", 1, nnz))
        cases.append(Case("f16", "i32", 64, True, 8, 2, "arb", "dense", 1, nnz))
    for blocks in (2, 3):
        for kind in ("f32", "f16", "bf16"):
            for data in ("arb", "exact"):
                seg = SEGMENT_LENS[(blocks + len(kind) + len(data)) % 4]
                cases.append(Case(kind, "i64" if (kind, blocks) == ("f16", 3) else "i32", mid[kind], data == "exact", seg,
                                  (1, 2, 4)[len(kind) - 2] if blocks == 2 else 1, data,
                                  "known" if blocks == 2 else ("over", "skip")[data == "arb"], blocks, None))
    return cases


CASES = {case_id(c): c for c in all_cases()}


def mix(a, b, salt):
    """A 32-bit hash of (a, b, salt), elementwise, as uint64 arrays."""
    h = (np.asarray(a).astype(np.uint64) * np.uint64(0x9E3779B1) + np.asarray(b).astype(np.uint64) * np.uint64(0x85EBCA6B)
         + np.uint64(salt)) & MASK
    h = (h * np.uint64(0x27D4EB2F)) & MASK
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(0x165667B1)) & MASK
    h ^= h >> np.uint64(13)
    return h


def run_lengths(seg, per_block, exact, total=None):
    """Run lengths of one sorted COO laid out against segments of `seg` lookups, `per_block` of them per workgroup:
    1, 2, seg - 1, seg, seg + 1; a run that ends exactly at a segment end; one through three and more segments of one
    workgroup; one that ends exactly at a workgroup end; two that cross one workgroup boundary (the second parks
    partials on both sides); on exact data one through three and more workgroups; a ragged end.  Arbitrary data: no run
    longer than a workgroup's lookups.  `total`: cut or fill with short runs to exactly that many lookups."""
    block = seg * per_block
    out = []
    pos = 0

    def add(n):
        nonlocal pos
        if n > 0:
            out.append(n)
            pos += n

    def fill(to):
        k = 0
        while pos < to:
            add(min((1, 2, 3)[k % 3], to - pos))
            k += 1

    def up(m):
        return -(-pos // m) * m

    for n in (1, 2, seg - 1, seg, seg + 1):
        if exact or n <= block:
            add(n)
    fill(up(seg))
    if per_block >= 4:
        if pos % block + 4 * seg > block:
            fill(up(block))
        add(3)
        add(3 * seg - 1)          # the rest of a segment, two whole segments, two lookups of the fourth
    fill(up(block))
    fill(pos + block - 3)
    add(7)
    if per_block >= 2:
        fill(up(block) - seg - 2)
        add(min(2 * seg + 4, block))
    if exact:
        fill(max(pos, up(block) - 5))
        add(2 * block + 9)
    fill(pos + seg // 2 + 3)
    if pos % seg == 0:
        add(1)
    if total is not None:
        while pos > total:
            pos -= out.pop()
        fill(total)
    return out


def sample_block_length(nnz, blocks):
    """detail::SortSegmentLength: lookups per sample block of transpose(..., sample_blocks=blocks)."""
    tiles = max(1, -(-nnz // TILE))
    want = 1 if tiles <= 32 else max(1, min(64, blocks))
    return -(-tiles // want) * TILE


def build(case, seg, per_block):
    """The inputs of a case for a launch shape of `seg` lookups per segment and `per_block` segments per workgroup, as
    numpy arrays in COO order (for blocks > 1: block after block, each sorted -- what transpose(sample_blocks=) makes of
    it, since a stable sort leaves sorted blocks alone):
      keys      table row of every lookup             sids     its sample
      weights   fp32 or None                          grad_y   fp32 [BATCH, width]
      runs      (block, start inside the block, length, key, whether an earlier block holds the key) per run
      block_len lookups per sample block              rows     table rows (dense gradient)"""
    exact = case.data == "exact"
    block = seg * per_block
    if case.blocks == 1:
        lengths = [run_lengths(seg, per_block, exact, case.nnz)]
        nnz = sum(lengths[0])
        block_len = nnz
    else:
        nnz = BLOCKED_NNZ
        block_len = sample_block_length(nnz, case.blocks)
        lengths = [run_lengths(seg, per_block, exact, min(block_len, nnz - lo)) for lo in range(0, nnz, block_len)]
        assert len(lengths) == case.blocks
    runs = []
    for p, lens in enumerate(lengths):
        lens = np.asarray(lens, dtype=np.int64)
        start = np.cumsum(lens) - lens
        j = np.arange(lens.shape[0], dtype=np.int64)
        if case.blocks == 1:
            key = 3 * j + (mix(j, 0, 11) % np.uint64(3)).astype(np.int64)
        else:
            # block 0 holds the keys 4 j; a later block repeats them except in every third run and -- arbitrary data --
            # in the runs that cross a workgroup boundary, which get keys of their own (4 j + p)
            crossing = start // block != (start + lens - 1) // block
            # (exact data: the crossing runs are the ones that repeat block 0's keys)
            own = (j % 3 == 0) & ~crossing if exact else (j % 3 == 0) | crossing
            key = 4 * j + np.where(own, p, 0)
        runs.append((p, start, lens, key))
    keys = np.concatenate([np.repeat(key, lens) for _, _, lens, key in runs])
    seen = set()
    structure = []
    for p, start, lens, key in runs:
        shared = np.fromiter((int(k) in seen for k in key), dtype=bool, count=key.shape[0])
        seen.update(int(k) for k in key)
        structure.append((p, start, lens, key, shared))
    i = np.arange(nnz, dtype=np.int64)
    c = np.arange(case.width, dtype=np.int64)[None, :]
    s = np.arange(BATCH, dtype=np.int64)[:, None]
    if exact:
        # consecutive samples along the COO; sample s holds ((s + c) mod 3 - 1) x (1 or 2, per triple of samples and
        # column) and weighs 0.5 or 0.25 per triple: three aligned lookups in a row cancel
        sids = i % BATCH
        grad_y = ((s + c) % 3 - 1) * (1 + (mix(s // 3, c, 5) % np.uint64(2)).astype(np.int64))
        grad_y = grad_y.astype(np.float32)
        weights = np.where(mix(sids // 3, 0, 7) % np.uint64(2) == 0, 0.5, 0.25).astype(np.float32)
    else:
        sids = (mix(i, 0, 3) % np.uint64(BATCH)).astype(np.int64)
        grad_y = (((mix(s, c, 5) >> np.uint64(8)).astype(np.int64) - (1 << 23)).astype(np.float32) / np.float32(1 << 23))
        weights = ((2 * (mix(i, 0, 7) >> np.uint64(25)).astype(np.int64) + 1).astype(np.float32) / np.float32(256))
    return dict(keys=keys, sids=sids, weights=weights if case.weighted else None, grad_y=grad_y, runs=structure,
                block_len=block_len, rows=int(keys.max()) + 3, nnz=nnz)


def compressed_ids(keys):
    """(the dense id of every lookup of the FULLY sorted order, the order itself, the number of distinct rows)."""
    order = np.argsort(keys, kind="stable")
    uniq, rank = np.unique(keys[order], return_inverse=True)
    return rank.astype(np.int64), order, int(uniq.shape[0])
