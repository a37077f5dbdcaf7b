"""Rows and offsets past 2^31 / 2^32 in every kernel that addresses a row as base + id * width.

One untouched 32 GiB byte arena (module scope) is viewed as a [rows, W] table of any type; a case writes only the few
dozen rows it looks up -- the rows on either side of every 2^31 / 2^32 threshold of the row id, the element offset and
the byte offset (tests/far_rows.py; the host conditions are tests/test_far_rows_host.py's) -- and runs the kernel on
small batches that name them.  The reference is the same call, under the same forced launch shape, on a COMPACT copy:
the same rows in a small tensor at the same alignment, ids remapped to 0..k-1.  Every result is compared bit for bit (an
address must not change arithmetic) and, wherever one exists, against the CPU oracle or the fp32 model as well.  Every
address a kernel would form after narrowing an id, an element offset or a byte offset to 32 bits holds a poison row
(finite, one row long): a narrowing bug reads a wrong VALUE and never faults, and a kernel that writes must leave every
poison byte as it was.  Rows are filled and read back through slices (host pointer arithmetic), never through torch's
own index kernels.

Data: arbitrary bits, except where the summation order is not fixed -- the split forward and the default backward
(float atomics) get small integers, on which every order is exact.

Not here: far OUTPUT rows of the forward (test_gpu_large_inputs.py), the exchange kernels (ids are values there), more
than INT_MAX lookups.  Adam's two per-element moments stop past 2^31 elements: two 16 GiB tensors do not fit the arena.
"""
import ctypes

import numpy as np
import pytest
import torch

import far_rows as F
import optimizer_bits_reference as M
import quantized_reference as R

pytestmark = pytest.mark.gpu

TORCH = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
POISON = 0x3B                      # 0x3B3B3B3B = 2.86e-3 (fp32, bf16), 0x3B3B = 0.904 (fp16): finite in every type
MEMORY_CAP = 40 << 30
INT32 = 1 << 31
#: integer gradients: the integers a type holds exactly, the largest |gradient| drawn, the hot row's run.  With weights
#: of 1 or 2 every partial sum of a row that is looked up n times is an integer of at most 2 * top * n.
EXACT_INTEGERS = {"f32": 2 ** 24, "f16": 2048, "bf16": 256}
GRAD_TOP = {"f32": 3, "f16": 3, "bf16": 1}
HOT_RUN = {"f32": 350, "f16": 300, "bf16": 40}


@pytest.fixture(scope="module")
def ce():
    import cuembed_amd
    assert torch.cuda.is_available()
    return cuembed_amd


@pytest.fixture(scope="module")
def arena():
    free, _ = torch.cuda.mem_get_info()
    if free < MEMORY_CAP:
        pytest.skip("the far-row tests need %d GiB of free device memory, %d GiB are free" % (MEMORY_CAP >> 30, free >> 30))
    torch.cuda.reset_peak_memory_stats()
    a = torch.empty((F.ARENA_BYTES,), dtype=torch.uint8, device="cuda")       # never touched as a whole
    assert a.data_ptr() % 256 == 0
    yield a
    peak = torch.cuda.max_memory_allocated()
    print("\nfar rows: peak device memory %.2f GiB" % (peak / 2.0 ** 30))
    assert peak < MEMORY_CAP
    del a
    torch.cuda.empty_cache()


@pytest.fixture(autouse=True)
def _no_error_left(ce, arena):
    """Every test of the module waits for the arena (so all of them skip together where the memory is short) and ends
    with no error pending."""
    yield
    torch.cuda.synchronize()
    assert ce._lib.lib().cuembed_peek_last_error() == 0


# ---- helpers ---------------------------------------------------------------------------------------------------------
def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def make(oracle, kind, a):
    """Values -> (the oracle's array of `kind`, the same elements on the device)."""
    a32 = np.ascontiguousarray(a, dtype=np.float32)
    if kind == "f32":
        return a32, dev(a32)
    if kind == "f16":
        h = a32.astype(np.float16)
        return h, dev(h)
    b = oracle.to_bf16_bits(a32)
    return b, dev(b.view(np.int16)).view(torch.bfloat16)


def ibits(t):
    t = t.contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def dev_bits(a):
    a = np.ascontiguousarray(a)
    return dev(a.view({1: np.uint8, 2: np.int16, 4: np.int32}[a.dtype.itemsize]))


def same_bits(got, want, label):
    assert torch.equal(ibits(got).view(-1), ibits(want).view(-1)), label


def at_residue(t, shift):
    """A contiguous copy of t whose data pointer is `shift` bytes past a 16-byte boundary: the compact twin of a view
    with a shifted base takes the same lane width."""
    size = t.element_size()
    flat = torch.empty((t.numel() + 32 // size,), dtype=t.dtype, device="cuda")
    first = ((shift - flat.data_ptr()) % 16) // size
    v = flat[first:first + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == shift % 16 and v.is_contiguous()
    return v


def lane_bytes(size, width, *pointers):
    bits = size * width
    for p in pointers:
        bits |= p
    return 16 if bits % 16 == 0 else (8 if bits % 8 == 0 else 4)


def tensor_of(arena, view, dtype):
    """The arena's bytes [view.base, view.end) as a [rows, width] tensor of dtype: a view, nothing is touched."""
    assert view.end <= arena.numel() and dtype.itemsize == view.elem_size
    t = arena[view.base:view.end].view(dtype).view(view.rows, view.width)
    assert t.data_ptr() == arena.data_ptr() + view.base and t.is_contiguous()
    return t


def put_rows(t, rows, compact):
    for k, r in enumerate(rows):
        t[r].copy_(compact[k])


def get_rows(t, rows):
    return torch.stack([t[r] for r in rows])


def poison(arena, layout, *compacts):
    """Fills every alias with the poison pattern; the compact rows must differ from it."""
    for a, n in layout.aliases:
        arena[a:a + n].fill_(POISON)
    for c in compacts:
        assert not bool((c.contiguous().view(torch.uint8).view(c.shape[0], -1) == POISON).all(dim=1).any())


def poison_intact(arena, layout):
    held = torch.cat([arena[a:a + n] for a, n in layout.aliases])
    assert bool((held == POISON).all()), "a store went to a narrowed address"


def bag_weights(oracle, kind, rng, n, mode, integer):
    if integer:
        w = rng.integers(1, 3, n)
    else:
        w = rng.uniform(0.25, 1.25, n) if mode == "mean" else rng.uniform(-1, 1, n)
    return make(oracle, kind, w)


# ---- forward ---------------------------------------------------------------------------------------------------------
BATCH, HOT, LONG_HOT = 300, 5, 4200       # 300 bags: two workgroups of one-lane rows; 4,200 ids per bag: too long to stage


def _forward_cases(oracle, kind, rows, idt, seed, integer=False):
    """Fixed hotness (staged; one bag too long to stage), CSR with int64 and int32 offsets, concat; sum and mean,
    weighted and not.  Each case: the far ids, the compact ids, and what the oracle needs."""
    rng = np.random.default_rng(seed)
    cases = []

    def add(name, ids, off, weighted, batch, hot, mode):
        w_o = w_d = None
        if weighted:
            w_o, w_d = bag_weights(oracle, kind, rng, ids.size, mode, integer)
        cmp_ids = F.compact(ids, rows)
        cases.append(dict(name=name, far=dev(ids), cmp=dev(cmp_ids), cmp_np=cmp_ids, off=dev(off), off_np=off, w=w_d,
                          w_o=w_o, batch=batch, hot=hot, mode=mode, csr=off is not None, want={}))

    hot = 8 if integer else HOT                                    # (the split kernel takes fixed bags from 8 lookups)
    fixed = F.fixed_bags(rows, BATCH, hot, seed, idt)
    for mode in ("sum", "mean"):
        for weighted in (False, True):
            add("fixed %s%s" % (mode, " weighted" * weighted), fixed, None, weighted, BATCH, hot, mode)
    for k, odt in enumerate((np.int64, np.int32)):
        ids, off = F.csr_bags(rows, BATCH, seed + 1 + k, dtype=idt, offset_dtype=odt)
        for mode, weighted in (("sum", k == 1), ("mean", k == 0)):
            add("csr o%d %s%s" % (8 * odt().itemsize, mode, " weighted" * weighted), ids, off, weighted, BATCH, 0, mode)
        add("csr o%d sum%s" % (8 * odt().itemsize, " weighted" * (k == 0)), ids, off, k == 0, BATCH, 0, "sum")
    if not integer:
        long_ids = F.fixed_bags(rows, 3, LONG_HOT, seed + 5, idt)
        add("fixed long sum", long_ids, None, False, 3, LONG_HOT, "sum")
        add("fixed long mean weighted", long_ids, None, True, 3, LONG_HOT, "mean")
        add("concat", fixed, None, False, BATCH, hot, "concat")
    return cases


def _oracle_forward(oracle, compact_o, c, fp16_math):
    if fp16_math not in c["want"]:
        want = oracle.embedding_forward(compact_o, c["cmp_np"], c["off_np"], c["w_o"], batch_size=c["batch"],
                                        num_hots=c["hot"], mode=c["mode"], fp16_math=fp16_math)
        c["want"][fp16_math] = dev_bits(want).view(-1)
    return c["want"][fp16_math]


def _both(ce, table, twin, c, **kw):
    args = dict(offsets=c["off"], weights=c["w"], batch_size=c["batch"], num_hots=c["hot"], mode=c["mode"], **kw)
    return ce.embedding_forward(table, c["far"], **args), ce.embedding_forward(twin, c["cmp"], **args)


@pytest.mark.parametrize("kind,width,shift,lane,int32_too", F.FORWARD_TABLES,
                         ids=["%s-W%d+%d" % c[:3] for c in F.FORWARD_TABLES])
def test_forward_reads_far_rows(ce, oracle, arena, kind, width, shift, lane, int32_too):
    """Every forward kernel: the sequential one with its three index sources (LDS-staged: fixed hotness; wave-shuffle:
    CSR and the bag too long to stage, where the lanes of a row divide a wavefront; global: W = 36 in fp32), the
    wide-load kernel with one and four samples per workgroup, the split kernel and concat -- with ordinary and
    non-temporal row loads, and under a sample order."""
    dtype, size = TORCH[kind], F.ELEM_SIZE[kind]
    view = F.table_view(kind, width, shift)
    table = tensor_of(arena, view, dtype)
    assert lane_bytes(size, width, table.data_ptr()) == lane
    shape = lambda c, it: ce.forward_launch_shape(dtype, it, width, c["batch"], c["hot"], c["csr"], c["w"] is not None,
                                                  c["mode"])
    ran, wrong = set(), []                                              # (every family runs before the test fails)

    def family(c, wide, lanes):
        if c["mode"] == "concat":
            return "concat"
        if wide != "never" and width != 36:
            return wide
        fixed_short = not c["csr"] and c["hot"] != LONG_HOT
        return "staged" if fixed_short else "shuffle" if 64 % lanes == 0 else "global"

    try:
        for idt, it in ((np.int64, torch.int64),) + (((np.int32, torch.int32),) if int32_too else ()):
            layout, (rows,) = F.pick([view], seed=11 + width, below=INT32 if idt == np.int32 else None)
            assert max(rows) * width >= INT32 and (idt == np.int32 or max(rows) * view.row_bytes >= (1 << 34))
            rng = np.random.default_rng(width + shift)
            compact_o, compact_d = make(oracle, kind, rng.uniform(-1, 1, (len(rows), width)))
            twin = at_residue(compact_d, shift)
            poison(arena, layout, compact_d)
            put_rows(table, rows, compact_d)
            cases = _forward_cases(oracle, kind, rows, idt, seed=width + 7)
            for wide in ("never", "always", "always4"):
                ce.set_forward_wide_load(wide)
                for c in cases:
                    if c["mode"] == "concat" and wide != "never":
                        continue
                    if shift == 0:                                            # (the planner is asked about aligned buffers)
                        s = shape(c, it)
                        if wide == "never":
                            assert not s["wide_load"]
                            assert s["staged"] == (not c["csr"] and c["mode"] != "concat" and c["hot"] != LONG_HOT)
                            ran.add("staged" if s["staged"] else "concat" if c["mode"] == "concat" else
                                    "shuffle" if 64 % s["lanes_per_row"] == 0 else "global")
                        elif c["mode"] != "concat":
                            assert s["wide_load"] == (width != 36), (wide, c["name"], s)
                            assert width == 36 or s["samples_per_block"] == (1 if wide == "always" else 4)
                            ran.add(wide if s["wide_load"] else "global")
                    options = [dict(), dict(row_loads="streaming")]
                    if kind == "f16" and c["mode"] != "concat":
                        options.append(dict(fp16_math=True))
                    if c["csr"] and wide == "never":
                        order = torch.flip(ce.bag_order_by_length(c["off"]), dims=(0,)).contiguous()
                        options.append(dict(sample_order=order))
                    for kw in options:
                        label = (family(c, wide, width * size // lane), idt.__name__, wide, c["name"], sorted(kw))
                        got, ref = _both(ce, table, twin, c, **kw)
                        if not torch.equal(ibits(got).view(-1), ibits(ref).view(-1)):
                            wrong.append(label)
                        assert torch.equal(ibits(ref).view(-1), _oracle_forward(oracle, compact_o, c, kw.get("fp16_math", False))), label
            # split: integer rows in {-1, 0, 1} and weights in {1, 2} -- sums of at most 140: exact in any order, in bf16 too
            ce.set_forward_wide_load("auto")
            int_o, int_d = make(oracle, kind, rng.integers(-1, 2, (len(rows), width)))
            twin = at_residue(int_d, shift)
            put_rows(table, rows, int_d)
            for c in _forward_cases(oracle, kind, rows, idt, seed=width + 9, integer=True):
                got, ref = _both(ce, table, twin, c, reduction_order="split")
                if not torch.equal(ibits(got).view(-1), ibits(ref).view(-1)):
                    wrong.append(("split" if width != 36 else "global", idt.__name__, "split", c["name"]))
                assert torch.equal(ibits(ref).view(-1), _oracle_forward(oracle, int_o, c, False)), ("split", c["name"])
            assert torch.equal(get_rows(table, rows), int_d)
    finally:
        ce.set_forward_wide_load("auto")
    assert ce.get_forward_reduction_order() == "sequential"
    assert not wrong, "%d far results differ from the compact run's; families: %s; the first: %r" % (
        len(wrong), sorted({w[0] for w in wrong}), wrong[0])
    if shift == 0:
        want = {"staged", "concat", "global" if width == 36 else "shuffle"} | ({"always", "always4"} if width != 36 else set())
        assert ran == want, ran


# ---- weight gradient -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,width,shift", F.WEIGHT_GRAD_TABLES, ids=["%s-W%d+%d" % c for c in F.WEIGHT_GRAD_TABLES])
def test_weight_gradient_reads_far_rows(ce, oracle, arena, kind, width, shift):
    """Integer data, at most 32 non-zero gradient columns: |dot| <= 128, every product and partial sum exact in fp32 in
    any order and the result representable in fp16 and bf16 -- the device's bits are those of the float64 dot product.
    W = 2 / 8: one lane or two per row (the fallback walk), 36: a masked lane group, 256 / 1024: rows wider than a wave."""
    dtype = TORCH[kind]
    view = F.table_view(kind, width, shift)
    table = tensor_of(arena, view, dtype)
    batch, hot = 45, 5
    for idt in (np.int64, np.int32):
        layout, (rows,) = F.pick([view], seed=23 + width, below=INT32 if idt == np.int32 else None)
        rng = np.random.default_rng(300 + width)
        values = rng.integers(-2, 3, (len(rows), width))
        values[:, 0] = np.arange(len(rows)) % 5 - 2                    # (no two rows alike by accident is not needed: the dot tells)
        _, compact_d = make(oracle, kind, values)
        poison(arena, layout, compact_d + 0)
        put_rows(table, rows, compact_d)
        gy = rng.integers(-2, 3, (batch, width))
        gy[:, rng.permutation(width)[32:]] = 0
        _, gy_d = make(oracle, kind, gy)
        fixed = F.fixed_bags(rows, batch, hot, 5, idt)
        csr, off = F.csr_bags(rows, batch, 6, longest=20, dtype=idt, offset_dtype=idt)
        for ids, o, sample in ((fixed, None, np.repeat(np.arange(batch), hot)),
                               (csr, off, np.repeat(np.arange(batch), np.diff(off)))):
            pos = F.compact(ids, rows)
            exact = (values[pos].astype(np.float64) * gy[sample].astype(np.float64)).sum(axis=1)
            assert np.abs(exact).max() <= 128 and np.abs(exact).max() >= min(8, width)
            want = dev_bits(make(oracle, kind, exact)[0])
            kw = dict(offsets=dev(o), num_hots=0 if o is not None else hot)
            got = ce.embedding_weight_grad(table, dev(ids), gy_d, **kw)
            ref = ce.embedding_weight_grad(at_residue(compact_d, shift), dev(pos), gy_d, **kw)
            assert torch.equal(ibits(got), want) and torch.equal(ibits(ref), want), (idt.__name__, o is not None)


# ---- 8-bit tables ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width,shift,codes", F.QUANTIZED_TABLES, ids=["W%d+%d" % c[:2] for c in F.QUANTIZED_TABLES])
def test_quantized_forward_and_dequantizer_read_far_rows(ce, arena, width, shift, codes):
    """Fused rows of W + 8 bytes past 4 GiB and 16 GiB, 16 / 8 / 4 codes per lane: the pooled forward (fp32 and fp16
    output, sum and mean, weighted, fixed hotness and CSR) bit-identical to the compact table's and inside pooled64's
    bound; dequantize_rows(qtable, ids) and concat are dequant32's bits."""
    view = F.quantized_view(width, shift)
    qtable = tensor_of(arena, view, torch.uint8)
    if shift == 0:
        s = ce.quantized_forward_launch_shape(torch.int64, torch.float32, width, 41, 7)
        assert s["codes_per_lane"] == codes, s
    for idt, it in ((np.int64, torch.int64), (np.int32, torch.int32)):
        layout, (rows,) = F.pick([view], seed=31 + width, below=INT32 if idt == np.int32 else None)
        assert max(rows) * view.row_bytes >= (1 << 32)
        k = len(rows)
        x = np.concatenate([R.make_table("normal", k - k // 2, width, seed=width), R.make_table("uniform", k // 2, width, seed=width + 17)])
        q_np = R.quantize(x)
        q_d = ce.quantize_rows(torch.from_numpy(x).cuda())
        assert np.array_equal(q_d.cpu().numpy(), q_np)
        twin = at_residue(q_d, shift)
        poison(arena, layout, q_d)
        put_rows(qtable, rows, q_d)
        want32 = R.dequant32(q_np)
        picked = F.fixed_bags(rows, 9, 5, 3, idt)
        pos = F.compact(picked, rows)
        got = ce.dequantize_rows(qtable, dev(picked).view(9, 5))
        assert torch.equal(ibits(got), dev_bits(want32[pos].reshape(9, 5, width)))
        got16 = ce.dequantize_rows(qtable, dev(picked), dtype=torch.float16)
        assert torch.equal(ibits(got16), dev_bits(want32.astype(np.float16)[pos]))
        concat = ce.embedding_forward_quantized(qtable, dev(picked), num_hots=5, mode="concat", out_dtype=torch.float32)
        assert torch.equal(ibits(concat).view(-1), dev_bits(want32[pos]).view(-1))
        fixed = F.fixed_bags(rows, 41, 7, 4, idt)
        csr, off = F.csr_bags(rows, 41, 5, longest=40, dtype=idt, offset_dtype=np.int32 if idt == np.int64 else np.int64)
        rng = np.random.default_rng(width)
        for out, np_out in (("f32", np.float32), ("f16", np.float16)):
            for ids, o, hot in ((fixed, None, 7), (csr, off, 0)):
                for mode in ("sum", "mean"):
                    for weighted in (False, True):
                        w = None
                        if weighted:
                            w = (rng.uniform(-1, 1, ids.size) if mode == "sum" else rng.uniform(0.25, 1.25, ids.size)).astype(np_out)
                        p = F.compact(ids, rows)
                        kw = dict(offsets=dev(o), weights=dev(w), num_hots=hot, mode=mode, out_dtype=TORCH[out])
                        label = (idt.__name__, out, o is not None, mode, weighted)
                        ref = ce.embedding_forward_quantized(twin, dev(p), **kw)
                        for extra in (dict(), dict(row_loads="streaming")):
                            same_bits(ce.embedding_forward_quantized(qtable, dev(ids), **kw, **extra), ref, label)
                        exact, bound = R.pooled64(q_np, p, offsets=o, num_hots=hot, weights=w, mode=mode, out=out)
                        assert R.worst_ratio(ref.float().cpu().numpy(), exact, bound) <= 1.0, label


# ---- grouped forward: three tables far apart ---------------------------------------------------------------------------
def _grouped_batch(rows_per_table, idt, seed, B=5):
    """B = 5 bags per table: table boundaries fall inside a wavefront.  Returns fixed-hotness ids [T, B, 3] and a CSR
    batch (ids, offsets, per-table slices) with empty bags."""
    rng = np.random.default_rng(seed)
    fixed = np.stack([F.fixed_bags(rows, B, 3, seed + t, idt).reshape(B, 3) for t, rows in enumerate(rows_per_table)])
    lens = rng.integers(0, 9, len(rows_per_table) * B)
    lens[[0, 6, len(lens) - 1]] = 0
    lens[7] = 70
    off = np.concatenate([[0], np.cumsum(lens)])
    ids = np.concatenate([np.asarray(rows, dtype=np.int64)[rng.integers(0, len(rows), int(lens[t * B:(t + 1) * B].sum()))]
                          for t, rows in enumerate(rows_per_table)]).astype(idt)
    return fixed, ids, off


@pytest.mark.parametrize("kind,width", F.GROUPED_TABLES, ids=["%s-W%d" % c for c in F.GROUPED_TABLES])
def test_grouped_forward_reads_far_rows_of_three_tables(ce, oracle, arena, kind, width):
    """embedding_forward_grouped on three 9 GiB tables 9 GiB apart, each looked up at its own boundary rows (element
    offsets past 2^32): torch.stack of the single-table calls on the compact copies, bit for bit."""
    dtype = TORCH[kind]
    views = F.grouped_views(F.ELEM_SIZE[kind], width)
    tables = [tensor_of(arena, v, dtype) for v in views]
    group = ce.TableGroup(tables)
    B, T = 5, 3
    for idt in (np.int64, np.int32):
        layout, rows = F.pick(views, seed=41 + width, below=INT32 if idt == np.int32 else None)
        assert all(max(r) * width >= (1 << 32) or idt == np.int32 for r in rows) and all(max(r) * width >= INT32 for r in rows)
        rng = np.random.default_rng(width)
        compacts = [make(oracle, kind, rng.uniform(-1, 1, (len(r), width)))[1] for r in rows]
        poison(arena, layout, *compacts)
        for t in range(T):
            put_rows(tables[t], rows[t], compacts[t])
        fixed, ids, off = _grouped_batch(rows, idt, seed=width)
        w_fixed = make(oracle, kind, rng.uniform(-1, 1, fixed.size))[1]
        w_csr = make(oracle, kind, rng.uniform(0.25, 1.25, ids.size))[1]
        for mode in ("sum", "mean"):
            for weighted in (False, True):
                got = ce.embedding_forward_grouped(group, dev(fixed), num_hots=3, mode=mode, weights=w_fixed if weighted else None)
                want = torch.stack([ce.embedding_forward(compacts[t], dev(F.compact(fixed[t].reshape(-1), rows[t])), num_hots=3,
                                                         mode=mode, weights=w_fixed.view(T, -1)[t].contiguous() if weighted else None)
                                    for t in range(T)], dim=1)
                same_bits(got, want, (idt.__name__, "fixed", mode, weighted))
                for odt in (np.int64, np.int32):
                    for extra in (dict(), dict(row_loads="streaming")):
                        got = ce.embedding_forward_grouped(group, dev(ids), dev(off.astype(odt)), mode=mode,
                                                           weights=w_csr if weighted else None, **extra)
                        per = []
                        for t in range(T):
                            lo, hi = int(off[t * B]), int(off[(t + 1) * B])
                            per.append(ce.embedding_forward(compacts[t], dev(F.compact(ids[lo:hi], rows[t])),
                                                            dev((off[t * B:(t + 1) * B + 1] - lo).astype(odt)), mode=mode,
                                                            weights=w_csr[lo:hi].contiguous() if weighted else None))
                        same_bits(got, torch.stack(per, dim=1), (idt.__name__, "csr", odt.__name__, mode, weighted))


def test_grouped_quantized_forward_reads_far_rows_of_three_tables(ce, arena):
    width = F.GROUPED_QUANTIZED_WIDTH
    views = F.grouped_views(1, width + 8)
    tables = [tensor_of(arena, v, torch.uint8) for v in views]
    group = ce.TableGroup(tables)
    B, T = 5, 3
    for idt in (np.int64, np.int32):
        layout, rows = F.pick(views, seed=51, below=INT32 if idt == np.int32 else None)
        assert all(max(r) * (width + 8) >= (1 << 32) for r in rows)
        compacts = [ce.quantize_rows(torch.from_numpy(R.make_table("normal", len(r), width, seed=t)).cuda())
                    for t, r in enumerate(rows)]
        poison(arena, layout, *compacts)
        for t in range(T):
            put_rows(tables[t], rows[t], compacts[t])
        fixed, ids, off = _grouped_batch(rows, idt, seed=9)
        rng = np.random.default_rng(2)
        for out in (torch.float32, torch.float16):
            w_csr = torch.from_numpy(rng.uniform(0.25, 1.25, ids.size)).to("cuda", out)
            for mode in ("sum", "mean"):
                got = ce.embedding_forward_quantized_grouped(group, dev(fixed), num_hots=3, mode=mode, out_dtype=out)
                want = torch.stack([ce.embedding_forward_quantized(compacts[t], dev(F.compact(fixed[t].reshape(-1), rows[t])),
                                                                   num_hots=3, mode=mode, out_dtype=out) for t in range(T)], dim=1)
                same_bits(got, want, (idt.__name__, "fixed", mode, out))
                for weighted in (False, True):
                    got = ce.embedding_forward_quantized_grouped(group, dev(ids), dev(off), mode=mode, out_dtype=out,
                                                                 weights=w_csr if weighted else None)
                    per = []
                    for t in range(T):
                        lo, hi = int(off[t * B]), int(off[(t + 1) * B])
                        per.append(ce.embedding_forward_quantized(compacts[t], dev(F.compact(ids[lo:hi], rows[t])),
                                                                  dev(off[t * B:(t + 1) * B + 1] - lo), mode=mode, out_dtype=out,
                                                                  weights=w_csr[lo:hi].contiguous() if weighted else None))
                    same_bits(got, torch.stack(per, dim=1), (idt.__name__, "csr", mode, out, weighted))


# ---- grouped, one storage: global row ids past 2^31 ------------------------------------------------------------------
def test_one_storage_group_trains_rows_past_2_31(ce, arena):
    """TableGroup.from_flat over 8-byte rows with row_counts (2^31 + 5, 17, 42): the keys are int64 and pass 2^31, the
    grouped backward returns global ids at and past 2^31, the table cuts fall between them, and one SGD step on
    group.flat with those ids updates exactly the named rows."""
    counts = F.FLAT_ROW_COUNTS
    view = F.flat_view()
    flat = tensor_of(arena, view, torch.float32)
    group = ce.TableGroup.from_flat(flat, counts)
    base = group.row_base
    assert base == (0, counts[0], counts[0] + 17, view.rows) and base[1] > INT32
    T, B, W = 3, 5, 2
    layout, (picked,) = F.pick([view], seed=61)
    local = [[r for r in picked if r < base[1]], [0, 1, 16], [0, 7, 40, 41]]
    rows = sorted(set(picked) | {base[1] + r for r in local[1]} | {base[2] + r for r in local[2]})
    layout = F.Layout([(view, rows)])
    rng = np.random.default_rng(6)
    weights = rng.uniform(-1, 1, (len(rows), W)).astype(np.float32)
    poison(arena, layout, dev(weights))
    put_rows(flat, rows, dev(weights))
    fixed, ids, off = _grouped_batch(local, np.int64, seed=4)
    want_sids = {}
    for name, idx, offsets, hot in (("fixed", fixed.reshape(-1), None, 3), ("csr", ids, off, 0)):
        lens = np.full(T * B, hot) if offsets is None else np.diff(offsets)
        bag = np.repeat(np.arange(T * B), lens)
        want_keys = idx.astype(np.int64) + np.asarray(base)[bag // B]
        want_sids[name] = (bag % B) * T + bag // B
        for idt in (np.int64, np.int32):
            if idx.astype(np.int64).max() >= INT32 and idt == np.int32:
                continue
            keys, sids = ce.grouped_backward_keys(group, dev(idx.astype(idt)), dev(offsets), num_hots=hot)
            assert keys.dtype == torch.int64 and sids.dtype == torch.int64
            assert np.array_equal(keys.cpu().numpy(), want_keys) and np.array_equal(sids.cpu().numpy(), want_sids[name])
        assert want_keys.max() >= INT32 + 5 + 17
    # the backward: integer gradients (atomics add in any order), the global ids and their rows against numpy
    bag = np.repeat(np.arange(T * B), np.diff(off))
    keys = ids.astype(np.int64) + np.asarray(base)[bag // B]
    gy = rng.integers(-3, 4, (B, T, W)).astype(np.float32)
    grad = ce.embedding_backward_grouped(group, dev(gy), dev(ids), dev(off))
    uniq = np.unique(keys)
    n = int(grad.last_id.item()) + 1
    assert n == uniq.size and grad.ids.dtype == torch.int64 and np.array_equal(grad.ids[:n].cpu().numpy(), uniq)
    sums = np.zeros((uniq.size, W))
    np.add.at(sums, np.searchsorted(uniq, keys), gy.reshape(B * T, W)[want_sids["csr"]].astype(np.float64))
    assert np.array_equal(grad.rows[:n].cpu().numpy(), sums.astype(np.float32))
    cuts = grad.table_cuts().cpu().numpy()
    assert np.array_equal(cuts, np.searchsorted(uniq, np.asarray(base)))
    assert cuts[1] < cuts[2] < cuts[3] == n and uniq[cuts[1]] >= INT32
    # one SGD step on the flat storage: w + -(lr * g), one fp32 operation each
    before = get_rows(flat, rows).cpu().numpy()
    ce.sparse_row_update(flat, grad.ids, grad.rows, rule="sgd", lr=0.05, last_id=grad.last_id)
    want = before.copy()
    at = np.searchsorted(np.asarray(rows), uniq)
    want[at] = before[at] + -(np.float32(0.05) * sums.astype(np.float32))
    after = get_rows(flat, rows).cpu().numpy()
    assert np.array_equal(after.view(np.uint32), want.view(np.uint32)) and not np.array_equal(after[at], before[at])
    poison_intact(arena, layout)


# ---- backward: the dense gradient in the arena -------------------------------------------------------------------------
def _backward_problem(oracle, kind, width, rows, idt, seed, arbitrary):
    """700 lookups of the picked rows but one, the last row hot with a run that chains across segments; the sorted COO
    from the oracle, far and compact."""
    rng = np.random.default_rng(seed)
    batch, hot = 175, 4
    named = np.asarray([r for k, r in enumerate(rows) if k != 2], dtype=np.int64)
    ids = F.fixed_bags(named, batch, hot, seed, np.int64)
    top = GRAD_TOP[kind]
    ids[ids == named[-1]] = named[0]
    ids[rng.choice(ids.size, HOT_RUN[kind], replace=False)] = named[-1]
    ids[:named.size] = named
    counts = np.bincount(F.compact(ids, rows))
    assert counts[-1] >= HOT_RUN[kind] - named.size and 2 * top * counts.max() <= EXACT_INTEGERS[kind]
    ids = ids.astype(idt)
    w_o = make(oracle, kind, rng.uniform(0.25, 1.25, ids.size) if arbitrary else rng.integers(1, 3, ids.size))[0]
    gy_o, gy_d = make(oracle, kind, rng.uniform(-1, 1, (batch, width)) if arbitrary else
                      rng.integers(-top, top + 1, (batch, width)))
    sid = oracle.extract_row_ids_from_fixed(batch, hot, dtype=idt)
    t_idx, t_sid, t_w = oracle.transpose(sid, ids, w_o)
    c_idx = F.compact(t_idx, rows)
    t_w_d = dev(t_w.view(np.int16)).view(torch.bfloat16) if kind == "bf16" else dev(t_w)
    want = {w: dev_bits(oracle.embedding_backward(gy_o, width, len(rows), c_idx, t_sid, None, t_w if w else None)[0])
            for w in (False, True)}
    return dict(gy=gy_d, t_idx=dev(t_idx), c_idx=dev(c_idx), t_sid=dev(t_sid), t_w=t_w_d, want=want)


@pytest.mark.parametrize("kind,width", F.BACKWARD_TABLES, ids=["%s-W%d" % c for c in F.BACKWARD_TABLES])
def test_backward_scatters_into_far_rows(ce, oracle, arena, kind, width):
    """grad_embedding is an arena view (skip_grad_init=True, the touched rows zeroed first): row ids up to 2^31 - 1,
    element offsets past 2^32.  Short and long segments, 1 and 4 column slices, weighted and not; reference_sums on
    arbitrary data.  The oracle's bits, the compact run's bits, an unnamed row stays zero, the poison stays."""
    dtype = TORCH[kind]
    view = F.backward_view(kind, width)
    grad = tensor_of(arena, view, dtype)
    assert ce.get_backward_tuning() == dict(segment_len=0, column_slices=0)
    try:
        for idt in (np.int64, np.int32):
            layout, (rows,) = F.pick([view], seed=71 + width)
            assert max(rows) < INT32 and max(rows) * view.row_bytes >= (1 << 34) - 2 * view.row_bytes
            assert max(rows) * width >= (1 << 32) or view.row_bytes == 8       # (8-byte fp32 rows: 2^32 - 2 elements)
            zeros = torch.zeros((len(rows), width), dtype=dtype, device="cuda")
            poison(arena, layout)
            for arbitrary in (False, True):
                p = _backward_problem(oracle, kind, width, rows, idt, seed=width + arbitrary, arbitrary=arbitrary)
                tunings = ((0, 0),) if arbitrary else ((0, 0), (8, 1), (8, 4), (256, 1), (256, 4))
                for segment_len, slices in tunings:
                    ce.set_backward_tuning(segment_len, slices)
                    for weighted in (False, True):
                        label = (idt.__name__, arbitrary, segment_len, slices, weighted)
                        put_rows(grad, rows, zeros)
                        kw = dict(transpose_weights=p["t_w"] if weighted else None, skip_grad_init=True,
                                  reference_sums=arbitrary)
                        ce.embedding_backward(p["gy"], view.rows, p["t_idx"], p["t_sid"], grad_embedding=grad, **kw)
                        ref, _ = ce.embedding_backward(p["gy"], len(rows), p["c_idx"], p["t_sid"], **kw)
                        got = get_rows(grad, rows)
                        same_bits(got, ref, label)
                        assert torch.equal(ibits(got).view(-1), p["want"][weighted].view(-1)), label
                        assert not bool(got[2].any()) and bool(got.any())
                        poison_intact(arena, layout)
    finally:
        ce.set_backward_tuning(0, 0)


def test_backward_zeroes_a_table_of_int_max_rows(ce, oracle, arena):
    """skip_grad_init=False on exactly 2^31 - 1 rows of 8 bytes: after the call every row the batch does not name reads
    zero -- boundary and random rows, the last MiB, and the whole tensor's count of non-zeros."""
    view = F.table_view("f32", 2, rows=F.BACKWARD_MAX_ROWS, name="grad")
    grad = tensor_of(arena, view, torch.float32)
    layout, (rows,) = F.pick([view], seed=81)
    others = F.boundary_rows(view, seed=82, random_rows=24)
    others = [r for r in others if r not in rows] + [r + 1 for r in rows if r + 1 < view.rows and r + 1 not in rows]
    for r in rows + others:
        grad[r].fill_(7.0)                                          # garbage where zeros are due
    grad[view.rows - (1 << 17):].fill_(3.0)
    p = _backward_problem(oracle, "f32", 2, rows, np.int64, seed=3, arbitrary=False)
    ce.embedding_backward(p["gy"], view.rows, p["t_idx"], p["t_sid"], grad_embedding=grad)
    got = get_rows(grad, rows)
    assert torch.equal(ibits(got).view(-1), p["want"][False].view(-1))
    assert not bool(get_rows(grad, others).any())
    # an 8-byte row is one int64 word; counted 2^27 rows at a time (the comparison's temporary stays at 128 MiB)
    words = grad.view(torch.int64).view(-1)
    named_words = got.view(torch.int64).view(-1) != 0
    first = view.rows - (1 << 17)
    assert rows[-1] == view.rows - 1 and bool(named_words[-1])
    in_tail = sum(int(named_words[k]) for k, r in enumerate(rows) if r >= first)
    assert int((words[first:] != 0).sum()) == in_tail
    total = sum(int((words[at:at + (1 << 27)] != 0).sum()) for at in range(0, view.rows, 1 << 27))
    assert total == int(named_words.sum()) and total >= len(rows) - 3


@pytest.mark.parametrize("kind,width", (("f32", 4), ("f16", 64), ("bf16", 8)), ids=["f32-W4", "f16-W64", "bf16-W8"])
def test_backward_gathers_far_gradient_rows(ce, oracle, arena, kind, width):
    """grad_y is the arena view: the SAMPLE ids are the boundary rows (below 2^31: a sample id travels in 31 bits), the
    gradient rows they name lie past 2^32 elements.  Full and compressed gradient, weighted, reference_sums."""
    dtype = TORCH[kind]
    view = F.backward_view(kind, width)
    grad_y = tensor_of(arena, view, dtype)
    ncat = 50
    for idt in (np.int64, np.int32):
        layout, (rows,) = F.pick([view], seed=91 + width)
        rng = np.random.default_rng(width)
        poison(arena, layout)
        nnz = 600
        sid = np.asarray(rows, dtype=np.int64)[rng.integers(0, len(rows), nnz)]
        sid[:len(rows)] = rows
        sid = np.sort(sid).astype(idt)                                # (sample-major, as a CSR batch would be)
        idx = rng.integers(0, ncat, nnz)
        idx[rng.choice(nnz, 40, replace=False)] = 7
        assert 2 * GRAD_TOP[kind] * np.bincount(idx).max() <= EXACT_INTEGERS[kind]
        idx = idx.astype(idt)
        for arbitrary in (False, True):
            gy_o, gy_d = make(oracle, kind, rng.uniform(-1, 1, (len(rows), width)) if arbitrary else
                              rng.integers(-GRAD_TOP[kind], GRAD_TOP[kind] + 1, (len(rows), width)))
            w_o = make(oracle, kind, rng.uniform(0.25, 1.25, nnz) if arbitrary else rng.integers(1, 3, nnz))[0]
            put_rows(grad_y, rows, gy_d)
            t_idx, t_sid, t_w = oracle.transpose(sid, idx, w_o)
            c_sid = F.compact(t_sid, rows)
            remap = oracle.compute_compressed_grad_indices(t_idx)
            nu = int(remap[-1]) + 1
            t_w_d = dev(t_w.view(np.int16)).view(torch.bfloat16) if kind == "bf16" else dev(t_w)
            for weighted in (False, True):
                kw = dict(transpose_weights=t_w_d if weighted else None, reference_sums=arbitrary)
                w = t_w if weighted else None
                full, _ = ce.embedding_backward(grad_y, ncat, dev(t_idx), dev(t_sid), **kw)
                want, _ = oracle.embedding_backward(gy_o, width, ncat, t_idx, c_sid, None, w)
                assert torch.equal(ibits(full), dev_bits(want)), (idt.__name__, arbitrary, weighted, "full")
                comp, inv = ce.embedding_backward(grad_y, nu, dev(t_idx), dev(t_sid), dev(remap), **kw)
                want, want_inv = oracle.embedding_backward(gy_o, width, nu, t_idx, c_sid, remap, w)
                assert torch.equal(ibits(comp), dev_bits(want)) and np.array_equal(inv.cpu().numpy(), want_inv)


def test_compressed_backward_carries_ids_past_2_32(ce, oracle):
    """int64 ids at and past 2^32 through transpose_fixed_hotness(remapped=True) and the compressed backward: the
    inverse mapping carries them verbatim, the gradient is the compact run's."""
    rng = np.random.default_rng(5)
    batch, hot, width = 300, 4, 32
    far = np.unique(np.concatenate([[0, 1, INT32 - 1, INT32, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 33) + 5, (1 << 40) + 3,
                                     (1 << 62) + 1], rng.integers(0, 1 << 45, 40)]))
    ids = F.fixed_bags(far, batch, hot, 9)
    gy = dev(rng.integers(-3, 4, (batch, width)).astype(np.float32))
    t_idx, t_sid, _, remap = ce.transpose_fixed_hotness(dev(ids), batch, hot, remapped=True)
    c_idx, c_sid, _, c_remap = ce.transpose_fixed_hotness(dev(F.compact(ids, far)), batch, hot, remapped=True)
    order = np.argsort(ids, kind="stable")
    assert np.array_equal(t_idx.cpu().numpy(), ids[order]) and np.array_equal(t_sid.cpu().numpy(), order // hot)
    assert torch.equal(t_sid, c_sid) and torch.equal(remap, c_remap)
    nu = int(remap[-1]) + 1
    assert nu == far.size
    grad, inv = ce.embedding_backward(gy, nu, t_idx, t_sid, remap)
    c_grad, c_inv = ce.embedding_backward(gy, nu, c_idx, c_sid, c_remap)
    assert np.array_equal(inv.cpu().numpy(), far) and np.array_equal(c_inv.cpu().numpy(), np.arange(nu))
    same_bits(grad, c_grad, "compressed gradient")
    want, _ = oracle.embedding_backward(gy.cpu().numpy(), width, nu, c_idx.cpu().numpy(), c_sid.cpu().numpy(), c_remap.cpu().numpy())
    assert np.array_equal(grad.cpu().numpy(), want)


# ---- optimizer -------------------------------------------------------------------------------------------------------
OPTIMIZER_CASES = F.optimizer_cases()
HYPER = dict(lr=0.05, eps=1e-6, bias_factor=0.7, betas=(0.9, 0.99), weight_decay=0.01)


def _state_data(rule, n, width, rng):
    out = []
    for k, what in enumerate(F.STATE[rule]):
        shape = (n, width) if what == "e" else (n,)
        if rule in ("adam", "rowwise_adam") and k == 0:
            out.append((rng.standard_normal(shape) * 0.1).astype(np.float32))
        else:
            out.append(rng.uniform(0.05, 0.6, shape).astype(np.float32))
    return out


@pytest.mark.parametrize("kind,width,scheme,rule", OPTIMIZER_CASES, ids=["%s-W%d-%s-%s" % c for c in OPTIMIZER_CASES])
def test_optimizer_step_updates_far_rows(ce, oracle, arena, kind, width, scheme, rule):
    """Table and states share the arena (far_rows.optimizer_views).  The step's bits are the fp32 model's
    (optimizer_bits_reference) on the compact copy -- with stochastic rounding the model rounds with the TRUE row id,
    which enters the Philox counter.  Picked rows that no id names keep their bits; the poison stays."""
    dtype = TORCH[kind]
    views = F.optimizer_views(kind, width, scheme, rule)
    table = tensor_of(arena, views[0], dtype)
    states = [tensor_of(arena, v, torch.float32) for v in views[1:]]
    states = [s if what == "e" else s.view(-1) for s, what in zip(states, F.STATE[rule])]
    adam = rule in ("adam", "rowwise_adam")
    rng = np.random.default_rng(width)
    for idt in (np.int64, np.int32):
        layout, rows = F.pick_shared(views, seed=101 + width, below=INT32 if idt == np.int32 else None)
        if idt == np.int32 and max(rows) * width < INT32:
            continue                                                   # (4-byte rows: int32 ids stay below 2^31 elements)
        n = len(rows)
        named = np.asarray([k for k in range(n) if k not in (2, n - 3)])
        named = named[rng.permutation(named.size)]
        ids = np.asarray(rows, dtype=np.int64)[named]
        for stochastic in ((False, True) if kind != "f32" else (False,)):
            table_o, table_d = make(oracle, kind, rng.uniform(-1, 1, (n, width)))
            grads_o, grads_d = make(oracle, kind, rng.uniform(-0.5, 0.5, (named.size, width)))
            state_np = _state_data(rule, n, width, rng)
            poison(arena, layout, table_d)
            put_rows(table, rows, table_d)
            for s, data in zip(states, state_np):
                put_rows(s, rows, dev(data))
            rounding = dict(stochastic_rounding=True, seed=0x1234ABCD5678, step=(1 << 33) + 7) if stochastic else {}
            if adam:
                ce.sparse_row_adam(table, dev(ids.astype(idt)), grads_d, exp_avg=states[0], exp_avg_sq=states[1],
                                   rowwise=rule == "rowwise_adam", **HYPER, **rounding)
                hyper = HYPER
            else:
                ce.sparse_row_update(table, dev(ids.astype(idt)), grads_d, rule=rule, lr=HYPER["lr"], eps=HYPER["eps"],
                                     state=states[0] if states else None, **rounding)
                hyper = dict(lr=HYPER["lr"], eps=HYPER["eps"])
            bits = M.BITS[kind]
            want_t, want_s, trace = M.step(rule, kind, np.ascontiguousarray(table_o).view(bits), [s.view(np.uint32) for s in state_np],
                                           named, np.ascontiguousarray(grads_o).view(bits), np.arange(named.size), **hyper)
            if stochastic:
                want_t[named] = M.store(trace["x"], kind, "stochastic", rounding["seed"], rounding["step"], ids)
            label = (idt.__name__, stochastic)
            got_t = ibits(get_rows(table, rows)).cpu().numpy().view(bits)
            assert np.array_equal(got_t, want_t), label
            assert not np.array_equal(got_t[named], np.ascontiguousarray(table_o).view(bits)[named])
            for s, want in zip(states, want_s):
                assert np.array_equal(ibits(get_rows(s, rows)).cpu().numpy().view(np.uint32), want), label
            poison_intact(arena, layout)


# ---- small things ------------------------------------------------------------------------------------------------------
def test_row_cache_translation_reads_slots_past_2_31(ce, arena):
    """slot_of_row of 2^31 + 8 entries: ids at and past 2^31 find their slots, ids outside the table pass through."""
    view = F.View("slot_of_row", F.GUARD, 4, 1, rows=INT32 + 8)
    slots = tensor_of(arena, view, torch.int32).view(-1)
    layout, (rows,) = F.pick([view], seed=111)
    assert INT32 in rows and INT32 + 7 in rows
    poison(arena, layout)                                             # (0x3B3B3B3B >= 0: a narrowed read returns a wrong slot)
    slot_of = {r: (k if k % 3 else -1) for k, r in enumerate(rows)}
    for r, s in slot_of.items():
        slots[r].fill_(s)
    offset = (1 << 36) + 12345
    outside = [INT32 + 8, (1 << 32) + 1, (1 << 40), -5]
    for idt in (torch.int64, torch.int32):
        ids = [r for r in rows if idt == torch.int64 or r < INT32] * 3 + ([] if idt == torch.int32 else outside)
        idx = torch.tensor(ids, dtype=idt, device="cuda")
        out = torch.empty(idx.shape, dtype=torch.int64, device="cuda")
        ce._lib.lib().cuembed_translate_indices_for_row_cache(
            ctypes.c_void_p(idx.data_ptr()), 0 if idt == torch.int32 else 1, idx.numel(), ctypes.c_void_p(slots.data_ptr()),
            view.rows, offset, ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        want = [offset + slot_of[r] if slot_of.get(r, -1) >= 0 else r for r in ids]
        assert out.cpu().tolist() == want


@pytest.mark.parametrize("categories,nnz", (((1 << 31) + 5, 40_000), ((1 << 32) + 5, 270_000)), ids=["bit32", "bit33"])
def test_transpose_sorts_keys_with_bits_32_and_33(ce, categories, nnz):
    rng = np.random.default_rng(nnz)
    cols = rng.integers(0, categories, nnz)
    cols[:8] = [categories - 1, 0, INT32 - 1, INT32, categories - 5, INT32 + 1, 1, categories - 1]
    cols[rng.choice(nnz, nnz // 4, replace=False)] = rng.integers(INT32, categories, nnz // 4)    # bit 31 / 32 set often
    rows = np.arange(nnz, dtype=np.int64)
    t_cols, t_rows, _ = ce.transpose(dev(rows), dev(cols), num_categories=categories)
    order = np.argsort(cols, kind="stable")
    assert np.array_equal(t_cols.cpu().numpy(), cols[order]) and np.array_equal(t_rows.cpu().numpy(), order)
    plain, plain_rows, _ = ce.transpose(dev(rows), dev(cols))
    assert torch.equal(plain, t_cols) and torch.equal(plain_rows, t_rows)


def test_row_load_decision_sees_the_high_word(ce):
    """2^18 int64 ids k << 32 are all distinct: "streaming" for a table of 2 GiB.  With the high word cleared they are
    one row: "default"."""
    ids = torch.arange(1 << 18, dtype=torch.int64, device="cuda") << 32
    assert int(ce.decide_row_loads(ids, 2 << 30)[0]) == 1
    assert int(ce.decide_row_loads(ids & 0xFFFFFFFF, 2 << 30)[0]) == 0
    assert int(ce.decide_row_loads(ids >> 32, 2 << 30)[0]) == 1
