"""The two promises of every call that takes a scratch buffer (include/cuembed_amd.h, "Two-phase workspace"), on the
device: a buffer of EXACTLY the queried size is enough, and what it holds on entry does not matter.

Every call below is made the way a C caller makes it -- the size queried through the same entry point with the same
parameters and work == NULL -- on a workspace of exactly that size between two 64 KiB guard bands
(tests/scratch_guard.py), at the weakest alignment the header promises to accept (8 bytes), holding zeros, 0xFF, seeded
random bytes, or what a previous, larger call of the same function on another key type left there ("stale": the bytes
from its workspace's start, as a re-used buffer shows them; "stale_tail": its last bytes, where the sort keeps its
state words and counters).  Every output sits between guards of its own, every input is compared bit for bit with a
copy taken before the call, every result is compared with plain numpy (stable argsort, cumsum of run heads,
argsort of -min(length, bound)) and must be the same for every fill, and cuembed_peek_last_error() stays 0.  Integers
and moved bit patterns only: no tolerance anywhere.

Who writes each workspace region first, and who reads or waits on it (R = read within the call, W = waited on).
Lines are of cuembed_amd/csrc/cuembed/include/.  "pass 0" launches always run; a pass > 0 may be skipped on the device.

RadixSortPlan (radix_sort_kernels.hpp:1043) -- the one-workgroup sort (n <= 4,096, block_sort_kernels.hpp) takes no
workspace pointer at all (radix_sort_kernels.hpp:1107-1112).
  region      regime                 first written by                                              read by
  keys_tmp,   chained                RadixScatterBody StoreRouted, pass 0 (:751, :791, :796)        R later passes :675/:690/:795; 32-bit
  v1_tmp,                                                                                          keys and payloads are ALSO requested
  v2_tmp                                                                                           from `tmp` and `out` before the route
                                                                                                   is known (:644-648) and the wrong one
                                                                                                   is dropped (:653, :687): the value of
                                                                                                   an unwritten element is never used
              tiled / folded scan    the same stores, pass 0 launch (:1179)                        R :247 (histogram), :675 (scatter)
              high word, one launch  the same stores, inside RadixHighPassesKernel (:958, :994)    R :940, :958, :994
  tile_hist   chained                RadixTileHistogramBody, pass 0: its own pass's counts (:308)  R :705 (every scatter pass adds them up);
                                     and ZEROES the words of every later pass (:309)               atomically added to by :776
              tiled, folded scan     RadixTileHistogramBody :311, every working pass (:1173)       R :720 (scatter adds the raw counts)
              tiled                  the same, :311                                                R+W in place :428-443 (scan), R :712
              high word, one launch  :311 through :940                                             R :949 (scan), :958 (scatter)
              sample blocks          as tiled; the scan runs per (segment, bin) :413-417           R :712
  bin_total   tiled                  RadixScanTilesBody :448, every working pass                   R :713
              chained, folded scan   never written                                                 never read (nullptr at :1154, :1180)
  tile_bits   chained                RadixTileHistogramBody pass 0 :321-323 (device state only)    R :601-603 (scatter pass 0)
              tiled (all)            the same                                                      R :378-380 (extra scan workgroup)
              fixed route (<= 3      never written                                                 never read (nullptr, :1132-1135)
              passes, narrow v1)
  varying     chained                RadixScatterBody pass 0, block 0 :628-630                     R PlanPass :144 in every later launch
  (3 state    tiled (all)            RadixScanTilesBody extra workgroup of pass 0 :404-406         R PlanPass :144 from the pass-0 scatter on
  words)
  varying     chained                ZeroSortBarrier :631 (same store site as the state words)     R+W SortWorkQueue :864, :870, :881, only
  (ticket,    tiled                  ZeroSortBarrier :407                                          in the high-word kernels (:916, :977),
  done)                                                                                            which are LATER launches on the stream
  remap after the sort               RunHeadScan re-uses work[0 .. tiles * 4) (:1163, :1191): see RunHeadScanWorkBytes
RunHeadScanWorkBytes (radix_sort_kernels.hpp:1466)
  tile_sum    <= 4 tiles; <= 16      never written (RunHeadScanKernel<kSelfCount> :1479,           never read (tile_count == nullptr :1364)
              (int64: 8) tiles       RunHeadScanWideKernel :1486)
              more tiles             RunHeadCountKernel :1256, every tile                          R :1362 (or :1360 after the prefix
                                                                                                   kernel :1267-1270, > 4,096 tiles)
BlockedRemapPlan (blocked_remap_kernels.hpp:34)
  tile_sum       RunHeadCountKernel radix_sort_kernels.hpp:1256                                    R :1362
  unique_keys    RunHeadScanKernel<kCompact> :1391, entries [0, M)                                 R blocked_remap_kernels.hpp:100, :169, :181
                                                                                                   (an index past M is only ever read
                                                                                                   into a value that is not used)
  fence_keys     RunHeadScanKernel<kCompact> :1392                                                 R blocked_remap_kernels.hpp:124
  block_start    RunHeadScanKernel<kCompact> :1395, :1397: every block's start and the total      R :85, :218, :244
  lower_bounds   BlockedRankSearchKernel :185, valid entries of the other blocks                  R :296, the same entries
  masks,         BlockedRankSearchKernel :195, :208, :209: all 16 words of every ACTIVE tile      R :254, :272, :307 (active tiles only)
  word_prefix,
  tile_count
  num_unique     BlockedRankFinishKernel :311                                                      never read
Bag order (index_transforms.hpp:331)
  chunk_hist     BagChunkHistogramKernel hint_kernels.hpp:141: all 256 counts of every chunk,      R hint_kernels.hpp:173
                 empty bins included (from the zeroed LDS histogram :133)
  keys           BagLengthKeysKernel index_transforms.hpp:316 (general path)                       R by the sort (its input)
  sorted_keys    the sort's key output                                                             never read
  sort           RadixSortPlan above (int32 keys, implicit payload)
RowCachePlan (row_cache.hpp:112)
  keys           CacheKeysKernel row_cache_kernels.hpp:101, every lookup; CacheHitKernel :126      R sort input; R :200 (place), the first
                 then writes the distinct keys over them                                           *last_run + 1 entries
  sorted         the sort's key output                                                             R :122
  order          the sort's payload output, then CacheRunIds' output (row_cache.hpp:259-261)       R :122-126, :184 (*last_run)    
  moves          CachePlaceKernel row_cache_kernels.hpp:217, :242, :257: entries [0, move count)   R :319, the same entries (:310)
  sort           RadixSortPlan above, then RunHeadScanWorkBytes (row_cache.hpp:118-120)
No region is read or waited on before a launch of the same call has written it; nothing had to be fixed.  The
alignment every plan needs from `work` is 8 bytes (the regions start at multiples of 256 from it and the widest access
is one 64-bit word): the header now says so.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import dynamic_row_cache_reference as M
import scratch_guard as G

pytestmark = pytest.mark.gpu

NP = {"i32": np.int32, "i64": np.int64}
TT = {"i32": torch.int32, "i64": torch.int64}
CODE = {"i32": 0, "i64": 1}                    # CUEMBED_I32 / CUEMBED_I64
WEIGHTS = {"none": None, "f32": np.float32, "f16": np.float16}
WCODE = {"none": 0, "f32": 0, "f16": 1}        # CUEMBED_F32 / CUEMBED_F16
SHARED_ROW_BIT = 1 << 30
VP = ctypes.c_void_p
CI = ctypes.c_int


@pytest.fixture(scope="module")
def ce():
    import cuembed_amd
    assert torch.cuda.is_available()
    return cuembed_amd


def lib():
    import cuembed_amd
    return cuembed_amd._lib.lib()


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ptr(t):
    return None if t is None else VP(t.data_ptr())


def stream():
    return VP(torch.cuda.current_stream().cuda_stream)


def bits(t):
    """The tensor as integers of its element size (bit-for-bit comparison of weights)."""
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def np_bits(a):
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def clean_exit():
    torch.cuda.synchronize()
    assert lib().cuembed_peek_last_error() == 0


# ---- the shared driver ---------------------------------------------------------------------------------------------
def call_args(args, work, lwork):
    """The argument list of a call: "work" / "lwork" markers replaced, tensors by their addresses."""
    out = []
    for a in args:
        if isinstance(a, str):
            out.append({"work": work, "lwork": ctypes.byref(lwork)}[a])
        else:
            out.append(ptr(a) if isinstance(a, torch.Tensor) else a)
    return out


def query(entry, *args):
    """Phase one, as a C caller does it: the same entry point and parameters, work == NULL; returns *lwork."""
    lwork = ctypes.c_size_t(0)
    entry(*call_args(args, None, lwork))
    return int(lwork.value)


def confined(what, entry, make_args, inputs, outputs, want, stale=None, fills=G.FILLS):
    """Query, then run `entry` once per fill on a guarded workspace of exactly the queried size, with guarded outputs.
      make_args(tensors) -> the argument list with "work" / "lwork" markers; tensors maps the names of `inputs`
      (device tensors or None) and `outputs` (name -> (shape, torch dtype)) to tensors;
      want: name -> numpy array that out[name].reshape(-1)[:want.size] must equal bit for bit.
    Returns the queried size."""
    before = {k: v.clone() for k, v in inputs.items() if v is not None}
    names = sorted(want)
    all_fills = list(fills) + (["stale", "stale_tail"] if stale is not None else [])
    sizes = []

    def one(fill):
        outs, checks = {}, {}
        for k, (shape, dtype) in outputs.items():
            outs[k], checks[k] = G.guarded_like(shape, dtype, fill="ones" if fill == "zeros" else "random",
                                                seed=all_fills.index(fill))
        tensors = dict(inputs)
        tensors.update(outs)
        need = query(entry, *make_args(tensors))
        sizes.append(need)
        if fill in ("stale", "stale_tail"):
            assert stale.numel() > need, "the previous call must be the larger one"
            work, check_work = G.guarded_bytes(need)
            work.copy_(stale[:need] if fill == "stale" else stale[stale.numel() - need:])
        else:
            work, check_work = G.guarded_bytes(need, fill=fill, seed=len(what))
        assert work.numel() == need and (need == 0 or work.data_ptr() % 16 == G.WORK_ALIGN)
        entry(*call_args(make_args(tensors), ptr(work), ctypes.c_size_t(need)))
        torch.cuda.synchronize()
        check_work("%s, fill %s: workspace" % (what, fill))
        for k in outs:
            checks[k]("%s, fill %s: output %s" % (what, fill, k))
        for k, v in before.items():
            assert torch.equal(bits(inputs[k]), bits(v)), "%s, fill %s: input %s was modified" % (what, fill, k)
        return tuple(outs[k].reshape(-1)[:want[k].size].cpu().numpy() for k in names)

    try:
        got = G.same_for_every_fill(one, all_fills)
    except AssertionError as e:
        if "depends on what the workspace held" in str(e):
            raise AssertionError("%s: %s (results %r)" % (what, e, names)) from None
        raise
    for k, g in zip(names, got):
        assert np.array_equal(np_bits(g), np_bits(want[k].reshape(-1))), "%s: %s is not numpy's" % (what, k)
    assert len(set(sizes)) == 1
    assert lib().cuembed_peek_last_error() == 0
    return sizes[0]


def run_heads(sorted_keys, block_len=0):
    """cumsum of run heads: the dense id of every element's run; block_len > 0 makes every block start a head."""
    n = sorted_keys.size
    heads = np.zeros(n, dtype=np.int64)
    heads[1:] = sorted_keys[1:] != sorted_keys[:-1]
    if block_len > 0:
        heads[block_len::block_len] = 1
    return np.cumsum(heads)


def blocked_order(cols, block_len):
    """The stable order of every block of block_len elements on its own."""
    return np.concatenate([at + np.argsort(cols[at:at + block_len], kind="stable") for at in range(0, cols.size, block_len)])


def key_sets(rng, n, index):
    """(name, keys, index_bits): the key sets every sort below runs on.  index_bits 0 = all bits of the type."""
    dt = NP[index]
    info = np.iinfo(dt)
    yield "rows10M", rng.integers(0, 10_000_000, n).astype(dt), 24          # three working passes
    yield "rows65537", rng.integers(0, 65_537, n).astype(dt), 17            # three, the top one nearly constant
    yield "rows65536", rng.integers(0, 65_536, n).astype(dt), 16            # two
    yield "full", rng.integers(info.min, info.max, n, endpoint=True).astype(dt), 0
    yield "equal", np.full(n, 77_777, dtype=dt), 0                          # every pass is skipped: a copy
    if index == "i64":
        yield "wide", rng.integers(1 << 32, 1 << 45, n).astype(dt), 0


def weights_of(rng, n, kind):
    return None if WEIGHTS[kind] is None else rng.uniform(-1, 1, n).astype(WEIGHTS[kind])


def hots_of(n):
    return next(h for h in (7, 5, 4, 3, 2, 1) if n % h == 0)


SIZES = (4096, 4097, 17409, 229376, 229377, 270001)
PREVIOUS = 600_001        # the "stale" previous call: larger than every size here, tiled, in two sample blocks


def transpose_remapped_args(index, wkind, n, index_bits, row_bits, blocks, remap):
    def make(t):
        return [t["rows"], t["cols"], t["weights"], n, CODE[index], WCODE[wkind], t["t_rows"], t["t_cols"],
                t["t_w"] if wkind != "none" else None, t["remap"] if remap else None, "work", "lwork", index_bits,
                row_bits, blocks, stream()]
    return make


def previous_workspace(index, kind="transpose"):
    """What a larger call of the same function on the OTHER key type leaves in its workspace (cloned after it ran)."""
    L = lib()
    other = "i32" if index == "i64" else "i64"
    rng = np.random.default_rng(99)
    n = PREVIOUS
    info = np.iinfo(NP[other])
    cols = dev(rng.integers(info.min, info.max, n, endpoint=True).astype(NP[other]))
    if kind == "compress":
        cols = cols.sort().values
        need = query(L.cuembed_compute_compressed_grad_indices, cols, n, CODE[other], cols, "work", "lwork", None)
        work = torch.empty(need, dtype=torch.uint8, device="cuda")
        out = torch.empty_like(cols)
        L.cuembed_compute_compressed_grad_indices(ptr(cols), n, CODE[other], ptr(out), ptr(work),
                                                  ctypes.byref(ctypes.c_size_t(need)), stream())
    else:
        w = dev(rng.uniform(-1, 1, n).astype(np.float32))
        rows = dev(np.arange(n).astype(NP[other]))
        outs = [torch.empty_like(cols), torch.empty_like(cols), torch.empty_like(w), torch.empty_like(cols)]
        need = query(L.cuembed_transpose_remapped, rows, cols, w, n, CODE[other], 0, cols, cols, w, cols, "work", "lwork",
                     0, 0, 2, None)
        work = torch.empty(need, dtype=torch.uint8, device="cuda")
        L.cuembed_transpose_remapped(ptr(rows), ptr(cols), ptr(w), n, CODE[other], 0, *[ptr(o) for o in outs], ptr(work),
                                     ctypes.byref(ctypes.c_size_t(need)), 0, 0, 2, stream())
    torch.cuda.synchronize()
    return work.clone()


@pytest.fixture(scope="module")
def stale_transpose():
    return {index: previous_workspace(index) for index in ("i32", "i64")}


# ---- Transpose family ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("index", ["i32", "i64"])
def test_transpose_remapped(ce, stale_transpose, index, n):
    L = lib()
    rng = np.random.default_rng(n)
    for name, cols, index_bits in key_sets(rng, n, index):
        order = np.argsort(cols, kind="stable")
        wide = name == "wide"
        rows = (rng.integers(1 << 32, 1 << 50, n) if wide else rng.integers(0, n, n)).astype(NP[index])
        want_remap = run_heads(cols[order]).astype(NP[index])
        for wkind in WEIGHTS:
            w = weights_of(rng, n, wkind)
            inputs = dict(rows=dev(rows), cols=dev(cols), weights=dev(w))
            for remap in (False, True):
                for row_bits in ((0, max(1, int(n - 1).bit_length())) if index == "i64" and not wide else (0,)):
                    outputs = dict(t_rows=(n, TT[index]), t_cols=(n, TT[index]))
                    want = dict(t_rows=cols[order], t_cols=rows[order])
                    if w is not None:
                        outputs["t_w"] = (n, inputs["weights"].dtype)
                        want["t_w"] = w[order]
                    if remap:
                        outputs["remap"] = (n, TT[index])
                        want["remap"] = want_remap
                    confined("transpose_remapped %s n=%d %s w=%s remap=%d row_bits=%d" % (index, n, name, wkind, remap, row_bits),
                             L.cuembed_transpose_remapped,
                             transpose_remapped_args(index, wkind, n, index_bits, row_bits, 1, remap), inputs, outputs,
                             want, stale=stale_transpose[index])
    clean_exit()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("index", ["i32", "i64"])
def test_transpose_fixed_hotness_remapped(ce, stale_transpose, index, n):
    L = lib()
    rng = np.random.default_rng(n + 1)
    hots = hots_of(n)
    sample = (np.arange(n) // hots).astype(NP[index])
    for name, cols, index_bits in key_sets(rng, n, index):
        order = np.argsort(cols, kind="stable")
        want_remap = run_heads(cols[order]).astype(NP[index])
        for wkind in WEIGHTS:
            w = weights_of(rng, n, wkind)
            inputs = dict(indices=dev(cols), weights=dev(w))
            for remap in (False, True):
                outputs = dict(t_idx=(n, TT[index]), t_sid=(n, TT[index]))
                want = dict(t_idx=cols[order], t_sid=sample[order])
                if w is not None:
                    outputs["t_w"] = (n, inputs["weights"].dtype)
                    want["t_w"] = w[order]
                if remap:
                    outputs["remap"] = (n, TT[index])
                    want["remap"] = want_remap

                def make(t, wkind=wkind, remap=remap, index_bits=index_bits):
                    return [t["indices"], t["weights"], n // hots, hots, CODE[index], WCODE[wkind], t["t_idx"], t["t_sid"],
                            t["t_w"] if wkind != "none" else None, t["remap"] if remap else None, "work", "lwork",
                            index_bits, 1, stream()]
                confined("transpose_fixed_hotness_remapped %s n=%d %s w=%s remap=%d" % (index, n, name, wkind, remap),
                         L.cuembed_transpose_fixed_hotness_remapped, make, inputs, outputs, want,
                         stale=stale_transpose[index])
    clean_exit()


@pytest.mark.parametrize("n", SIZES)
def test_transpose_i64_f32_the_reference_signature(ce, stale_transpose, n):
    """cuembed_transpose_i64_f32: all 64 key bits whatever the keys hold -- eight passes, the high word in one launch."""
    L = lib()
    entry = L.cuembed_transpose_i64_f32
    entry.restype = None
    entry.argtypes = [VP, VP, VP, CI, VP, VP, VP, VP, ctypes.POINTER(ctypes.c_size_t), VP]
    rng = np.random.default_rng(n + 2)
    for name, cols, _ in key_sets(rng, n, "i64"):
        order = np.argsort(cols, kind="stable")
        rows = (rng.integers(1 << 32, 1 << 50, n) if name == "wide" else rng.integers(0, n, n)).astype(np.int64)
        for wkind in ("none", "f32"):
            w = weights_of(rng, n, wkind)
            inputs = dict(rows=dev(rows), cols=dev(cols), weights=dev(w))
            outputs = dict(t_rows=(n, torch.int64), t_cols=(n, torch.int64))
            want = dict(t_rows=cols[order], t_cols=rows[order])
            if w is not None:
                outputs["t_w"] = (n, torch.float32)
                want["t_w"] = w[order]

            def make(t, wkind=wkind):
                return [t["rows"], t["cols"], t["weights"], n, t["t_rows"], t["t_cols"],
                        t["t_w"] if wkind != "none" else None, "work", "lwork", stream()]
            confined("transpose_i64_f32 n=%d %s w=%s" % (n, name, wkind), entry, make, inputs, outputs, want,
                     stale=stale_transpose["i64"])
    clean_exit()


# ---- sample blocks ---------------------------------------------------------------------------------------------------
BLOCKED = ((139_281, 2), (270_001, 3))


@pytest.mark.parametrize("n,blocks", BLOCKED)
@pytest.mark.parametrize("index", ["i32", "i64"])
def test_transpose_in_sample_blocks(ce, stale_transpose, index, n, blocks):
    L = lib()
    rng = np.random.default_rng(n + 3)
    block_len = int(L.cuembed_transpose_sample_block_length(n, blocks))
    assert block_len % 4096 == 0 and -(-n // block_len) == blocks
    for name, cols, index_bits in key_sets(rng, n, index):
        order = blocked_order(cols, block_len)
        rows = rng.integers(0, n, n).astype(NP[index])
        want_remap = run_heads(cols[order]).astype(NP[index])       # (the sort's own remap knows no block starts)
        for wkind in ("none", "f32"):
            w = weights_of(rng, n, wkind)
            inputs = dict(rows=dev(rows), cols=dev(cols), weights=dev(w))
            for remap in (False, True):
                outputs = dict(t_rows=(n, TT[index]), t_cols=(n, TT[index]))
                want = dict(t_rows=cols[order], t_cols=rows[order])
                if w is not None:
                    outputs["t_w"] = (n, torch.float32)
                    want["t_w"] = w[order]
                if remap:
                    outputs["remap"] = (n, TT[index])
                    want["remap"] = want_remap
                confined("transpose_remapped %s n=%d blocks=%d %s w=%s remap=%d" % (index, n, blocks, name, wkind, remap),
                         L.cuembed_transpose_remapped, transpose_remapped_args(index, wkind, n, index_bits, 0, blocks, remap),
                         inputs, outputs, want, stale=stale_transpose[index])
    clean_exit()


def blocked_remap_reference(blocked, block_len):
    pairs = run_heads(blocked, block_len)
    heads = np.concatenate(([0], np.nonzero(np.diff(pairs))[0] + 1))
    keys = blocked[heads]
    uniq, rank = np.unique(blocked, return_inverse=True)
    first_block = np.full(uniq.size, 1 << 30)
    np.minimum.at(first_block, rank, np.arange(blocked.size) // block_len)
    shared = (heads // block_len) > first_block[rank[heads]]
    ids = rank[heads].astype(np.int64) | np.where(shared, SHARED_ROW_BIT, 0)
    assert np.array_equal(uniq[rank[heads]], keys)
    return pairs, ids.astype(np.uint32).view(np.int32), uniq.size


@pytest.mark.parametrize("n,blocks", BLOCKED + ((4097, 2),))
@pytest.mark.parametrize("index", ["i32", "i64"])
def test_compressed_grad_indices_blocked(ce, index, n, blocks):
    L = lib()
    rng = np.random.default_rng(n + 4)
    block_len = int(L.cuembed_transpose_sample_block_length(n, blocks))
    # the previous call: larger, three blocks, the other key type
    prev_n, other = PREVIOUS, "i32" if index == "i64" else "i64"
    prev_len = int(L.cuembed_transpose_sample_block_length(prev_n, 3))
    prev = rng.integers(0, 50_000, prev_n).astype(NP[other])
    prev = dev(prev[blocked_order(prev, prev_len)])
    prev_out = [torch.empty_like(prev), torch.empty(prev_n, dtype=torch.int32, device="cuda"),
                torch.empty(1, dtype=torch.int32, device="cuda")]
    need = query(L.cuembed_compute_compressed_grad_indices_blocked, prev, prev_n, CODE[other], 3, *prev_out, "work", "lwork",
                 stream())
    stale = torch.empty(need, dtype=torch.uint8, device="cuda")
    L.cuembed_compute_compressed_grad_indices_blocked(*call_args(
        [prev, prev_n, CODE[other], 3] + prev_out + ["work", "lwork", stream()], ptr(stale), ctypes.c_size_t(need)))
    torch.cuda.synchronize()
    for name, rows in (("skewed", 3_000), ("spread", 5_000_000), ("one", 1)):
        cols = rng.integers(0, rows, n).astype(NP[index])
        blocked = cols[blocked_order(cols, block_len)]
        pairs, ids, unique = blocked_remap_reference(blocked, block_len)
        inputs = dict(indices=dev(blocked))
        outputs = dict(remap=(n, TT[index]), block_row_ids=(n, torch.int32), num_unique=(1, torch.int32))
        want = dict(remap=pairs.astype(NP[index]), num_unique=np.array([unique], dtype=np.int32))
        if -(-n // block_len) > 1:
            want["block_row_ids"] = ids                     # (one block: not written)

        def make(t):
            return [t["indices"], n, CODE[index], blocks, t["remap"], t["block_row_ids"], t["num_unique"], "work", "lwork",
                    stream()]
        confined("compressed_grad_indices_blocked %s n=%d blocks=%d %s" % (index, n, blocks, name),
                 L.cuembed_compute_compressed_grad_indices_blocked, make, inputs, outputs, want, stale=stale)
    clean_exit()


# ---- ComputeCompressedGradIndices ------------------------------------------------------------------------------------
# 16,384 / 16,385: the one-launch limit of the run-head scan; 32,768 (int64) and 65,536 (int32): the limit of its
# 1024-thread one-launch form
@pytest.mark.parametrize("index", ["i32", "i64"])
def test_compressed_grad_indices(ce, index):
    L = lib()
    rng = np.random.default_rng(5)
    stale = previous_workspace(index, "compress")
    for n in (1, 4096, 4097, 16384, 16385, 32768, 32769, 65536, 65537, 270001):
        for name, rows in (("runs", n // 3 + 1), ("distinct", 0), ("one", 1)):
            cols = (np.sort(rng.integers(0, rows, n)) if rows else np.arange(n) * 3 - 5).astype(NP[index])
            inputs = dict(indices=dev(cols))
            outputs = dict(remap=(n, TT[index]))
            want = dict(remap=run_heads(cols).astype(NP[index]))

            def make(t):
                return [t["indices"], n, CODE[index], t["remap"], "work", "lwork", stream()]
            confined("compressed_grad_indices %s n=%d %s" % (index, n, name), L.cuembed_compute_compressed_grad_indices,
                     make, inputs, outputs, want, stale=stale)
    clean_exit()


# ---- BagOrderByLength ------------------------------------------------------------------------------------------------
def bag_offsets(rng, batch, lengths, dtype):
    lens = rng.choice(np.asarray(lengths), batch)
    return np.concatenate(([0], np.cumsum(lens))).astype(dtype), lens


def bag_order_reference(lens, max_length):
    bound = max_length if max_length > 0 else (255 if max_length < 0 else np.iinfo(np.int32).max)
    return np.argsort(-np.minimum(lens, bound), kind="stable").astype(np.int32)


def bag_previous(offset):
    """A larger general-path call on the other offset type: what it leaves in its workspace."""
    L = lib()
    other = "i32" if offset == "i64" else "i64"
    off, _ = bag_offsets(np.random.default_rng(6), 200_000, (0, 1, 2, 700), NP[other])
    need = query(L.cuembed_bag_order_by_length, VP(256), CODE[other], 200_000, 0, VP(256), "work", "lwork", None)
    work = torch.empty(need, dtype=torch.uint8, device="cuda")
    L.cuembed_bag_order_by_length(ptr(dev(off)), CODE[other], 200_000, 0, ptr(torch.empty(200_000, dtype=torch.int32, device="cuda")),
                                  ptr(work), ctypes.byref(ctypes.c_size_t(need)), stream())
    torch.cuda.synchronize()
    return work


@pytest.mark.parametrize("offset", ["i32", "i64"])
def test_bag_order_by_length(ce, offset):
    L = lib()
    rng = np.random.default_rng(7)
    stale = bag_previous(offset)
    # counting sort: lengths that leave most of the 256 bins of a chunk empty -- they must come out of a 0xFF-filled
    # chunk_hist as zero; general path: more samples than the counting sort takes, and a bound beyond 255
    cases = [(batch, bound, (0, 3, 7, 300)) for batch in (1, 1023, 1025, 131_072) for bound in (9, 255, -1)]
    cases += [(131_073, 59, (0, 1, 58, 59, 90)), (20_000, 2_999, (0, 5, 2_998, 2_999, 4_000))]
    for batch, bound, lengths in cases:
        off, lens = bag_offsets(rng, batch, lengths, NP[offset])
        inputs = dict(offsets=dev(off))
        outputs = dict(order=(batch, torch.int32))
        want = dict(order=bag_order_reference(lens, bound))

        def make(t):
            return [t["offsets"], CODE[offset], batch, bound, t["order"], "work", "lwork", stream()]
        need = confined("bag_order_by_length %s batch=%d bound=%d" % (offset, batch, bound), L.cuembed_bag_order_by_length,
                        make, inputs, outputs, want, stale=stale)
        if bound <= 255 and batch <= 131_072:
            assert need == -(-batch // 1024) * 256 * 4            # the counting sort's chunk_hist and nothing else
    clean_exit()


# ---- row-cache prefetch ----------------------------------------------------------------------------------------------
def make_cache(planes, num_sets, seed=7):
    from cuembed_amd.row_cache import AdamRowCache, DynamicRowCache
    rng = np.random.default_rng(seed)
    table = torch.from_numpy(rng.integers(-8, 9, (M.ROWS, 16)).astype(np.float32)).pin_memory()
    if planes == 0:
        return table, DynamicRowCache(table, "cuda", num_sets=num_sets)
    if planes == 1:
        state = torch.from_numpy(rng.integers(0, 9, (M.ROWS, 16)).astype(np.float32)).pin_memory()
        return table, DynamicRowCache(table, "cuda", num_sets=num_sets, rule="adagrad", state=state)
    moments = [torch.from_numpy(rng.integers(0, 9, (M.ROWS, 16)).astype(np.float32)).pin_memory() for _ in range(2)]
    return table, AdamRowCache(table, "cuda", num_sets=num_sets, exp_avg=moments[0], exp_avg_sq=moments[1])


def cache_state(cache):
    stats = cache.stats()
    return (cache.tags.cpu().numpy().copy(), cache.stamps.view(torch.int32).cpu().numpy().copy(),
            cache.dirty.cpu().numpy().copy(), cache.slot_of_row.cpu().numpy().copy(),
            np.array([stats[k] for k in M.COUNTERS] + [stats["clock"]], dtype=np.int64))


@pytest.mark.parametrize("planes", [0, 1, 2], ids=["rows", "one_state_plane", "two_state_planes"])
@pytest.mark.parametrize("num_sets,index", [(1, "i32"), (4, "i64")])
def test_row_cache_prefetch(ce, planes, num_sets, index):
    """One set of 64 ways (every batch of 320 lookups overflows it) and four sets with a batch of 70 rows of one set:
    the cache's whole state after every prefetch equals the Python model's and is the same for every fill."""
    L = lib()
    batches = [(idx, fu) for idx, fu in zip(M.batches(), M.FOR_UPDATE)]
    conflict = np.resize(np.concatenate([M.conflict_rows(num_sets, num_sets // 2, 70), np.arange(20)]), (18, 5))
    batches.insert(2, (conflict.astype(np.int64), True))
    model = M.CacheModel(M.ROWS, num_sets)
    snapshots = []
    for idx, for_update in batches:
        model.prefetch(idx, for_update)
        snapshots.append((model.tags.copy(), model.stamps.copy(), model.dirty.copy(), model.slot_of_row.copy(),
                          np.array([model.counters[k] for k in M.COUNTERS] + [model.clock], dtype=np.int64)))
    assert model.counters["unplaced"] > 0 and model.counters["evictions"] > 0 and model.counters["hits"] > 0

    def one(fill):
        table, cache = make_cache(planes, num_sets)
        got = []
        for step, ((idx, for_update), snapshot) in enumerate(zip(batches, snapshots)):
            d_idx = torch.from_numpy(idx).to(TT[index]).cuda()
            kept = d_idx.clone()
            need = int(L.cuembed_row_cache_workspace_bytes(d_idx.numel(), M.ROWS, num_sets))
            if fill == "stale" and step > 0:                      # what the previous prefetch left, repeated to this size
                work, check = G.guarded_bytes(need)
                work.copy_(left.repeat(-(-need // left.numel()))[:need])
            else:
                work, check = G.guarded_bytes(need, fill="random" if fill == "stale" else fill, seed=step)
            cache._work = work                                    # (prefetch keeps a buffer that is large enough)
            cache.prefetch(d_idx, for_update=for_update)
            torch.cuda.synchronize()
            assert cache._work is work and work.numel() == need
            check("row-cache prefetch, %d planes, step %d, fill %s: workspace" % (planes, step, fill))
            assert torch.equal(d_idx, kept)
            state = cache_state(cache)
            for k, (a, b) in enumerate(zip(state, snapshot)):
                assert np.array_equal(a.reshape(-1), np.asarray(b).reshape(-1).astype(a.dtype)), (
                    "row-cache prefetch, %d planes, step %d, fill %s: %s differ from the model's" % (
                        planes, step, fill, ("tags", "stamps", "dirty bytes", "slot_of_row", "counters and clock")[k]))
            slots = np.nonzero(state[0].reshape(-1) >= 0)[0]
            rows = state[0].reshape(-1)[slots]
            assert torch.equal(cache.cache.cpu()[slots], table[rows])
            if planes == 1:
                assert torch.equal(cache.state_cache.cpu()[slots], cache.state[rows])
            if planes == 2:
                assert torch.equal(cache.exp_avg_cache.cpu()[slots], cache.exp_avg[rows])
                assert torch.equal(cache.exp_avg_sq_cache.cpu()[slots], cache.exp_avg_sq[rows])
            got.extend(state)
            left = work.clone()
        return tuple(got)

    G.same_for_every_fill(one, G.FILLS + ("stale",))
    clean_exit()


# ---- the Python wrappers: their own query covers the call they make --------------------------------------------------
@pytest.mark.parametrize("index", ["i32", "i64"])
def test_python_wrappers_query_what_they_call(ce, index):
    L = lib()
    rng = np.random.default_rng(8)
    for n, blocks in ((4097, 1), (229_376, 1), (270_001, 1)) + BLOCKED:
        block_len = int(L.cuembed_transpose_sample_block_length(n, blocks))
        hots = hots_of(n)
        sample = (np.arange(n) // hots).astype(NP[index])
        for ncat in (10_000_000, 65_537, None):
            info = np.iinfo(NP[index])
            cols = (rng.integers(0, ncat, n) if ncat else rng.integers(info.min, info.max, n, endpoint=True)).astype(NP[index])
            rows = rng.integers(0, n, n).astype(NP[index])
            order = blocked_order(cols, block_len)
            for wkind in WEIGHTS:
                w = weights_of(rng, n, wkind)
                wt = None if w is None else torch.from_numpy(w).dtype
                need = ce.transpose_workspace_bytes(n, TT[index], wt)

                def one(fill):
                    work, check = G.guarded_bytes(need, fill=fill, seed=n)
                    got = ce.transpose(dev(rows), dev(cols), dev(w), workspace=work, num_categories=ncat, num_rows=n,
                                       sample_blocks=blocks, remapped=True)
                    torch.cuda.synchronize()
                    check("ops.transpose n=%d blocks=%d, fill %s" % (n, blocks, fill))
                    work2, check2 = G.guarded_bytes(need, fill=fill, seed=n + 1)
                    fixed = ce.transpose_fixed_hotness(dev(cols), n // hots, hots, dev(w), workspace=work2,
                                                       num_categories=ncat, sample_blocks=blocks, remapped=True)
                    torch.cuda.synchronize()
                    check2("ops.transpose_fixed_hotness n=%d blocks=%d, fill %s" % (n, blocks, fill))
                    return tuple(None if t is None else t.cpu().numpy() for t in got + fixed)

                got = G.same_for_every_fill(one)
                assert np.array_equal(got[0], cols[order]) and np.array_equal(got[1], rows[order])
                assert np.array_equal(got[4], cols[order]) and np.array_equal(got[5], sample[order])
                if w is not None:
                    assert np.array_equal(np_bits(got[2]), np_bits(w[order])) and np.array_equal(np_bits(got[6]), np_bits(w[order]))
                assert np.array_equal(got[3], run_heads(cols[order])) and np.array_equal(got[7], got[3])
            # the remaps on the sorted array
            blocked = cols[order]
            pairs, ids, unique = blocked_remap_reference(blocked, block_len)
            need_plain = ce.compressed_grad_workspace_bytes(n, TT[index])
            need_blocked = ce.compressed_grad_blocked_workspace_bytes(n, TT[index], blocks)

            def remaps(fill):
                work, check = G.guarded_bytes(need_plain, fill=fill, seed=n)
                plain = ce.compute_compressed_grad_indices(dev(blocked), workspace=work)
                work2, check2 = G.guarded_bytes(need_blocked, fill=fill, seed=n + 1)
                ids_out, check_ids = G.guarded_like(n, torch.int32, seed=2)
                count, check_count = G.guarded_like(1, torch.int32, seed=3)
                remap, _, _ = ce.compute_compressed_grad_indices_blocked(dev(blocked), blocks, workspace=work2,
                                                                         num_unique=count, block_row_ids=ids_out)
                torch.cuda.synchronize()
                for c in (check, check2, check_ids, check_count):
                    c("ops.compute_compressed_grad_indices[_blocked] n=%d blocks=%d, fill %s" % (n, blocks, fill))
                return (plain.cpu().numpy(), remap.cpu().numpy(), count.cpu().numpy(),
                        ids_out.cpu().numpy()[:pairs[-1] + 1] if blocks > 1 else None)

            got = G.same_for_every_fill(remaps)
            assert np.array_equal(got[0], run_heads(blocked)) and np.array_equal(got[1], pairs) and got[2][0] == unique
            if blocks > 1:
                assert np.array_equal(got[3], ids)
    for offset in ("i32", "i64"):
        for batch, bound, lengths in ((1025, 255, (0, 3, 7, 300)), (131_072, -1, (0, 3, 7, 300)), (20_000, 2_999, (5, 2_999, 4_000)),
                                      (20_000, None, (5, 2_999, 4_000))):
            off, lens = bag_offsets(rng, batch, lengths, NP[offset])
            need = query(L.cuembed_bag_order_by_length, None, CODE[offset], batch, bound or 0, None, "work", "lwork", None)

            def bag(fill):
                work, check = G.guarded_bytes(need, fill=fill, seed=batch)
                order = ce.bag_order_by_length(dev(off), max_length=bound, workspace=work)
                torch.cuda.synchronize()
                check("ops.bag_order_by_length batch=%d, fill %s" % (batch, fill))
                return (order.cpu().numpy(),)

            assert np.array_equal(G.same_for_every_fill(bag)[0], bag_order_reference(lens, bound or 0))
    clean_exit()


# ---- graph replay ----------------------------------------------------------------------------------------------------
def test_graph_replay_on_rewritten_workspaces(ce):
    """transpose_fixed_hotness(remapped=True) and bag_order_by_length captured as ONE chain on a side stream: every
    replay gives numpy's result for the indices of the moment, whatever was written into the workspaces in between."""
    L = lib()
    rng = np.random.default_rng(9)
    n, hots, ncat, batch = 17_409, 3, 10_000_000, 1_025
    sample = np.arange(n) // hots
    indices = torch.zeros(n, dtype=torch.int64, device="cuda")
    offsets = torch.zeros(batch + 1, dtype=torch.int32, device="cuda")
    work_t, check_t = G.guarded_bytes(ce.transpose_workspace_bytes(n, torch.int64, None), fill="ones")
    work_b, check_b = G.guarded_bytes(query(L.cuembed_bag_order_by_length, None, 0, batch, 255, None, "work", "lwork", None),
                                      fill="ones")

    def fresh():
        cols = rng.integers(0, ncat, n)
        off, lens = bag_offsets(rng, batch, (0, 3, 7, 300), np.int32)
        indices.copy_(torch.from_numpy(cols))
        offsets.copy_(torch.from_numpy(off))
        return cols, lens

    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    fresh()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            got = ce.transpose_fixed_hotness(indices, n // hots, hots, None, workspace=work_t, num_categories=ncat,
                                             remapped=True)
            order = ce.bag_order_by_length(offsets, max_length=255, workspace=work_b)
    for fill in ("ones", "random", "zeros"):
        cols, lens = fresh()
        G.fill_bytes(work_t, fill, seed=1)
        G.fill_bytes(work_b, fill, seed=2)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        check_t("graph replay, fill %s: transpose workspace" % fill)
        check_b("graph replay, fill %s: bag-order workspace" % fill)
        want = np.argsort(cols, kind="stable")
        assert np.array_equal(got[0].cpu().numpy(), cols[want]) and np.array_equal(got[1].cpu().numpy(), sample[want])
        assert np.array_equal(got[3].cpu().numpy(), run_heads(cols[want]))
        assert np.array_equal(order.cpu().numpy(), bag_order_reference(lens, 255))
        assert np.array_equal(indices.cpu().numpy(), cols)
    clean_exit()


# ---- the knobs that move the limits between the sort's implementations -------------------------------------------------
def knob_child():
    """Runs in a process of its own with the knobs set (the chained limit changes the plan's size: the query happens
    here too): the sort with and without the remap, and the remap alone, on both sides of the moved limits."""
    L = lib()
    rng = np.random.default_rng(10)
    for index in ("i32", "i64"):
        for n in (900, 1001, 19_999, 20_001, 70_000):
            for name, cols, index_bits in key_sets(rng, n, index):
                order = np.argsort(cols, kind="stable")
                rows = rng.integers(0, n, n).astype(NP[index])
                w = weights_of(rng, n, "f32")
                for wkind, weights in (("none", None), ("f32", w)):
                    inputs = dict(rows=dev(rows), cols=dev(cols), weights=dev(weights))
                    outputs = dict(t_rows=(n, TT[index]), t_cols=(n, TT[index]), remap=(n, TT[index]))
                    want = dict(t_rows=cols[order], t_cols=rows[order], remap=run_heads(cols[order]).astype(NP[index]))
                    if weights is not None:
                        outputs["t_w"] = (n, torch.float32)
                        want["t_w"] = weights[order]
                    confined("knobs: transpose_remapped %s n=%d %s w=%s" % (index, n, name, wkind), L.cuembed_transpose_remapped,
                             transpose_remapped_args(index, wkind, n, index_bits, 0, 1, True), inputs, outputs, want)
                sorted_cols = cols[order]

                def make(t):
                    return [t["indices"], n, CODE[index], t["remap"], "work", "lwork", stream()]
                confined("knobs: compressed_grad_indices %s n=%d %s" % (index, n, name),
                         L.cuembed_compute_compressed_grad_indices, make, dict(indices=dev(sorted_cols)),
                         dict(remap=(n, TT[index])), dict(remap=run_heads(sorted_cols).astype(NP[index])))
    clean_exit()
    print("confined with knobs ok")


def test_confinement_with_the_regime_knobs_moved():
    import subprocess
    tests = os.path.dirname(os.path.abspath(__file__))
    script = ("import sys; sys.path[:0] = [%r, %r]; import test_gpu_scratch_confinement as T; T.knob_child()"
              % (os.path.dirname(tests), tests))
    env = dict(os.environ, CUEMBED_BLOCK_SORT_MAX="1000", CUEMBED_CHAINED_SORT_MAX="20000",
               CUEMBED_SORT_HIGH_WORD_LAUNCHES="1")
    r = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "confined with knobs ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
