"""The kernel instantiations that the alignment of the caller's base pointers selects, launched from 4-, 8- and 12-byte
shifted views (torch's allocator hands out 512-byte aligned blocks, so everything else in the suite runs the 16-byte
lanes).  Every comparison is bit for bit -- against the CPU oracle, an exact integer result, the recipe, or the aligned
run of the same inputs -- except the split forward (its existing fp64 bound) and the quantized pooled forward (also
inside pooled64's bound).  Every buffer that is written through a shifted view sits between sentinel bytes that must
survive the call.

Lane width per dispatcher (r = residue mod 16 of the shifted base pointer(s); every other pointer is 16-byte aligned):

  SplitRow (embedding_lookup.hpp:144-163: forward, weight gradient, both backwards) and UpdateLaneBytes
  (sparse_update.hpp:57-74: SGD, Adagrad, row-wise Adagrad, Adam, row-wise Adam) -- the widest of 16 / 8 / 4 bytes that
  divides the row size AND every data pointer:

      type    W                            row bytes     r = 0    r = 8    r = 4, 12     lanes at 16 / 8 / 4 bytes
      f32     4                            16            16       8        4             1 / 2 / 4
      f32     8, 64, 256, 1024             % 16 == 0     16       8        4             W / 4, W / 2, W   (1024: 1,024 lanes)
      f32     36, 1000, 2056               % 16 == 0     16       8        4             9 / 18 / 36, 250 / 500 / 1000, 514 / .. / 2056
      f32     50                           200           8        8        4             - / 25 / 50
      16-bit  8, 64, 256, 512, 2048        % 16 == 0     16       8        4             W / 8, W / 4, W / 2   (512: 256 lanes, 2048: 1,024)
      16-bit  36                           72            8        8        4             - / 9 / 18
      16-bit  1000, 2056                   % 16 == 0     16       8        4             125 / 250 / 500, 257 / 514 / 1028
      16-bit  50                           100           4        4        4             - / - / 25

  Adagrad's accumulator (per-element fp32 state) narrows the lane on top: N elements per lane move 4 * min(N, 4) bytes of
  state, so under an fp32 table a state at r = 8 gives 8-byte lanes, r = 4 / 12 4-byte lanes; under a 16-bit table a state
  at r = 8 gives 4-byte lanes (two elements, 8 bytes of state) and r = 4 / 12 is refused.

  QuantizedCodesPerLane (quantized_lookup.hpp:34-44: quantizer, dequantizer / concat, pooled forward) looks at the fused
  table's base alone:

      W                   table % 8 == 0                                   table % 8 == 4 (r = 4, 12)
      8                   8 codes (forward: 8)                             4
      64, 256, 4096       8 codes (forward: 16 -- W % 16 == 0, W / 16 <= 256)   4      (4096: 1,024 lanes)
      8192                8 codes, 1,024 lanes                             4: 2,048 lanes -- refused (the quantizer loops: accepted)
"""
import numpy as np
import pytest
import torch

import exact_sums as X
import quantized_reference as R

pytestmark = pytest.mark.gpu

TORCH = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
KINDS = ("f32", "f16", "bf16")
SHIFTS = (4, 8, 12)
SENTINEL = 0xA5
_CACHE = {}


@pytest.fixture(scope="module")
def ce():
    import cuembed_amd
    assert torch.cuda.is_available()
    return cuembed_amd


# ---- helpers ---------------------------------------------------------------------------------------------------------
def shifted(t, nbytes):
    """A contiguous view of t's shape and content whose data pointer is `nbytes` past a 16-byte boundary, inside a flat
    buffer of t.numel() + 32 elements (+ 16 bytes of room for the shift itself) whose every other byte is a sentinel: at
    least 16 elements on either side.  Returns (view, check); check() asserts that the sentinels are intact."""
    size = t.element_size()
    flat = torch.empty((t.numel() + 32 + 16 // size,), dtype=t.dtype, device="cuda")
    raw = flat.view(torch.uint8)
    raw.fill_(SENTINEL)
    first = 16 + ((nbytes - flat.data_ptr()) % 16) // size
    view = flat[first:first + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == nbytes and view.is_contiguous()
    lo, hi = first * size, (first + t.numel()) * size
    assert lo >= 16 * size and raw.numel() - hi >= 16 * size

    def check():
        assert bool((raw[:lo] == SENTINEL).all()) and bool((raw[hi:] == SENTINEL).all()), "a store left the view"
    return view, check


def lane_bytes(size, width, *pointers):
    """SplitRow's / UpdateLaneBytes' rule (the header's table), for asserting which instantiation a call reaches."""
    bits = size * width
    for p in pointers:
        bits |= p
    return 16 if bits % 16 == 0 else (8 if bits % 8 == 0 else 4)


def to_kind(oracle, kind, a):
    """Values -> (the oracle's array of `kind`, the same elements on the device, their exact fp64 values)."""
    a32 = np.ascontiguousarray(a, dtype=np.float32)
    if kind == "f32":
        return a32, torch.from_numpy(a32).cuda(), a32.astype(np.float64)
    if kind == "f16":
        h = a32.astype(np.float16)
        return h, torch.from_numpy(h).cuda(), h.astype(np.float64)
    b = oracle.to_bf16_bits(a32)
    return b, torch.from_numpy(b.view(np.int16)).cuda().view(torch.bfloat16), oracle.from_bf16_bits(b).astype(np.float64)


def ibits(t):
    """A tensor's elements as integers of their size (on the device)."""
    t = t.contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def dev_bits(a):
    """A numpy array's elements as integers of their size, on the device."""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view({1: np.uint8, 2: np.int16, 4: np.int32}[a.dtype.itemsize])).cuda()


def host64(oracle, kind, t):
    if kind == "bf16":
        return oracle.from_bf16_bits(t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)).astype(np.float64)
    return t.cpu().numpy().astype(np.float64)


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ragged_offsets(rng, batch, longest):
    """Bag lengths in [0, 14] with empty bags (first, last, two inside), one of one lookup and one of `longest`."""
    lens = rng.integers(0, 15, batch)
    lens[[0, 13, 14, batch - 1]] = 0
    lens[5] = longest
    lens[6] = 1
    return lens, np.concatenate([[0], np.cumsum(lens)])


# ---- forward ---------------------------------------------------------------------------------------------------------
FORWARD_KINDS = [("f32", False), ("f16", False), ("bf16", False), ("f16", True)]
FORWARD_IDS = ["f32", "f16", "bf16", "f16-fp16math"]
FORWARD_WIDTHS = {4: (4, 64, 256, 1024), 2: (8, 64, 256, 512, 2048)}    # by element size; the last: 1,024 lanes of 4 bytes
B, NCAT = 40, 300


def _forward_problem(oracle, kind, fp16_math, W):
    """The table and every layout of one (type, width), with the oracle's bits -- computed once, shared by all shifts."""
    key = ("forward", kind, fp16_math, W)
    if key in _CACHE:
        return _CACHE[key]
    rng = np.random.default_rng(7000 + W)
    table_o, table_d, _ = to_kind(oracle, kind, rng.uniform(-1, 1, (NCAT, W)))
    cases = []

    def add(name, idx, off, w, batch, hot, mode):
        it = np.int32 if len(cases) % 2 == 0 else np.int64            # int32 and int64 indices (and offsets) alternate
        idx = idx.astype(it)
        off = None if off is None else off.astype(it)
        w_o, w_d = (None, None) if w is None else to_kind(oracle, kind, w)[:2]
        want = oracle.embedding_forward(table_o, idx, off, w_o, batch_size=batch, num_hots=hot, mode=mode,
                                        fp16_math=fp16_math)
        shape = (batch, hot, W) if mode == "concat" else (batch, W)
        cases.append(dict(name=name, idx=dev(idx), off=dev(off), w=w_d, batch=batch, hot=hot, mode=mode, shape=shape,
                          want=dev_bits(want).view(-1)))

    for hot in (1, 7, 40):                                             # fixed hotness: staged in LDS
        add("fixed sum H=%d" % hot, rng.integers(0, NCAT, B * hot), None, None, B, hot, "sum")
    lens, off = ragged_offsets(rng, B, 40)
    nnz = int(off[-1])
    csr_idx = rng.integers(0, NCAT, nnz)
    add("csr sum", csr_idx, off, None, B, 0, "sum")
    add("csr mean", csr_idx, off, None, B, 0, "mean")
    add("csr weighted sum", csr_idx, off, rng.uniform(-1, 1, nnz), B, 0, "sum")
    add("csr weighted mean", csr_idx, off, rng.uniform(0.25, 1.25, nnz), B, 0, "mean")
    fixed_idx = rng.integers(0, NCAT, B * 7)
    add("fixed weighted sum", fixed_idx, None, rng.uniform(-1, 1, B * 7), B, 7, "sum")
    add("fixed weighted mean", fixed_idx, None, rng.uniform(0.25, 1.25, B * 7), B, 7, "mean")
    add("fixed mean", fixed_idx, None, None, B, 7, "mean")
    add("concat", fixed_idx, None, None, B, 7, "concat")
    if W * table_d.element_size() <= 1024:                             # the small batch the wide-load kernel takes
        add("small batch B=64 H=64", rng.integers(0, NCAT, 64 * 64), None, None, 64, 64, "sum")
    _CACHE[key] = (table_d, cases)
    return _CACHE[key]


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("kind,fp16_math", FORWARD_KINDS, ids=FORWARD_IDS)
def test_forward_from_shifted_views_matches_the_oracle(ce, oracle, kind, fp16_math, shift):
    """Table shifted, out= shifted, both: fixed hotness (LDS-staged), CSR with ragged and empty bags (wavefront-shuffle
    index source where the lanes of a row divide 64, global otherwise), weighted sum / mean, concat; with the wide-load
    kernel as the launcher decides and forbidden (so that the sequential kernel's narrow instantiations run too)."""
    size = TORCH[kind].itemsize
    try:
        for W in FORWARD_WIDTHS[size]:
            table_d, cases = _forward_problem(oracle, kind, fp16_math, W)
            assert lane_bytes(size, W, table_d.data_ptr()) == 16          # the aligned run: 16-byte lanes
            ce.set_forward_wide_load("auto")
            if W * size <= 1024:
                assert ce.forward_launch_shape(TORCH[kind], torch.int32, W, 64, 64)["wide_load"]
            for which in ("table", "out", "both"):
                table_v, table_ok = shifted(table_d, shift if which != "out" else 0)
                for wide in ("auto", "never"):
                    ce.set_forward_wide_load(wide)
                    for c in cases:
                        out_v, out_ok = shifted(torch.full(c["shape"], -77.0, dtype=TORCH[kind], device="cuda"),
                                                shift if which != "table" else 0)
                        assert (table_v.data_ptr() | out_v.data_ptr()) % 16 == shift
                        lane = lane_bytes(size, W, table_v.data_ptr(), out_v.data_ptr())
                        assert lane == (8 if shift == 8 else 4) and W * size // lane <= 1024
                        got = ce.embedding_forward(table_v, c["idx"], c["off"], c["w"], batch_size=c["batch"],
                                                   num_hots=c["hot"], mode=c["mode"], fp16_math=fp16_math, out=out_v)
                        assert got.data_ptr() == out_v.data_ptr()
                        assert torch.equal(ibits(out_v).view(-1), c["want"]), (W, which, wide, c["name"])
                        out_ok()
                table_ok()
    finally:
        ce.set_forward_wide_load("auto")


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("kind,fp16_math", FORWARD_KINDS, ids=FORWARD_IDS)
def test_split_forward_from_shifted_views_within_its_bound(ce, oracle, kind, fp16_math, shift):
    """reduction_order="split" is not bit-exact: the per-element fp64 bound of test_split_forward_per_element_bound
    (exact_sums.assert_split_forward_within_bound), on its shapes, with the narrower lanes of a shifted table and out."""
    size = TORCH[kind].itemsize
    ncat, batch, hot = 2_000, 37, 61
    for W in (8, 64, 256):
        key = ("split", kind, fp16_math, W)
        if key not in _CACHE:
            rng = np.random.default_rng(60 + W)
            t_o, t_d, t64 = to_kind(oracle, kind, rng.uniform(-1, 1, (ncat, W)))
            lens = rng.integers(0, 2 * hot, batch)
            lens[3] = 0
            off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
            w_o, w_d, w64 = to_kind(oracle, kind, rng.uniform(0, 1, int(off[-1])))
            idx_csr = rng.integers(0, ncat, int(off[-1])).astype(np.int64)
            idx = rng.integers(0, ncat, batch * hot).astype(np.int32)
            fixed_off = np.arange(0, batch * hot + 1, hot)
            layouts = []
            for mode, ids, o, csr, weighted in (("sum", idx, fixed_off, False, False), ("mean", idx_csr, off, True, True)):
                exact, scale, h = X.forward(t64, ids, o, w64 if weighted else None, mean=mode == "mean")
                want = oracle.embedding_forward(t_o, ids, o if csr else None, w_o if weighted else None,
                                                num_hots=0 if csr else hot, mode=mode, fp16_math=fp16_math)
                ora = oracle.from_bf16_bits(want).astype(np.float64) if kind == "bf16" else want.astype(np.float64)
                layouts.append((mode, dev(ids), dev(o) if csr else None, w_d if weighted else None, 0 if csr else hot,
                                exact, scale, h, ora))
            _CACHE[key] = (t_d, layouts)
        t_d, layouts = _CACHE[key]
        for which in ("table", "both"):
            table_v, table_ok = shifted(t_d, shift)
            for mode, ids_d, off_d, w_d, hots, exact, scale, h, ora in layouts:
                out_v, out_ok = shifted(torch.full((batch, W), -77.0, dtype=TORCH[kind], device="cuda"),
                                        shift if which == "both" else 0)
                assert table_v.data_ptr() % 16 == shift and lane_bytes(size, W, table_v.data_ptr()) < 16
                ce.embedding_forward(table_v, ids_d, off_d, w_d, num_hots=hots, mode=mode, fp16_math=fp16_math, out=out_v,
                                     reduction_order="split")
                X.assert_split_forward_within_bound(kind, fp16_math, host64(oracle, kind, out_v), exact, scale, h, ora,
                                                    mode == "mean", (W, which, mode))
                out_ok()
            table_ok()
    assert ce.get_forward_reduction_order() == "sequential"


# ---- weight gradient -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("kind", KINDS)
def test_weight_gradient_from_shifted_views_is_the_exact_dot_product(ce, oracle, kind, shift):
    """Integer data with |dot| <= 256: every product and partial sum is exact in fp32 in any order and the result is
    representable in fp16 and bf16, so the device's bits are those of the numpy dot product."""
    size = TORCH[kind].itemsize
    batch, hot, ncat = 45, 5, 200
    for W, top in ((64, 2), (256, 1)):                       # values in {-2 .. 2} / {-1, 0, 1}
        rng = np.random.default_rng(300 + W)
        _, table_d, t64 = to_kind(oracle, kind, rng.integers(-top, top + 1, (ncat, W)))
        _, gy_d, g64 = to_kind(oracle, kind, rng.integers(-top, top + 1, (batch, W)))
        assert np.abs(t64).max() * np.abs(g64).max() * W <= 256
        lens, off = ragged_offsets(rng, batch, 20)
        layouts = [(rng.integers(0, ncat, batch * hot).astype(np.int32), None, np.repeat(np.arange(batch), hot)),
                   (rng.integers(0, ncat, int(off[-1])).astype(np.int64), off.astype(np.int64), np.repeat(np.arange(batch), lens))]
        for idx, o, sample in layouts:
            exact = (t64[idx] * g64[sample]).sum(axis=1)
            assert np.abs(exact).max() <= 256 and np.abs(exact).max() >= 8          # (not a vacuous comparison)
            want = dev_bits(to_kind(oracle, kind, exact)[0])
            for which in ("params", "grad_y", "both"):
                p_v, p_ok = shifted(table_d, shift if which != "grad_y" else 0)
                g_v, g_ok = shifted(gy_d, shift if which != "params" else 0)
                assert (p_v.data_ptr() | g_v.data_ptr()) % 16 == shift
                assert lane_bytes(size, W, p_v.data_ptr(), g_v.data_ptr()) == (8 if shift == 8 else 4)
                got = ce.embedding_weight_grad(p_v, dev(idx), g_v, offsets=dev(o), num_hots=0 if o is not None else hot)
                assert torch.equal(ibits(got), want), (W, which, o is not None)
                p_ok()
                g_ok()


# ---- backward --------------------------------------------------------------------------------------------------------
#: the integers a type holds exactly: |row sum| and every partial sum must stay within them
EXACT_INTEGERS = {"f32": 2 ** 24, "f16": 2048, "bf16": 256}
#: run length of the hot row; with |gradient| <= 3 and weights <= 2 a row sum is at most 6 * run: 1,500 lookups for
#: fp32, 300 for fp16 (1,800 <= 2,048), 40 for bf16 (240 <= 256)
HOT_RUN = {"f32": 1500, "f16": 300, "bf16": 40}
BWD_BATCH, BWD_HOT, BWD_NCAT, TAIL = 700, 8, 700, 37


def _backward_problem(oracle, kind, W):
    key = ("backward", kind, W)
    if key in _CACHE:
        return _CACHE[key]
    rng = np.random.default_rng(900 + W)
    it = np.int32 if W in (8, 64) else np.int64
    nnz = BWD_BATCH * BWD_HOT
    idx = rng.integers(0, BWD_NCAT - 1, nnz)
    idx[idx >= 7] += 1                                                   # row 7 is the hot row, and only that
    idx[rng.choice(nnz, HOT_RUN[kind], replace=False)] = 7
    idx = idx.astype(it)
    longest = int(np.bincount(idx).max())
    assert longest == HOT_RUN[kind] and 6 * longest <= EXACT_INTEGERS[kind]       # the run-length bound, on the data
    w_o = to_kind(oracle, kind, rng.integers(1, 3, nnz))[0]
    gy_o, gy_d, _ = to_kind(oracle, kind, rng.integers(-3, 4, (BWD_BATCH, W)))
    sid = oracle.extract_row_ids_from_fixed(BWD_BATCH, BWD_HOT, dtype=it)
    t_idx, t_sid, t_w = oracle.transpose(sid, idx, w_o)
    remap = oracle.compute_compressed_grad_indices(t_idx)
    nu = int(remap[-1]) + 1
    p = dict(W=W, nu=nu, gy=gy_d, t_idx=dev(t_idx), t_sid=dev(t_sid), remap=dev(remap),
             rows_of_batch=dev(np.unique(idx)))
    p["t_w"] = torch.from_numpy(t_w.view(np.int16)).cuda().view(torch.bfloat16) if kind == "bf16" else dev(t_w)
    full, _ = oracle.embedding_backward(gy_o, W, BWD_NCAT, t_idx, t_sid, None, t_w)
    comp, inv = oracle.embedding_backward(gy_o, W, nu + TAIL, t_idx, t_sid, remap, t_w)
    assert not comp[nu:].any() and np.abs(full.astype(np.float64) if kind != "bf16" else
                                          oracle.from_bf16_bits(full)).max() > 8
    p.update(full=dev_bits(full), comp=dev_bits(comp), inv=dev(inv[:nu]))
    # reference sums: arbitrary data, the reference's own rounding chain
    a_gy_o, a_gy_d, _ = to_kind(oracle, kind, rng.uniform(-1, 1, (BWD_BATCH, W)))
    a_w_o = to_kind(oracle, kind, rng.uniform(0.25, 1.25, nnz))[0]
    _, _, a_tw = oracle.transpose(sid, idx, a_w_o)
    r_full, _ = oracle.embedding_backward(a_gy_o, W, BWD_NCAT, t_idx, t_sid, None, a_tw)
    r_comp, _ = oracle.embedding_backward(a_gy_o, W, nu, t_idx, t_sid, remap, a_tw)
    fill_o, fill_d, _ = to_kind(oracle, kind, rng.uniform(-1, 1, (BWD_NCAT, W)))
    r_added, _ = oracle.embedding_backward(a_gy_o, W, BWD_NCAT, t_idx, t_sid, None, a_tw, skip_grad_init=True,
                                           grad_embedding=fill_o.copy())
    p.update(a_gy=a_gy_d, r_full=dev_bits(r_full), r_comp=dev_bits(r_comp), fill=fill_d, r_added=dev_bits(r_added),
             a_tw=torch.from_numpy(a_tw.view(np.int16)).cuda().view(torch.bfloat16) if kind == "bf16" else dev(a_tw))
    _CACHE[key] = p
    return p


def _backward_cases(ce, kind, p, shift, which, cases):
    """Runs the named backward cases with grad_y and / or grad_embedding= shifted; every result against the oracle's
    bits, every written buffer's sentinels checked."""
    W, nu, dtype = p["W"], p["nu"], TORCH[kind]
    size = dtype.itemsize
    gy_shift = shift if which != "out" else 0
    out_shift = shift if which != "gy" else 0
    gy_v, gy_ok = shifted(p["gy"], gy_shift)
    a_gy_v, a_gy_ok = shifted(p["a_gy"], gy_shift)

    def out(rows, fill=None):
        t = torch.full((rows, W), -77.0, dtype=dtype, device="cuda") if fill is None else fill
        v, ok = shifted(t, out_shift)
        assert (gy_v.data_ptr() | v.data_ptr()) % 16 == shift
        want_lane = 4 if shift != 8 else min(8, lane_bytes(size, W))
        assert lane_bytes(size, W, gy_v.data_ptr(), v.data_ptr()) == want_lane
        return v, ok

    def same(got, want, label):
        assert torch.equal(ibits(got).view(-1), want.view(-1)), (kind, W, shift, which, label)

    index_dtype = p["t_idx"].dtype
    for case in cases:
        if case == "full":
            ge, ok = out(BWD_NCAT)
            ce.embedding_backward(gy_v, BWD_NCAT, p["t_idx"], p["t_sid"], None, p["t_w"], grad_embedding=ge)
            same(ge, p["full"], case)
        elif case == "compressed, over-allocated tail":           # host-known count: the zeroing kernel's ragged ends
            ge, ok = out(nu + TAIL)
            inv = torch.full((nu + TAIL,), -1, dtype=index_dtype, device="cuda")
            ce.embedding_backward(gy_v, nu + TAIL, p["t_idx"], p["t_sid"], p["remap"], p["t_w"], grad_embedding=ge,
                                  inverse_mapping=inv)
            same(ge, p["comp"], case)
            assert not ibits(ge[nu:]).any() and torch.equal(inv[:nu], p["inv"])
        elif case == "compressed, device-side count, padded":
            ge, ok = out(nu + TAIL)
            inv = torch.full((nu + TAIL,), -1, dtype=index_dtype, device="cuda")
            ce.embedding_backward(gy_v, None, p["t_idx"], p["t_sid"], p["remap"], p["t_w"], grad_embedding=ge,
                                  inverse_mapping=inv, pad_to_capacity=True)
            same(ge, p["comp"], case)
            assert not ibits(ge[nu:]).any() and torch.equal(inv[:nu], p["inv"])
            assert bool(torch.isin(inv[nu:], p["rows_of_batch"]).all())      # the tail names rows of the batch
            assert not ce.capacity_overflowed()
        elif case == "skip_grad_init":                            # no memset: a buffer the caller zeroed (the contract)
            ge, ok = out(BWD_NCAT, torch.zeros((BWD_NCAT, W), dtype=dtype, device="cuda"))
            ce.embedding_backward(gy_v, BWD_NCAT, p["t_idx"], p["t_sid"], None, p["t_w"], skip_grad_init=True,
                                  grad_embedding=ge)
            same(ge, p["full"], case)
        elif case == "reference sums, skip_grad_init":            # ... which ADD to a buffer the caller pre-filled
            ge, ok = out(BWD_NCAT, p["fill"])
            ce.embedding_backward(a_gy_v, BWD_NCAT, p["t_idx"], p["t_sid"], None, p["a_tw"], skip_grad_init=True,
                                  grad_embedding=ge, reference_sums=True)
            same(ge, p["r_added"], case)
        elif case == "reference sums, full":
            ge, ok = out(BWD_NCAT)
            ce.embedding_backward(a_gy_v, BWD_NCAT, p["t_idx"], p["t_sid"], None, p["a_tw"], grad_embedding=ge,
                                  reference_sums=True)
            same(ge, p["r_full"], case)
        elif case == "reference sums, compressed":
            ge, ok = out(nu)
            _, inv = ce.embedding_backward(a_gy_v, nu, p["t_idx"], p["t_sid"], p["remap"], p["a_tw"], grad_embedding=ge,
                                           reference_sums=True)
            same(ge, p["r_comp"], case)
            assert torch.equal(inv, p["inv"])
        else:
            raise AssertionError(case)
        ok()
    gy_ok()
    a_gy_ok()


BACKWARD_CASES = ("full", "compressed, over-allocated tail", "compressed, device-side count, padded", "skip_grad_init",
                  "reference sums, full", "reference sums, compressed", "reference sums, skip_grad_init")


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("kind", KINDS)
def test_backward_from_shifted_views_matches_the_oracle(ce, oracle, kind, shift):
    """700 samples x 8 lookups of 700 rows, one hot row whose run crosses workgroups: its pieces arrive through atomics
    in any order, which is why the data is integer-valued and the run length bounded (HOT_RUN) -- the sums are exact
    and the result is the oracle's, bit for bit.  reference_sums=True is bit-identical on arbitrary data by design, and
    the arithmetic in which skip_grad_init=True adds to a buffer the caller pre-filled (EmbeddingBackward's own contract
    is a zeroed buffer: a run inside one workgroup is stored, not added)."""
    assert ce.get_backward_tuning() == dict(segment_len=0, column_slices=0)
    for W in (8, 36, 64, 256):
        p = _backward_problem(oracle, kind, W)
        for which in ("gy", "out", "both"):
            _backward_cases(ce, kind, p, shift, which, BACKWARD_CASES)
    try:                                                          # forced launch shapes: results never depend on them
        for tuning, W in ((dict(segment_len=8), 64), (dict(column_slices=2), 256)):
            ce.set_backward_tuning(**tuning)
            _backward_cases(ce, kind, _backward_problem(oracle, kind, W), shift, "both", BACKWARD_CASES[:4])
    finally:
        ce.set_backward_tuning(0, 0)


# ---- sparse optimizer step -------------------------------------------------------------------------------------------
RULES = ("sgd", "adagrad", "rowwise_adagrad", "adam", "rowwise_adam")
#: one slice per lane group, an odd split, one slice per lane, four with a partial last, the run-time loop
UPDATE_WIDTHS = (8, 50, 256, 1000, 2056)


def _step(ce, rule, table, ids, rows, state):
    if rule in ("adam", "rowwise_adam"):
        ce.sparse_row_adam(table, ids, rows, exp_avg=state[0], exp_avg_sq=state[1], lr=0.01, bias_factor=0.7,
                           weight_decay=0.01, rowwise=rule == "rowwise_adam")
    else:
        ce.sparse_row_update(table, ids, rows, rule=rule, lr=0.05, state=state[0] if state else None)


def _new_state(rule, ncat, width):
    if rule == "sgd":
        return ()
    if rule == "adagrad":
        return (torch.rand((ncat, width), device="cuda") * 0.5 + 0.1,)
    if rule == "rowwise_adagrad":
        return (torch.rand((ncat,), device="cuda") * 0.5 + 0.1,)
    v_shape = (ncat, width) if rule == "adam" else (ncat,)
    return (torch.randn((ncat, width), device="cuda") * 0.1, torch.rand(v_shape, device="cuda") * 0.5 + 0.01)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("rule", RULES)
def test_optimizer_step_from_shifted_views_equals_the_aligned_step(ce, rule, kind):
    """Table, gradient rows and (Adagrad) the accumulator shifted alone and together: bit-identical to the aligned step
    of the same inputs -- the per-element rules do not depend on the lane mapping, and gradients of +-2^-3 .. 2^-5 keep
    a row's sum of squares exact in any order.  Rows that no id names keep their bits.  (The aligned step against fp64
    is test_gpu_sparse_update.py's and test_gpu_sparse_adam.py's business.)"""
    dtype = TORCH[kind]
    size = dtype.itemsize
    for W in UPDATE_WIDTHS:
        ncat, n = (2000, 300) if W <= 1000 else (400, 60)
        table = (torch.rand((ncat, W), device="cuda") * 2 - 1).to(dtype)
        ids = torch.randperm(ncat, device="cuda")[:n].to(torch.int32 if W in (8, 256, 2056) else torch.int64)
        mag = torch.tensor([2.0 ** -3, 2.0 ** -4, 2.0 ** -5], device="cuda")[torch.randint(0, 3, (n, W), device="cuda")]
        rows = (mag * (torch.randint(0, 2, (n, W), device="cuda") * 2 - 1)).to(dtype)
        state = _new_state(rule, ncat, W)
        unnamed = torch.ones(ncat, dtype=torch.bool, device="cuda")
        unnamed[ids.long()] = False
        want_table, want_state = table.clone(), tuple(s.clone() for s in state)
        _step(ce, rule, want_table, ids, rows, want_state)
        assert not torch.equal(ibits(want_table[~unnamed]), ibits(table[~unnamed]))          # the step moved the named rows
        assert torch.equal(ibits(want_table[unnamed]), ibits(table[unnamed]))
        parts = ("table", "rows") + (("state",) if rule in ("adagrad", "rowwise_adagrad") else ())
        for shift in SHIFTS:
            # a 16-bit table's narrowest lane moves 8 bytes of Adagrad's accumulator: its shift is 8 (4 and 12 are refused)
            state_shift = 8 if (rule == "adagrad" and size == 2) else shift
            for which in [(part,) for part in parts] + [parts]:
                t_v, t_ok = shifted(table, shift if "table" in which else 0)
                r_v, r_ok = shifted(rows, shift if "rows" in which else 0)
                checks = [t_ok, r_ok]
                s_v = []
                for k, s in enumerate(state):
                    v, ok = shifted(s, state_shift if ("state" in which and k == 0 and rule.endswith("adagrad")) else 0)
                    s_v.append(v)
                    checks.append(ok)
                # the residues this case relies on (row-wise Adagrad's one word per row takes no part in the lane width)
                expect = (shift if ("table" in which or "rows" in which) else 0) | \
                         (state_shift if ("state" in which and rule == "adagrad") else 0)
                residues = t_v.data_ptr() | r_v.data_ptr() | (s_v[0].data_ptr() if rule == "adagrad" else 0)
                assert residues % 16 == expect
                lane = lane_bytes(size, W, t_v.data_ptr(), r_v.data_ptr())
                if rule == "adagrad" and s_v[0].data_ptr() % 16:     # the state narrows the lane on top (UpdateLaneBytes)
                    lane = min(lane, 4 if size == 2 else lane_bytes(4, 4, s_v[0].data_ptr()))
                assert lane <= lane_bytes(size, W) and (lane < 16 or expect == 0)
                _step(ce, rule, t_v, ids, r_v, tuple(s_v))
                label = (W, shift, which)
                assert torch.equal(ibits(t_v), ibits(want_table)), label
                for got, want in zip(s_v, want_state):
                    assert torch.equal(ibits(got), ibits(want)), label
                assert torch.equal(ibits(t_v[unnamed]), ibits(table[unnamed])), label
                assert torch.equal(ibits(r_v), ibits(rows)), label
                for ok in checks:
                    ok()
        if rule == "adagrad" and size == 2 and W == 8:
            for bad in (4, 12):                                    # the next-narrower residue is refused, not run
                s_bad, _ = shifted(state[0], bad)
                t_try = table.clone()
                with pytest.raises(ValueError, match="aligned"):
                    _step(ce, rule, t_try, ids, rows, (s_bad,))
                assert torch.equal(ibits(t_try), ibits(table))


# ---- quantized tables from a 4-byte aligned base -----------------------------------------------------------------------
Q_ROWS, Q_BATCH, Q_HOT = 400, 41, 7


def _quantized_problem(width, out):
    key = ("quantized", width, out)
    if key in _CACHE:
        return _CACHE[key]
    rng = np.random.default_rng(5000 + width)
    parts = [R.make_table("normal", Q_ROWS // 4, width, seed=width), R.make_table("uniform", Q_ROWS // 4, width, seed=width + 17),
             R.make_table("offset", Q_ROWS // 4, width, seed=width + 34) - np.float32(1e4 - 30.0),
             R.make_table("constant", Q_ROWS // 4, width, seed=width + 51)]
    x = np.ascontiguousarray(np.stack(parts, axis=1).reshape(-1, width))
    q_np = R.quantize(x)
    lens = rng.integers(0, 2 * Q_HOT + 1, Q_BATCH)
    lens[[0, Q_BATCH // 3, Q_BATCH - 1]] = 0
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    cases = []
    np_out = {"f32": np.float32, "f16": np.float16}[out]
    for csr in (False, True):
        nnz = int(off[-1]) if csr else Q_BATCH * Q_HOT
        idx = rng.integers(0, Q_ROWS, nnz)
        for mode in ("sum", "mean"):
            for weighted in (False, True):
                w = None
                if weighted:
                    w = (rng.uniform(-1, 1, nnz) if mode == "sum" else rng.uniform(0.25, 1.25, nnz)).astype(np_out)
                exact, bound = R.pooled64(q_np, idx, offsets=off if csr else None, num_hots=0 if csr else Q_HOT, weights=w,
                                          mode=mode, out=out)
                cases.append(dict(csr=csr, mode=mode, idx=idx, off=off if csr else None, w=w, exact=exact, bound=bound,
                                  empty=(np.diff(off) == 0) if csr else None))
    _CACHE[key] = (x, q_np, cases)
    return _CACHE[key]


@pytest.mark.parametrize("shift", (4, 12))
@pytest.mark.parametrize("width", (8, 64, 256, 4096))
def test_quantized_table_from_a_4_byte_aligned_base(ce, width, shift):
    """data_ptr() % 8 == 4: every quantized kernel runs its N = 4 instantiation (aligned: 8 codes per lane, 16 in the
    forward of W = 64 / 256 / 4096).  The quantizer's bytes are the recipe's, the dequantizer's and concat's bits
    dequant32's; sum and mean are bit-identical to the same call on the aligned copy -- every element is the same
    sequence of fp32 operations at any N -- and inside pooled64's bound."""
    x, q_np, _ = _quantized_problem(width, "f32")
    x_d = torch.from_numpy(x).cuda()
    aligned = ce.quantize_rows(x_d)
    assert aligned.data_ptr() % 16 == 0 and np.array_equal(aligned.cpu().numpy(), q_np)
    # quantizer into a shifted buffer
    q_v, q_ok = shifted(torch.zeros((Q_ROWS, width + 8), dtype=torch.uint8, device="cuda"), shift)
    assert q_v.data_ptr() % 8 == 4
    got = ce.quantize_rows(x_d, out=q_v)
    assert got.data_ptr() == q_v.data_ptr() and torch.equal(q_v, aligned)
    q_ok()
    # ... and a copy of the aligned table at the other residue: the same bytes, read from there
    copy_v, copy_ok = shifted(aligned, 16 - shift)
    assert copy_v.data_ptr() % 8 == 4 and copy_v.data_ptr() % 16 != q_v.data_ptr() % 16
    want32 = R.dequant32(q_np)
    want16 = want32.astype(np.float16)
    ids_np = np.random.default_rng(width).integers(0, Q_ROWS, (Q_BATCH, 5))
    for table in (q_v, copy_v):
        assert torch.equal(ibits(ce.dequantize_rows(table)), dev_bits(want32))
        assert torch.equal(ibits(ce.dequantize_rows(table, dtype=torch.float16)), dev_bits(want16))
        for idt in (torch.int32, torch.int64):
            ids = torch.from_numpy(ids_np).to("cuda", idt)
            assert torch.equal(ibits(ce.dequantize_rows(table, ids)), dev_bits(want32[ids_np]))
            c16 = ce.embedding_forward_quantized(table, ids.view(-1), num_hots=5, mode="concat")
            c32 = ce.embedding_forward_quantized(table, ids.view(-1), num_hots=5, mode="concat", out_dtype=torch.float32)
            assert torch.equal(ibits(c16), dev_bits(want16[ids_np])) and torch.equal(ibits(c32), dev_bits(want32[ids_np]))
    for out in ("f32", "f16"):
        _, _, cases = _quantized_problem(width, out)
        for n, c in enumerate(cases):
            idt = torch.int32 if n % 2 == 0 else torch.int64
            kw = dict(offsets=None if c["off"] is None else torch.from_numpy(c["off"]).to("cuda", idt),
                      weights=dev(c["w"]), num_hots=0 if c["csr"] else Q_HOT, mode=c["mode"], out_dtype=TORCH[out])
            idx = torch.from_numpy(c["idx"]).to("cuda", idt)
            twin = ce.embedding_forward_quantized(aligned, idx, **kw)
            assert R.worst_ratio(twin.float().cpu().numpy(), c["exact"], c["bound"]) <= 1.0
            for table in (q_v, copy_v):
                got = ce.embedding_forward_quantized(table, idx, **kw)
                assert torch.equal(ibits(got), ibits(twin)), (width, out, c["mode"], c["csr"], c["w"] is not None)
            if c["csr"]:
                assert c["empty"].any() and not twin[torch.from_numpy(c["empty"]).cuda()].any()
    q_ok()
    copy_ok()


def test_quantized_rows_too_wide_for_a_4_byte_aligned_base_are_refused(ce):
    """W = 8192 from a 4-byte aligned base is 2,048 lanes of 4 codes: the dequantizer, concat and the pooled forward
    raise; the quantizer's lane groups loop over a row, so it still writes the recipe's bytes there."""
    width, rows = 8192, 9
    x = R.make_table("normal", rows, width, seed=3)
    q_np = R.quantize(x)
    q_v, q_ok = shifted(torch.zeros((rows, width + 8), dtype=torch.uint8, device="cuda"), 4)
    ce.quantize_rows(torch.from_numpy(x).cuda(), out=q_v)
    assert np.array_equal(q_v.cpu().numpy(), q_np)
    q_ok()
    idx = torch.arange(rows, device="cuda")
    for call in (lambda: ce.dequantize_rows(q_v), lambda: ce.dequantize_rows(q_v, idx),
                 lambda: ce.embedding_forward_quantized(q_v, idx, num_hots=3),
                 lambda: ce.embedding_forward_quantized(q_v, idx, num_hots=3, mode="concat")):
        with pytest.raises(ValueError, match="2048 lanes"):
            call()
    aligned = torch.from_numpy(q_np).cuda()                       # the same bytes from an aligned base: 1,024 lanes of 8
    assert torch.equal(ibits(ce.dequantize_rows(aligned)), dev_bits(R.dequant32(q_np)))
    assert np.array_equal(q_v.cpu().numpy(), q_np)


# ---- rejections, wired -------------------------------------------------------------------------------------------------
def _off_by(t, elements):
    """t's content in a contiguous view `elements` elements into a zeroed buffer."""
    flat = torch.zeros((t.numel() + 16,), dtype=t.dtype, device="cuda")
    view = flat[elements:elements + t.numel()].view(t.shape)
    view.copy_(t)
    return view


def test_misaligned_and_over_wide_calls_raise_before_any_launch(ce):
    """What the native dispatchers abort on is an exception at every Python entry point and torch op: a 16-bit tensor
    viewed one element in (data_ptr() % 4 == 2) and a row too wide for the lanes its alignment allows (fp16 W = 2052 from
    a 4-byte aligned view: 1,026 lanes; the optimizer steps and the quantizer loop over a row and take any width).  The
    inputs keep their bits, and the process goes on to run an ordinary call."""
    from cuembed_amd import cuembed_pyt as P
    op_error = RuntimeError if P.BACKEND == "native" else (RuntimeError, ValueError)
    ops = torch.ops.cuembed_pyt
    half = torch.float16
    batch, hot, ncat = 6, 3, 20
    idx = torch.randint(0, ncat, (batch * hot,), device="cuda", dtype=torch.int32)
    off = torch.arange(0, batch * hot + 1, hot, device="cuda", dtype=torch.int32)
    sid = ce.extract_row_ids_from_fixed(batch, hot, torch.int32, "cuda")
    t_idx, t_sid, _ = ce.transpose(sid, idx)
    remap = ce.compute_compressed_grad_indices(t_idx)
    ids = torch.arange(5, device="cuda", dtype=torch.int32)
    for W, elements in ((8, 1), (2052, 2)):                       # one element off; over-wide from a 4-byte aligned view
        table = torch.rand((ncat, W), device="cuda").to(half)
        gy = torch.rand((batch, W), device="cuda").to(half)
        bad_table, bad_gy = _off_by(table, elements), _off_by(gy, elements)
        assert bad_table.data_ptr() % 4 == 2 * elements % 4 and bad_table.data_ptr() % 16 == 2 * elements
        assert bad_gy.data_ptr() % 16 == 2 * elements
        bad_out = _off_by(torch.zeros((batch, W), device="cuda", dtype=half), elements)
        bad_grad = _off_by(torch.zeros((ncat, W), device="cuda", dtype=half), elements)
        calls = [
            lambda: ce.embedding_forward(bad_table, idx, num_hots=hot),
            lambda: ce.embedding_forward(table, idx, num_hots=hot, out=bad_out),
            lambda: ce.embedding_forward(bad_table, idx, off, mode="mean"),
            lambda: ce.embedding_weight_grad(bad_table, idx, gy, num_hots=hot),
            lambda: ce.embedding_weight_grad(table, idx, bad_gy, num_hots=hot),
            lambda: ce.embedding_backward(bad_gy, ncat, t_idx, t_sid),
            lambda: ce.embedding_backward(gy, ncat, t_idx, t_sid, grad_embedding=bad_grad),
            lambda: ce.embedding_backward(bad_gy, ncat, t_idx, t_sid, reference_sums=True),
            lambda: ce.embedding_backward(gy, ncat, t_idx, t_sid, grad_embedding=bad_grad, reference_sums=True),
        ]
        op_calls = [
            lambda: ops.cuembed_embedding_forward(bad_table, idx, off, None, "sum"),
            lambda: ops.cuembed_embedding_forward_fixed(bad_table, idx.view(batch, hot), None, "sum"),
            lambda: ops.cuembed_embedding_weight_grad(bad_table, idx, off, gy),
            lambda: ops.cuembed_embedding_weight_grad(table, idx, off, bad_gy),
            lambda: ops.cuembed_embedding_backward(bad_gy, ncat, t_idx, t_sid, None),
            lambda: ops.cuembed_embedding_backward_compressed(bad_gy, int(remap[-1]) + 1, t_idx, t_sid, remap, None),
        ]
        if elements == 1:                                         # (the optimizer steps take any width: no lane limit)
            rows = torch.rand((5, W), device="cuda").to(half)
            bad_rows = _off_by(rows, 1)
            acc = torch.ones((ncat, W), device="cuda")
            m, v = torch.zeros((ncat, W), device="cuda"), torch.zeros((ncat, W), device="cuda")
            calls += [
                lambda: ce.sparse_row_update(bad_table, ids, rows, rule="sgd", lr=0.1),
                lambda: ce.sparse_row_update(table, ids, bad_rows, rule="adagrad", lr=0.1, state=acc),
                lambda: ce.sparse_row_update(bad_table, ids, rows, rule="rowwise_adagrad", lr=0.1, state=acc[:, 0].contiguous()),
                lambda: ce.sparse_row_adam(bad_table, ids, rows, exp_avg=m, exp_avg_sq=v, lr=0.1),
                lambda: ce.sparse_row_adam(table, ids, bad_rows, exp_avg=m, exp_avg_sq=v[:, 0].contiguous(), lr=0.1, rowwise=True),
            ]
            op_calls += [
                lambda: ops.cuembed_sparse_row_update_(bad_table, None, ids, rows, "sgd", 0.1, 1e-8, None, -1, None, None, 0),
                lambda: ops.cuembed_sparse_row_update_(table, acc, ids, bad_rows, "adagrad", 0.1, 1e-8, None, -1, None, None, 0),
                lambda: ops.cuembed_sparse_row_adam_(bad_table, m, v, ids, rows, False, 0.1, 1.0, 0.9, 0.999, 1e-8, 0.0, None,
                                                     None, -1, None, None, 0),
            ]
        before = [t.clone() for t in (bad_table, bad_gy, bad_out, bad_grad, table, gy)]
        for n, call in enumerate(calls):
            with pytest.raises(ValueError, match="aligned"):
                call()
        for n, call in enumerate(op_calls):
            with pytest.raises(op_error, match="aligned|align the data"):
                call()
        for t, was in zip((bad_table, bad_gy, bad_out, bad_grad, table, gy), before):
            assert torch.equal(ibits(t), ibits(was))
    # a 16-bit table's Adagrad accumulator 4 bytes off, through the torch op as well
    table = torch.rand((ncat, 8), device="cuda").to(half)
    rows = torch.rand((5, 8), device="cuda").to(half)
    acc_bad = _off_by(torch.ones((ncat, 8), device="cuda"), 1)
    assert acc_bad.data_ptr() % 8 == 4
    with pytest.raises(ValueError, match="8-byte aligned"):
        ce.sparse_row_update(table, ids, rows, rule="adagrad", lr=0.1, state=acc_bad)
    with pytest.raises(op_error, match="8-byte aligned"):
        ops.cuembed_sparse_row_update_(table, acc_bad, ids, rows, "adagrad", 0.1, 1e-8, None, -1, None, None, 0)
    # quantized: the fused table 2 bytes off, a quantizer output 2 bytes off, W = 8192 from a 4-byte aligned base
    x = torch.rand((ncat, 8), device="cuda")
    q = ce.quantize_rows(x)
    q_off2 = _off_by(q, 2)
    q_wide = _off_by(ce.quantize_rows(torch.rand((3, 8192), device="cuda")), 4)
    assert q_off2.data_ptr() % 4 == 2 and q_wide.data_ptr() % 8 == 4
    wide_idx = torch.zeros((2, 2), device="cuda", dtype=torch.int64)
    for call in (lambda: ce.quantize_rows(x, out=q_off2), lambda: ce.dequantize_rows(q_off2),
                 lambda: ce.embedding_forward_quantized(q_off2, idx, num_hots=hot),
                 lambda: ce.dequantize_rows(q_wide), lambda: ce.embedding_forward_quantized(q_wide, wide_idx.view(-1), num_hots=2)):
        with pytest.raises(ValueError, match="aligned"):
            call()
    for call in (lambda: ops.dequantize_rows(q_off2, None, torch.float32),
                 lambda: ops.cuemb_embedding_quantized(q_off2, idx.view(batch, hot), None, None, "sum", half, -1, None, None),
                 lambda: ops.dequantize_rows(q_wide, None, torch.float32),
                 lambda: ops.cuemb_embedding_quantized(q_wide, wide_idx, None, None, "sum", half, -1, None, None),
                 lambda: ops.quantize_rows(_off_by(x, 1))):
        with pytest.raises(op_error, match="aligned|align the table"):
            call()
    # the process is alive and an ordinary aligned call of every family still runs
    table = torch.rand((ncat, 8), device="cuda").to(half)
    out = ce.embedding_forward(table, idx, num_hots=hot)
    assert torch.equal(out, ops.cuembed_embedding_forward(table, idx, off, None, "sum"))
    assert ce.embedding_weight_grad(table, idx, out, num_hots=hot).numel() == batch * hot
    grad, _ = ce.embedding_backward(out, ncat, t_idx, t_sid)
    assert tuple(grad.shape) == (ncat, 8)
    ce.sparse_row_update(table, ids, rows, rule="sgd", lr=0.1)
    assert torch.equal(ce.dequantize_rows(q), ops.dequantize_rows(q, None, torch.float32))
    torch.cuda.synchronize()
