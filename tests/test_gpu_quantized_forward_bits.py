"""The quantized forward, pinned bit for bit: for every case the SHA-256 of the output bytes of
cuembed_amd.embedding_forward_quantized, compared with tests/golden/quantized_forward_bits.json.  The documents promise
fp32 accumulation strictly in lookup order (one fma per code, the bag's bias once) and scheduling hints -- row-load
policy, sample_order -- that change no bit; the fp64 bounds and the "fixed = CSR" checks of test_gpu_quantized.py leave
room for a changed order, or for a lookup pooled twice with weight 0, this does not.

A case is one shape of the walk (which IndexSource, how many lanes, how many lookups around the unroll and the chunk of
the wave shuffle, a partial last workgroup); every case runs as int32 / int64 indices (offsets of the same type) x
weighted or not x sum / mean x fp32 / fp16 output, each with default and with streaming row loads (equal fingerprints,
asserted), the CSR cases also with a sample_order permutation (equal fingerprints, asserted).

The inputs are integer arithmetic in numpy (a multiplicative hash; no RNG stream); the table is quantized on the device
by quantize_rows from hashed fp32 values k / 9973 scaled per row, so the scales are no powers of two and the fp32 sums
round.  The results do not depend on the grid, so the fingerprints hold on any device.  The fixture is written by this
module run as a script,

    python tests/test_gpu_quantized_forward_bits.py --record [--commit ID] [--out FILE]

on a build of the commit whose behaviour is to be kept; `recorded_from` names that commit.  A fingerprint that differs
means that a kernel edit changed an operation or an order: fix the kernel, never the fixture."""
import functools
import hashlib
import itertools
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "quantized_forward_bits.json")
INDEX = {"i32": torch.int32, "i64": torch.int64}
OUT = {"f32": torch.float32, "f16": torch.float16}
NUM_ROWS = 300
# width -> (codes per lane, lanes per row): one 4-code and one 8-code lane; 2, 4 and 64 lanes of 16 codes (divide 64: the
# wave shuffle when not staged); 3 and 5 lanes of 8 codes and 9 lanes of 4 codes (do not divide 64: the global source)
WIDTHS = {4: (4, 1), 8: (8, 1), 32: (16, 2), 64: (16, 4), 24: (8, 3), 40: (8, 5), 36: (4, 9), 1024: (16, 64)}
STAGED_HOTNESS = (1, 7, 8, 9, 17)          # around the unroll of 8, and of 4 for 16 codes per lane
STAGED_BATCH = 41                          # the last workgroup is partial: some threads leave after the barrier
LONG_HOTNESS, LONG_BATCH, LONG_WIDTHS = 1400, 3, (64, 36)    # int64 indices + fp32 weights: too long to stage
CSR_WIDTHS = (64, 1024, 36)                # groups of 4 and 64 lanes (wave shuffle) and of 9 (global)
# (index, weighted, mode, out): the sixteen variants of a case
VARIANTS = list(itertools.product(("i32", "i64"), (False, True), ("sum", "mean"), ("f32", "f16")))


def variant_id(index, weighted, mode, out):
    return "-".join([index, "weighted" if weighted else "plain", mode, out])


def hashed(n, salt):
    """uint64 [n]: a multiplicative hash of (position, salt), in 64-bit integer arithmetic reduced mod 2^32."""
    mask = np.uint64(0xFFFFFFFF)
    h = (np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B1) + np.uint64(salt * 0xC2B2AE35 + 0x85EBCA6B)) & mask
    h = (h * np.uint64(0x27D4EB2F)) & mask
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(0x165667B1)) & mask
    h ^= h >> np.uint64(13)
    return h


def shuffled(n, salt):
    """A permutation of range(n): i -> (a * i + salt) mod n with a coprime to n."""
    a = next(a for a in range(max(2, (5 * n) // 8), 3 * n + 8) if math.gcd(a, n) == 1)
    return (np.arange(n, dtype=np.int64) * a + salt) % n


@functools.lru_cache(maxsize=None)
def qtable(width):
    """The fused table of a width, quantized on the device from hashed fp32 values off every dyadic grid: k / 9973 with
    |k| <= 10005, times 1 + (row mod 7) / 7.  Never modified."""
    import cuembed_amd
    k = (hashed(NUM_ROWS * width, 1) % np.uint64(20011)).astype(np.int64) - 10005
    x = (k.astype(np.float32) / np.float32(9973)).reshape(NUM_ROWS, width)
    x *= (np.float32(1) + (np.arange(NUM_ROWS) % 7).astype(np.float32) / np.float32(7))[:, None]
    q = cuembed_amd.quantize_rows(torch.from_numpy(x).cuda())
    scales = q[:, width:width + 4].contiguous().view(torch.float32).cpu().numpy().ravel()
    mant = np.frexp(scales)[0]
    assert np.count_nonzero(mant != 0.5) > NUM_ROWS // 2, "the scales are powers of two: the sums would not round"
    return q


@functools.lru_cache(maxsize=None)
def lookups(nnz, salt):
    """(row ids, weights for sum in (-1, 1), weights for mean in [0.25, 1.25]) as numpy, never modified."""
    ids = (hashed(nnz, salt) % np.uint64(NUM_ROWS)).astype(np.int64)
    w_sum = ((hashed(nnz, salt + 1) % np.uint64(2001)).astype(np.int64) - 1000).astype(np.float32) / np.float32(1001)
    w_mean = np.float32(0.25) + (hashed(nnz, salt + 2) % np.uint64(1001)).astype(np.float32) / np.float32(1000)
    return ids, w_sum, w_mean


def csr_lengths(group):
    """Bag lengths 0 .. 2 * group + 1 in order, an empty bag, the same lengths shuffled, an empty bag: the chunk loop of
    the wave shuffle runs zero, one, two and three times with full and partial last chunks; the first, a middle and
    the last bag are empty."""
    n = 2 * group + 2
    return np.concatenate([np.arange(n), [0], shuffled(n, 3), [0]]).astype(np.int64)


def sha(t):
    t = t.detach().contiguous().cpu()
    return hashlib.sha256(t.view(torch.int16 if t.element_size() == 2 else torch.int32).numpy().tobytes()).hexdigest()


def run_case(ce, width, num_hots, batch, lengths, salt, expect_staged):
    """variant id -> fingerprint.  Streaming row loads and (CSR) a sample_order must reproduce it."""
    codes, lanes = WIDTHS[width]
    q = qtable(width)
    is_csr = lengths is not None
    nnz = int(lengths.sum()) if is_csr else batch * num_hots
    ids, w_sum, w_mean = lookups(nnz, salt)
    order = torch.from_numpy(shuffled(batch, 5).astype(np.int32)).cuda() if is_csr else None
    got = {}
    for index, weighted, mode, out in VARIANTS:
        shape = ce.quantized_forward_launch_shape(INDEX[index], OUT[out], width, batch, num_hots, is_csr=is_csr,
                                                  is_weighted=weighted, compute_units=0)
        assert (shape["codes_per_lane"], shape["lanes_per_row"]) == (codes, lanes)
        if expect_staged is not None and (expect_staged or (index, weighted, out) == ("i64", True, "f32")):
            assert shape["staged"] == expect_staged, "W = %d, hotness %d moved to another index source" % (width, num_hots)
        kw = dict(mode=mode, out_dtype=OUT[out], batch_size=batch)
        if weighted:
            kw["weights"] = torch.from_numpy(w_mean if mode == "mean" else w_sum).to(OUT[out]).cuda()
        if is_csr:
            off = np.concatenate([[0], np.cumsum(lengths)])
            kw["offsets"] = torch.from_numpy(off).to(INDEX[index]).cuda()
        else:
            kw["num_hots"] = num_hots
        idx = torch.from_numpy(ids).to(INDEX[index]).cuda()
        y = ce.embedding_forward_quantized(q, idx, **kw)
        assert bool(y.ne(0).any()), "the case pooled nothing"
        h = sha(y)
        name = variant_id(index, weighted, mode, out)
        assert sha(ce.embedding_forward_quantized(q, idx, row_loads="streaming", **kw)) == h, name + ": streaming row loads"
        if is_csr:
            assert sha(ce.embedding_forward_quantized(q, idx, sample_order=order, **kw)) == h, name + ": sample_order"
            assert sha(ce.embedding_forward_quantized(q, idx, sample_order=order, row_loads="streaming", **kw)) == h, \
                name + ": sample_order, streaming row loads"
        got[name] = h
    return got


def all_cases():
    """case id -> the function of `ce` that computes its fingerprints."""
    cases = {}
    for width in WIDTHS:
        for h in STAGED_HOTNESS:
            cases["staged-W%d-H%d" % (width, h)] = functools.partial(
                run_case, width=width, num_hots=h, batch=STAGED_BATCH, lengths=None, salt=10 + h, expect_staged=True)
    for width in LONG_WIDTHS:
        cases["long-W%d-H%d" % (width, LONG_HOTNESS)] = functools.partial(
            run_case, width=width, num_hots=LONG_HOTNESS, batch=LONG_BATCH, lengths=None, salt=40, expect_staged=False)
    for width in CSR_WIDTHS:
        lengths = csr_lengths(WIDTHS[width][1])
        cases["csr-W%d" % width] = functools.partial(
            run_case, width=width, num_hots=0, batch=len(lengths), lengths=lengths, salt=50, expect_staged=None)
    return cases


CASES = all_cases()


@pytest.fixture(scope="module")
def ce():
    import cuembed_amd
    assert torch.cuda.is_available()
    return cuembed_amd


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_fixture_holds_exactly_these_cases(golden):
    assert sorted(golden["cases"]) == sorted(CASES)
    names = sorted(variant_id(*v) for v in VARIANTS)
    assert all(sorted(v) == names for v in golden["cases"].values())
    assert set(golden["recorded_from"]) >= {"commit", "device", "torch"}


@pytest.mark.parametrize("case", sorted(CASES))
def test_forward_bit_for_bit(ce, golden, case):
    got = CASES[case](ce)
    want = golden["cases"][case]
    wrong = sorted(v for v in want if got[v] != want[v])
    assert not wrong, "%s: the output differs from %s's for %d of %d variants: %s" % (
        case, golden["recorded_from"]["commit"][:12], len(wrong), len(want), ", ".join(wrong))


def record(argv):
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import cuembed_amd
    commit = argv[argv.index("--commit") + 1] if "--commit" in argv else subprocess.check_output(
        ["git", "rev-parse", "HEAD"], cwd=root, text=True).strip()
    out = argv[argv.index("--out") + 1] if "--out" in argv else GOLDEN
    doc = {"recorded_from": {"commit": commit, "device": torch.cuda.get_device_name(0),
                             "arch": torch.cuda.get_device_properties(0).gcnArchName, "torch": torch.__version__},
           "cases": {case: CASES[case](cuembed_amd) for case in sorted(CASES)}}
    with open(out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("recorded %d cases from %s into %s" % (len(doc["cases"]), commit[:12], out))


if __name__ == "__main__":
    if "--record" not in sys.argv:
        sys.exit(__doc__)
    record(sys.argv)
