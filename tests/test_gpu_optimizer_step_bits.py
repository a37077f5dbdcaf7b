"""The sparse optimizer step, pinned bit for bit: for every case two consecutive steps through the public entry points
(cuembed_amd.sparse_row_update / sparse_row_adam), and after each step the SHA-256 of the table's bytes followed by the
state tensors' bytes, compared with tests/golden/optimizer_step_bits.json.  The documents promise fp32 arithmetic with
one unfused IEEE operation per step, one rounding at the store and stochastic bits that depend on (seed, step, row,
column) only; the fp64 bounds of the other suites leave room for a changed operation or order, this does not.

The inputs are integer arithmetic in numpy (a multiplicative hash), the results do not depend on the grid, so the
fingerprints hold on any device.  The fixture is written by this module run as a script,

    python tests/test_gpu_optimizer_step_bits.py --record [--commit ID] [--out FILE]

on a build of the commit whose behaviour is to be kept; `recorded_from` names that commit.  A fingerprint that differs
means that a kernel edit changed an operation or an order: fix the kernel, never the fixture.  Every fingerprint is
also reproduced on the CPU by an independent numpy-float32 statement of the contract (test_optimizer_bits_host.py)."""
import functools
import hashlib
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "optimizer_step_bits.json")
TORCH = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
INDEX = {"i32": torch.int32, "i64": torch.int64}
RULES = ["sgd", "adagrad", "rowwise_adagrad", "adam", "rowwise_adam"]
LR, EPS, BETAS, WEIGHT_DECAY, SEED = 0.01, 1e-8, (0.9, 0.999), 0.01, 1234
STEPS = (1, 2)

# width -> slices per lane (0: the run-time loop).  16-bit: 8 = one 16-byte lane; 50 = 4-byte lanes (N = 2, 25 lanes in
# a group of 32); 64 = one slice per lane, two entries in flight; 1000 = 125 lanes, four slices with a partial second
# and empty third and fourth; 2056 = 257 lanes.  fp32: two lanes; 8-byte lanes; one slice; 250 lanes, four slices with
# a partial last; 512 lanes.
WIDTHS = {"f16": {8: 1, 50: 1, 64: 1, 1000: 4, 2056: 0},
          "bf16": {8: 1, 50: 1, 64: 1, 1000: 4, 2056: 0},
          "f32": {8: 1, 50: 1, 64: 1, 1000: 4, 2048: 0}}
ROUNDINGS = {"f16": ("nearest", "stochastic"), "bf16": ("nearest", "stochastic"), "f32": ("nearest",)}
SMALL_NCAT, SMALL_N, SMALL_TAIL = 512, 200, 5
GRID_NCAT, GRID_N, GRID_WIDTH = 80000, 70000, 64
PIECE_ROWS, PIECE_COUNTS = 64, (64, 0, 65)     # the third count is over capacity: that piece changes nothing


def small_cases():
    out = []
    for kind, widths in WIDTHS.items():
        for width in widths:
            for index in ("i32", "i64") if width == 64 else ("i32",):
                out += [(kind, width, index, rounding) for rounding in ROUNDINGS[kind]]
    return out


def case_id(group, rule, *rest):
    return "-".join([group, rule] + [str(x) for x in rest])


def hashed(nrows, ncols, step, salt):
    """fp32 [nrows, ncols] of multiples of 2^-10 in [-1, 1): the top 11 bits of a multiplicative hash of (row, column,
    step), in 64-bit integer arithmetic reduced mod 2^32."""
    mask = np.uint64(0xFFFFFFFF)
    r = np.arange(nrows, dtype=np.uint64)[:, None]
    c = np.arange(ncols, dtype=np.uint64)[None, :]
    h = (r * np.uint64(0x9E3779B1) + c * np.uint64(0x85EBCA6B) + np.uint64(step * 0xC2B2AE35 + salt)) & mask
    h = (h * np.uint64(0x27D4EB2F)) & mask
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(0x165667B1)) & mask
    return ((h >> np.uint64(21)).astype(np.int64) - 1024).astype(np.float32) / np.float32(1024)


def permutation(ncat, n):
    """The first n entries of i -> (40503 * i + 7) mod ncat: distinct and unsorted."""
    assert math.gcd(40503, ncat) == 1 and n <= ncat
    return (np.arange(n, dtype=np.int64) * 40503 + 7) % ncat


@functools.lru_cache(maxsize=None)
def problem(kind, ncat, n, tail, width):
    """(table, ids as int64, the gradient rows of steps 1 and 2) on the CPU, never modified: n distinct ids, then `tail`
    entries past the count that name the first rows again, with gradient rows of magnitude 1."""
    table = torch.from_numpy(hashed(ncat, width, 0, 1)).to(TORCH[kind])
    ids = permutation(ncat, n)
    ids = torch.from_numpy(np.concatenate([ids, ids[:tail]]))
    rows = []
    for t in STEPS:
        g = hashed(n + tail, width, t, 2)
        g[n:] = 1.0
        rows.append(torch.from_numpy(g).to(TORCH[kind]))
    return table, ids, rows


def fresh_state(rule, ncat, width):
    """The state tensors of a rule, zero: the second step then starts from non-zero state."""
    per_element = lambda: torch.zeros((ncat, width), dtype=torch.float32, device="cuda")
    per_row = lambda: torch.zeros((ncat,), dtype=torch.float32, device="cuda")
    return {"sgd": [], "adagrad": [per_element()], "rowwise_adagrad": [per_row()], "adam": [per_element(), per_element()],
            "rowwise_adam": [per_element(), per_row()]}[rule]


def raw_bytes(t):
    t = t.detach().contiguous().cpu()
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32).numpy().tobytes()


def fingerprints(ce, rule, kind, ncat, n, tail, width, index, rounding, **count):
    """The two steps of one case: [sha256(table, state...) after step 1, after step 2]."""
    table0, ids, rows = problem(kind, ncat, n, tail, width)
    table, ids = table0.cuda(), ids.to(INDEX[index]).cuda()
    state = fresh_state(rule, ncat, width)
    kw = dict(count) if count else dict(count=n)
    out = []
    for t, g in zip(STEPS, rows):
        if rounding == "stochastic":
            kw.update(stochastic_rounding=True, seed=SEED, step=t)
        if rule in ("adam", "rowwise_adam"):
            ce.sparse_row_adam(table, ids, g.cuda(), exp_avg=state[0], exp_avg_sq=state[1], lr=LR,
                               bias_factor=ce.adam_bias_factor(t, BETAS), betas=BETAS, eps=EPS,
                               weight_decay=WEIGHT_DECAY, rowwise=rule == "rowwise_adam", **kw)
        else:
            ce.sparse_row_update(table, ids, g.cuda(), rule=rule, lr=LR, state=state[0] if state else None, eps=EPS, **kw)
        h = hashlib.sha256(raw_bytes(table))
        for s in state:
            h.update(raw_bytes(s))
        out.append(h.hexdigest())
    assert not torch.equal(table.cpu(), table0), "the steps changed nothing"
    return out


def small_fingerprints(ce, rule, kind, width, index, rounding):
    want = WIDTHS[kind][width]
    got = ce.sparse_row_update_launch_shape(TORCH[kind], width, SMALL_N + SMALL_TAIL)["slices_per_lane"]
    assert got == want, "W = %d moved to another body of the walk: %d slices per lane, not %d" % (width, got, want)
    return fingerprints(ce, rule, kind, SMALL_NCAT, SMALL_N, SMALL_TAIL, width, index, rounding)


def grid_fingerprints(ce, rule, rounding):
    shape = ce.sparse_row_update_launch_shape(torch.float16, GRID_WIDTH, 1 << 30, compute_units=0)
    assert shape["slices_per_lane"] == 1
    per_pass = shape["grid"] * (256 // shape["lanes_per_entry"])     # 65,536 on 256 compute units
    assert GRID_N > per_pass, "every entry fits one pass of the grid: the second in-flight entry is never live"
    return fingerprints(ce, rule, "f16", GRID_NCAT, GRID_N, 0, GRID_WIDTH, "i32", rounding)


def pieces_fingerprints(ce, rule):
    counts = torch.tensor(PIECE_COUNTS, dtype=torch.int32, device="cuda")
    return fingerprints(ce, rule, "f16", SMALL_NCAT, len(PIECE_COUNTS) * PIECE_ROWS, 0, 64, "i32", "nearest",
                        counts=counts, piece_rows=PIECE_ROWS)


def all_cases():
    """case id -> the function of `ce` that computes its fingerprints."""
    cases = {}
    for rule in RULES:
        for kind, width, index, rounding in small_cases():
            cases[case_id("small", rule, kind, "W%d" % width, index, rounding)] = functools.partial(
                small_fingerprints, rule=rule, kind=kind, width=width, index=index, rounding=rounding)
        for rounding in ROUNDINGS["f16"]:
            cases[case_id("grid", rule, rounding)] = functools.partial(grid_fingerprints, rule=rule, rounding=rounding)
        cases[case_id("pieces", rule)] = functools.partial(pieces_fingerprints, rule=rule)
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
    assert all(len(v) == len(STEPS) for v in golden["cases"].values())
    assert set(golden["recorded_from"]) >= {"commit", "device", "torch"}


@pytest.mark.parametrize("case", sorted(CASES))
def test_two_steps_bit_for_bit(ce, golden, case):
    got = CASES[case](ce)
    want = golden["cases"][case]
    for t, g, w in zip(STEPS, got, want):
        assert g == w, "%s: the table or the state after step %d differs from %s's" % (
            case, t, golden["recorded_from"]["commit"][:12])


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
