"""The default backward, pinned bit for bit: for every case of backward_bits_cases.py one call of
cuembed_amd.embedding_backward (fp32 partial sums, not reference_sums) under a forced launch shape, with both output
buffers pre-filled with a fixed bit pattern, and the SHA-256 of grad_embedding's bytes, then inverse_mapping's bytes,
then the value of capacity_overflowed(reset=True), compared with tests/golden/backward_bits.json.  The other suites
compare with the oracle on exactly representable data and with fp64 bounds otherwise; a changed order of the fp32
additions passes both, it does not pass this.

set_backward_tuning(segment_len, column_slices) fixes the launch shape, so the arithmetic does not depend on the
device's CU count; the cases are built so that the float atomics across workgroups cannot round differently by arrival
order (backward_bits_cases.py; test_backward_bits_host.py asserts it for every case).  Cases on exact data must also
equal the CPU oracle.  Sample-blocked cases need more than 32 sort tiles (135,245 lookups); the others have a few
hundred to about 20,000.  The fixture is written by this module run as a script,

    python tests/test_gpu_backward_bits.py --record [--commit ID] [--out FILE]

on a build of the commit whose behaviour is to be kept; `recorded_from` names that commit.  A fingerprint that differs
means that a kernel edit changed an operation or an order: fix the kernel, never the fixture."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

import backward_bits_cases as C

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "backward_bits.json")
TORCH = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
INDEX = {"i32": torch.int32, "i64": torch.int64}
EXTRA_ROWS = {"fit": 0, "over": 5, "small": -1, "pad": 37}


def pinned_shape(ce, case, nnz=1000, **device):
    """The launch shape under the case's forced tuning (it does not depend on nnz then); the tuning is restored."""
    ce.set_backward_tuning(case.segment_len, case.slices)
    try:
        return ce.backward_launch_shape(TORCH[case.kind], INDEX[case.index], case.width, nnz, case.weighted, **device)
    finally:
        ce.set_backward_tuning(0, 0)


def raw_bytes(t):
    t = t.detach().contiguous().cpu()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]).numpy().tobytes()


def planned_shape(ce, case):
    """The case's launch shape on a full chip, which this device must plan too."""
    full = pinned_shape(ce, case, compute_units=256, xcds=8)
    here = pinned_shape(ce, case)
    keep = ("column_slices", "lanes", "segments_per_block", "segment_len")
    assert [here[k] for k in keep] == [full[k] for k in keep], "this device plans another launch shape: %r" % (here,)
    assert full["column_slices"] == case.slices
    return full


def launch_case(ce, case, d, gy=None, w=None):
    """The call sequence of one case on the inputs `d` (backward_bits_cases.build's dict; gy / w: device tensors to use
    in place of d's grad_y / weights).  Returns (grad_embedding, inverse_mapping, the overflow word, and
    backward_bits_cases.compressed_ids(keys))."""
    dev = lambda a, dtype: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()
    elem, index = TORCH[case.kind], INDEX[case.index]
    gy = dev(d["grad_y"], elem) if gy is None else gy
    w = dev(d["weights"], elem) if w is None else w
    keys, sids = dev(d["keys"], index), dev(d["sids"], index)
    dense_ids, order, unique = C.compressed_ids(d["keys"])
    table = None
    if case.blocks > 1:
        assert ce.transpose_sample_block_length(d["nnz"], case.blocks) == d["block_len"]
        t_idx, t_sid, t_w = ce.transpose(sids, keys, w, sample_blocks=case.blocks)
        assert torch.equal(t_idx, keys) and torch.equal(t_sid, sids)       # the blocks were sorted already
        remap, table, count = ce.compute_compressed_grad_indices_blocked(t_idx, case.blocks)
        assert int(count.item()) == unique
    else:
        t_idx, t_sid, t_w = keys, sids, w
        remap = None if case.out == "dense" else dev(dense_ids, index)
    ce.capacity_overflowed(reset=True)
    ce.set_backward_tuning(case.segment_len, case.slices)
    try:
        if case.out == "dense":
            grad = torch.full((d["rows"], case.width), C.PATTERN, dtype=elem, device="cuda")
            ce.embedding_backward(gy, d["rows"], t_idx, t_sid, None, t_w, grad_embedding=grad)
            inverse = torch.empty((0,), dtype=index)
        else:
            rows = unique + EXTRA_ROWS.get(case.out, 0)
            fill = 0.0 if case.out == "skip" else C.PATTERN
            grad = torch.full((rows, case.width), fill, dtype=elem, device="cuda")
            inverse = torch.full((rows,), C.INVERSE_PATTERN, dtype=index, device="cuda")
            ce.embedding_backward(gy, None if case.out in EXTRA_ROWS else unique, t_idx, t_sid, remap, t_w,
                                  skip_grad_init=case.out == "skip", grad_embedding=grad, inverse_mapping=inverse,
                                  sample_blocks=case.blocks, block_row_ids=table, pad_to_capacity=case.out == "pad")
        torch.cuda.synchronize()
    finally:
        ce.set_backward_tuning(0, 0)
    overflowed = ce.capacity_overflowed(reset=True)
    return grad, inverse, overflowed, (dense_ids, order, unique)


def run_case(ce, oracle, case):
    """One call; returns the fingerprint.  Exact data is also compared with the oracle."""
    full = planned_shape(ce, case)
    d = C.build(case, full["segment_len"], full["segments_per_block"])
    grad, inverse, overflowed, (dense_ids, order, unique) = launch_case(ce, case, d)
    assert overflowed == (case.out == "small")
    if case.out == "small":
        assert float(grad.float().max()) == C.PATTERN == float(grad.float().min()), "nothing may be written"
    elif case.data == "exact":
        weights = None if d["weights"] is None else d["weights"][order]
        if case.out == "dense":
            want, want_inverse = oracle.embedding_backward(d["grad_y"], case.width, d["rows"], d["keys"], d["sids"],
                                                           None, weights)
        else:
            sorted_keys = np.ascontiguousarray(d["keys"][order])
            want, want_inverse = oracle.embedding_backward(d["grad_y"], case.width, unique, sorted_keys,
                                                           np.ascontiguousarray(d["sids"][order]), dense_ids, weights)
            assert np.array_equal(inverse[:unique].cpu().numpy(), want_inverse)
        got = grad[:want.shape[0]].float().cpu().numpy()
        assert np.array_equal(got, want), "exact data: the gradient differs from the CPU oracle's"
    h = hashlib.sha256(raw_bytes(grad))
    h.update(raw_bytes(inverse))
    h.update(b"\x01" if overflowed else b"\x00")
    return h.hexdigest()


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
    assert sorted(golden["cases"]) == sorted(C.CASES)
    assert set(golden["recorded_from"]) >= {"commit", "device", "torch"}


@pytest.mark.parametrize("case", sorted(C.CASES))
def test_backward_bit_for_bit(ce, oracle, golden, request, case):
    request.addfinalizer(lambda: ce.set_backward_tuning(0, 0))
    got = run_case(ce, oracle, C.CASES[case])
    assert got == golden["cases"][case], "%s: grad_embedding, inverse_mapping or the overflow flag differs from %s's" % (
        case, golden["recorded_from"]["commit"][:12])


def record(argv):
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import cuembed_amd
    from oracle import oracle
    commit = argv[argv.index("--commit") + 1] if "--commit" in argv else subprocess.check_output(
        ["git", "rev-parse", "HEAD"], cwd=root, text=True).strip()
    out = argv[argv.index("--out") + 1] if "--out" in argv else GOLDEN
    doc = {"recorded_from": {"commit": commit, "device": torch.cuda.get_device_name(0),
                             "arch": torch.cuda.get_device_properties(0).gcnArchName, "torch": torch.__version__},
           "cases": {case: run_case(cuembed_amd, oracle, C.CASES[case]) for case in sorted(C.CASES)}}
    with open(out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("recorded %d cases from %s into %s" % (len(doc["cases"]), commit[:12], out))


if __name__ == "__main__":
    if "--record" not in sys.argv:
        sys.exit(__doc__)
    record(sys.argv)
