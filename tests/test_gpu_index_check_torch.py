"""The index check as a torch op and inside the group modules.

    torch.ops.cuembed_pyt.cuembed_check_indices agrees with cuembed_amd.check_indices;
    bounds_check="repair": EmbeddingBagGroup / QuantizedEmbeddingBagGroup on a batch with bad ids and offsets return, bit
        for bit, the forward of the batch repaired ON THE HOST by the numpy model (tests/index_check_reference.py);
    bounds_check="raise": IndexError naming the position and the table, before the forward is launched;
    bounds_check=None: what the module launched before -- identical outputs, no .last_check;
    check with repair + the grouped forward captured ONCE into a HIP graph and replayed on a clean, a bad and a clean batch.

The forward only ever sees repaired (or clean) batches: bad data goes into the check alone.
"""
import numpy as np
import pytest
import torch

import grouped_cases as C
import index_check_reference as M

pytestmark = pytest.mark.gpu

WIDTH, BATCH = 128, 5
T = len(C.ROWS)


@pytest.fixture(scope="module")
def ce():
    import cuembed_amd
    assert torch.cuda.is_available()
    return cuembed_amd


@pytest.fixture(scope="module")
def tables():
    return [torch.from_numpy(C.table_values(t, rows, WIDTH).astype(np.float16)).cuda() for t, rows in enumerate(C.ROWS)]


def batches():
    """{name: (clean ids, clean offsets or None, hot)} at B = 5, int64."""
    return {name: (ids, off, hot) for name, ids, off, hot, _ in C.layouts(BATCH)}


def corrupt(ids, offsets, hot):
    """A copy with bad ids (negative, exactly rows_t, valid for a neighbouring table only) and, for CSR, a decreasing
    offset and an end past nnz.  The model says what is left of it."""
    ids, nnz = ids.copy(), ids.size
    if offsets is not None:
        offsets = offsets.copy()
        cuts = offsets[::BATCH]
        assert cuts[1] < nnz
        ids[cuts[1]] = 4000                  # the first lookup of table 1 (17 rows) -- of table 2 (300) where table 1 is empty
        mid = 7
        offsets[mid] = offsets[mid - 1] - 1 if offsets[mid - 1] > 0 else -1
        offsets[-1] = nnz + 9
    else:
        per_table = BATCH * hot
        ids[per_table] = 17                  # first of table 1: a row of tables 0 and 2 only
        ids[2 * per_table - 1] = 4999        # last of table 1
    ids[0] = -1
    ids[nnz - 1] = C.ROWS[2]
    ids[nnz // 2] = np.iinfo(np.int64).min
    return ids, offsets


def repaired_on_the_host(ids, offsets, hot):
    report, fixed, fixed_offsets = M.check(ids, offsets, C.ROWS, BATCH, hot)
    return report, fixed, fixed_offsets


def dev(a):
    return None if a is None else torch.from_numpy(a).cuda()


def test_the_op_agrees_with_the_function(ce):
    from cuembed_amd import cuembed_pyt  # noqa: F401  (loads the ops)
    op = torch.ops.cuembed_pyt.cuembed_check_indices
    group = ce.TableGroup([torch.zeros((r, 4), device="cuda") for r in C.ROWS])
    for name, (ids, off, hot) in batches().items():
        for bad in (False, True):
            i, o = corrupt(ids, off, hot) if bad else (ids, off)
            for dtype in (torch.int32, torch.int64):
                di = dev(i).to(dtype) if dtype == torch.int64 else dev(np.clip(i, -2 ** 31, 2 ** 31 - 1)).to(dtype)
                do = None if o is None else dev(o).to(dtype)
                for repair in (False, True):
                    want = ce.check_indices(di, do, group=group, num_hots=hot, repair=repair)
                    report, out_i, out_o = op(di, do, group.row_base_device, 0, T, BATCH, hot, repair)
                    assert torch.equal(report, want.report), (name, bad, dtype, repair)
                    assert (report[0] > 0) == bad
                    if repair:
                        assert out_i.dtype == dtype and torch.equal(out_i, want.indices)
                        assert (out_o.numel() == 0) if o is None else torch.equal(out_o, want.offsets)
                    else:
                        assert out_i.numel() == 0 and out_o.numel() == 0
    # one table, no row_base
    single = torch.tensor([0, 16, 17, -1, 5], device="cuda")
    offsets = torch.tensor([0, 2, 5], device="cuda")
    report, out_i, out_o = op(single, offsets, None, 17, 1, 2, 0, True)
    assert report.tolist() == [2, 2, 0, -1] and out_i.tolist() == [0, 16, 0, 0, 5] and torch.equal(out_o, offsets)
    report, _, _ = op(single[:4].view(1, 2, 2), None, None, 17, 1, 2, 2, False)
    assert report.tolist() == [2, 2, 0, -1]
    with pytest.raises(RuntimeError, match="num_rows >= 1"):
        op(single, offsets, None, 0, 1, 2, 0, False)
    with pytest.raises(RuntimeError, match="without row_base"):
        op(single, offsets, None, 17, 3, 2, 0, False)


_PYTHON_BACKEND_CHILD = """
import sys, torch
sys.path.insert(0, %r)
import cuembed_amd as ce
from cuembed_amd import cuembed_pyt as P
assert P.BACKEND == "python"
op = torch.ops.cuembed_pyt.cuembed_check_indices
group = ce.TableGroup([torch.zeros((r, 4), device="cuda") for r in (5000, 17, 300)])
idx = torch.tensor([4999, 5000, 16, 17, -1, 299, 300], device="cuda", dtype=torch.int32)
off = torch.tensor([0, 2, 9, 4], device="cuda")
for repair in (False, True):
    want = ce.check_indices(idx, off, group=group, repair=repair)
    report, out_i, out_o = op(idx, off, group.row_base_device, 0, 3, 1, 0, repair)
    assert torch.equal(report, want.report) and report.tolist() == [5, 1, 2, 2], report.tolist()   # table 1 owns [2, 7)
    if repair:
        assert torch.equal(out_i, want.indices) and torch.equal(out_o, want.offsets) and out_o.tolist() == [0, 2, 7, 7]
    else:
        assert out_i.numel() == 0 and out_o.numel() == 0
report, _, _ = op(idx[:6].view(1, 3, 2), None, None, 17, 1, 3, 2, False)
assert report.tolist() == [5, 0, 0, -1], report.tolist()
print("python backend OK")
"""


def test_the_op_from_the_python_backend():
    """CUEMBED_PYT_BACKEND=python registers the same op from Python (a fresh process: the backend is chosen at import)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, CUEMBED_PYT_BACKEND="python")
    r = subprocess.run([sys.executable, "-c", _PYTHON_BACKEND_CHILD % root], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and "python backend OK" in r.stdout, r.stdout


def modules(ce, tables, bounds_check):
    return (ce.EmbeddingBagGroup(tables, mode="sum", bounds_check=bounds_check),
            ce.QuantizedEmbeddingBagGroup.from_float(tables, mode="mean", out_dtype=torch.float32,
                                                     bounds_check=bounds_check))


def test_repair_mode_gives_the_forward_of_the_host_repaired_batch(ce, tables):
    for bags, plain in zip(modules(ce, tables, "repair"), modules(ce, tables, None)):
        for name, (ids, off, hot) in batches().items():
            bad_ids, bad_off = corrupt(ids, off, hot)
            report, fixed_ids, fixed_off = repaired_on_the_host(bad_ids, bad_off, hot)
            assert report[0] >= 3 and (off is None or report[2] >= 2)

            def shaped(a):
                return a if off is not None else a.reshape(T, BATCH, hot)

            want = plain(dev(shaped(fixed_ids)), dev(fixed_off))
            got = bags(dev(shaped(bad_ids)), dev(bad_off))
            assert torch.equal(got, want), (type(bags).__name__, name)
            check = bags.last_check
            assert check.repaired and check.words() == tuple(int(w) for w in report), (name, check.words())
            assert np.array_equal(check.indices.cpu().numpy().reshape(-1), fixed_ids)
            assert off is None or np.array_equal(check.offsets.cpu().numpy(), fixed_off)
            assert plain.last_check is None


def test_raise_mode_raises_before_the_forward(ce, tables):
    for bags in modules(ce, tables, "raise"):
        for name, (ids, off, hot) in batches().items():
            bad_ids, bad_off = corrupt(ids, off, hot)
            report, _, _ = repaired_on_the_host(bad_ids, bad_off, hot)
            out = torch.full((BATCH, T, WIDTH), 7.0, dtype=torch.float32 if bags.group.quantized else torch.float16,
                             device="cuda")
            idx = dev(bad_ids if off is not None else bad_ids.reshape(T, BATCH, hot))
            with pytest.raises(IndexError) as err:
                bags(idx, dev(bad_off), out=out)
            text = str(err.value)
            assert "%d bad indices, first at position 0 (table 0 of 5000 rows): indices[0] = -1" % report[0] in text, text
            if off is not None:
                assert "%d bad offsets, first at position %d (table %d)" % (report[2], report[3], report[3] // BATCH) in text
            torch.cuda.synchronize()
            assert bool((out == 7.0).all()), "the forward must not have been launched"
            # a clean batch goes through, with the bits of the unchecked module
            clean = dev(ids if off is not None else ids.reshape(T, BATCH, hot))
            assert bags(clean, dev(off)) is not None and bags.last_check.words() == (0, -1, 0, -1)


def test_no_bounds_check_launches_what_it_launched_before(ce, tables):
    for bags, checked in zip(modules(ce, tables, None), modules(ce, tables, "repair")):
        for name, (ids, off, hot) in batches().items():
            idx = dev(ids if off is not None else ids.reshape(T, BATCH, hot))
            if bags.group.quantized:
                want = ce.embedding_forward_quantized_grouped(bags.group, idx, dev(off), num_hots=hot, mode="mean",
                                                              out_dtype=torch.float32)
            else:
                want = ce.embedding_forward_grouped(bags.group, idx, dev(off), num_hots=hot, mode="sum")
            assert torch.equal(bags(idx, dev(off)), want), name
            assert bags.last_check is None
            assert torch.equal(checked(idx, dev(off)), want), name        # clean: the repair is a bit-identical copy
            assert checked.last_check.words() == (0, -1, 0, -1)


def test_check_and_forward_in_one_graph(ce, tables):
    """Captured once: check with repair into static buffers + the grouped forward on them.  Replayed on a clean, a bad and
    a clean batch copied into the static inputs: outputs and reports match the eager results on the host-repaired batch."""
    group = ce.TableGroup(tables)
    clean_ids, clean_off, hot = batches()["csr_ragged"]
    bad_ids, bad_off = corrupt(clean_ids, clean_off, hot)
    idx, off = dev(clean_ids), dev(clean_off)
    safe_idx, safe_off = torch.empty_like(idx), torch.empty_like(off)
    report = ce.new_index_report("cuda")
    need = ce.check_indices_workspace_bytes(T, BATCH)
    workspace = torch.full((need,), 0xFF, dtype=torch.uint8, device="cuda")
    out = torch.empty((BATCH, T, WIDTH), dtype=torch.float16, device="cuda")

    def step():
        check = ce.check_indices(idx, off, group=group, repair=True, out_indices=safe_idx, out_offsets=safe_off,
                                 report=report, workspace=workspace)
        ce.embedding_forward_grouped(group, check.indices, check.offsets, mode="sum", out=out)

    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        step()                               # warm-up outside capture (module loading, group.row_base_device)
        torch.cuda.current_stream().synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            step()
    for which, (ids, offsets) in enumerate(((clean_ids, clean_off), (bad_ids, bad_off), (clean_ids, clean_off))):
        idx.copy_(dev(ids))
        off.copy_(dev(offsets))
        out.zero_()
        report.fill_(77)
        g.replay()
        torch.cuda.synchronize()
        want_report, fixed_ids, fixed_off = repaired_on_the_host(ids, offsets, hot)
        assert report.tolist() == want_report.tolist(), which
        assert (want_report[0] > 0) == (which == 1)
        eager = ce.embedding_forward_grouped(group, dev(fixed_ids), dev(fixed_off), mode="sum")
        assert torch.equal(out, eager), which
        assert np.array_equal(safe_idx.cpu().numpy(), fixed_ids) and np.array_equal(safe_off.cpu().numpy(), fixed_off)
