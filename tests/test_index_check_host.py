"""The index check without a GPU: the names exist at every layer (C++ header, C ABI, ctypes binding, torch op, Python,
modules), every host refusal is raised before a launch and in its documented order (the tensors here live on the CPU: a
call that got as far as the device check raises RuntimeError), the C ABI aborts on misuse before any launch, and the
numpy model keeps its own promises on random garbage."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import index_check_reference as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = (5000, 17, 300)


@pytest.fixture(scope="module")
def ce():
    import cuembed_amd
    return cuembed_amd


def group_of(ce, rows=ROWS):
    return ce.TableGroup([torch.zeros(n, 4) for n in rows])


# ---- the names -------------------------------------------------------------------------------------------------------

def test_the_names_exist_at_every_layer(ce):
    include = os.path.join(ROOT, "cuembed_amd", "csrc", "cuembed", "include")
    with open(os.path.join(include, "index_check.hpp")) as f:
        host = f.read()
    assert re.search(r"template <typename IndexT, typename OffsetT>\s*void CheckIndices\(", host)
    assert os.path.exists(os.path.join(include, "index_check_kernels.hpp"))
    pre = subprocess.run(["gcc", "-std=c99", "-E", "-P", "-x", "c", os.path.join(ROOT, "include", "cuembed_amd.h")],
                         check=True, stdout=subprocess.PIPE, text=True).stdout
    proto = re.search(r"void cuembed_check_indices\s*\(([^)]*)\)", pre)
    assert proto, "declared in plain C"
    assert len(proto.group(1).split(",")) == 16
    from cuembed_amd import build
    assert "c_api_index_check.hip" in build.UNITS
    L = ctypes.CDLL(build.build())
    assert hasattr(L, "cuembed_check_indices"), "exported"
    vp, i, l = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    fn = ce._lib.lib().cuembed_check_indices
    assert fn.restype is None
    assert list(fn.argtypes) == [vp, i, vp, i, l, vp, l, i, i, i, vp, vp, vp, vp, ctypes.POINTER(ctypes.c_size_t), vp]
    from cuembed_amd import cuembed_pyt  # noqa: F401  (loads the ops)
    schema = str(torch.ops.cuembed_pyt.cuembed_check_indices.default._schema)
    assert schema.endswith("-> (Tensor, Tensor, Tensor)") and "Tensor? offsets" in schema and "bool repair" in schema
    assert callable(ce.check_indices) and callable(ce.IndexCheck.raise_if_bad)
    for cls in (ce.EmbeddingBagGroup, ce.QuantizedEmbeddingBagGroup):
        assert "bounds_check" in cls.__init__.__code__.co_varnames


def test_the_python_backend_defines_the_same_op():
    """CUEMBED_PYT_BACKEND=python registers the ops from Python (a fresh process: the backend is chosen at import)."""
    import sys
    from cuembed_amd import cuembed_pyt  # noqa: F401
    native = str(torch.ops.cuembed_pyt.cuembed_check_indices.default._schema)
    code = ("import sys, torch\nsys.path.insert(0, %r)\nfrom cuembed_amd import cuembed_pyt as P\n"
            "assert P.BACKEND == 'python'\nprint(torch.ops.cuembed_pyt.cuembed_check_indices.default._schema)\n" % ROOT)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, CUEMBED_PYT_BACKEND="python"),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == native, r.stdout


def test_the_modules_take_a_bounds_check(ce):
    tables = [torch.zeros(n, 8) for n in (3, 5)]
    for mode in (None, "raise", "repair"):
        bags = ce.EmbeddingBagGroup(tables, bounds_check=mode)
        assert bags.bounds_check == mode and bags.last_check is None
        qbags = ce.QuantizedEmbeddingBagGroup([torch.zeros(n, 16, dtype=torch.uint8) for n in (3, 5)], bounds_check=mode)
        assert qbags.bounds_check == mode and qbags.last_check is None
    assert ce.EmbeddingBagGroup(tables).bounds_check is None
    for cls, arg in ((ce.EmbeddingBagGroup, tables),
                     (ce.QuantizedEmbeddingBagGroup, [torch.zeros(3, 16, dtype=torch.uint8)])):
        with pytest.raises(ValueError, match="bounds_check must be None, 'raise' or 'repair'"):
            cls(arg, bounds_check="warn")


# ---- the refusals, in order ------------------------------------------------------------------------------------------

def test_a_valid_call_gets_as_far_as_the_device_check(ce):
    idx, off = torch.zeros(6, dtype=torch.int64), torch.zeros(4, dtype=torch.int32)
    for kwargs in (dict(num_rows=7), dict(group=group_of(ce)), dict(num_rows=7, repair=True),
                   dict(num_rows=7, repair=True, out_indices=idx, out_offsets=off),
                   dict(num_rows=7, repair=True, out_indices=torch.zeros(6, dtype=torch.int64))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ce.check_indices(idx, off, **kwargs)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ce.check_indices(idx.view(1, 3, 2), num_rows=7, num_hots=2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ce.check_indices(idx, group=group_of(ce), num_hots=2)
    for bags in (ce.EmbeddingBagGroup([torch.zeros(n, 8) for n in ROWS], bounds_check="repair"),
                 ce.QuantizedEmbeddingBagGroup([torch.zeros(n, 16, dtype=torch.uint8) for n in ROWS], bounds_check="raise")):
        with pytest.raises(RuntimeError, match="no CPU fallback"):       # the check runs in front of the forward
            bags(idx, off)


def test_the_refusals_come_in_their_documented_order(ce):
    """Each call is wrong in the named way AND in every way named after it."""
    idx = torch.zeros(6, dtype=torch.int64)
    off = torch.zeros(4, dtype=torch.int64)
    bad_off = torch.zeros(5, dtype=torch.float32)
    out = torch.zeros(6, dtype=torch.int32)
    with pytest.raises(TypeError, match="indices must be a torch.Tensor"):
        ce.check_indices([1, 2], bad_off, num_rows=0, group=None, repair=False, out_indices=out)
    with pytest.raises(TypeError, match="indices must be int32 or int64"):
        ce.check_indices(idx.float(), bad_off, out_indices=out)
    with pytest.raises(ValueError, match="exactly one of num_rows"):
        ce.check_indices(idx, bad_off, out_indices=out)                                   # neither
    with pytest.raises(ValueError, match="exactly one of num_rows"):
        ce.check_indices(idx, bad_off, num_rows=0, group=group_of(ce), out_indices=out)   # both
    with pytest.raises(TypeError, match="num_rows must be an int"):
        ce.check_indices(idx, bad_off, num_rows=7.0, out_indices=out)
    with pytest.raises(ValueError, match="table 0 has 0 rows"):
        ce.check_indices(idx, bad_off, num_rows=0, out_indices=out)
    with pytest.raises(ValueError, match="table 1 has 0 rows"):
        ce.check_indices(idx, bad_off, group=group_of(ce, (5, 0, 3)), out_indices=out)
    with pytest.raises(ValueError, match="at most 1023 tables"):
        ce.check_indices(idx, bad_off, group=group_of(ce, (1,) * 1024), out_indices=out)
    with pytest.raises(ValueError, match="either CSR"):
        ce.check_indices(idx, bad_off, num_rows=7, num_hots=2, out_indices=out)           # both layouts
    with pytest.raises(ValueError, match="either CSR"):
        ce.check_indices(idx, None, num_rows=7, out_indices=out)                          # neither layout
    with pytest.raises(TypeError, match="offsets must be a torch.Tensor"):
        ce.check_indices(idx, [0, 6], num_rows=7, out_indices=out)
    with pytest.raises(TypeError, match="offsets must be int32 or int64"):
        ce.check_indices(idx, bad_off, num_rows=7, out_indices=out)
    with pytest.raises(ValueError, match="not a multiple of 3 tables"):
        ce.check_indices(idx, bad_off.long(), group=group_of(ce), out_indices=out)
    with pytest.raises(ValueError, match=r"num_tables \* batch_size \+ 1 = 3 entries, got 5"):
        ce.check_indices(idx, bad_off.long(), num_rows=7, batch_size=2, out_indices=out)
    with pytest.raises(ValueError, match=r"num_tables \* batch_size \* num_hots"):
        ce.check_indices(idx, None, group=group_of(ce), num_hots=4, batch_size=1, out_indices=out)
    with pytest.raises(ValueError, match="repair=True only"):
        ce.check_indices(idx, off, num_rows=7, out_indices=out)
    with pytest.raises(ValueError, match="a fixed-hotness batch has no offsets"):
        ce.check_indices(idx, None, num_rows=7, num_hots=2, repair=True, out_offsets=off, out_indices=out)
    with pytest.raises(TypeError, match="out_indices must have its input's dtype"):
        ce.check_indices(idx, off, num_rows=7, repair=True, out_indices=out, out_offsets=off[:3])
    with pytest.raises(ValueError, match="out_indices must have its input's 6 entries"):
        ce.check_indices(idx, off, num_rows=7, repair=True, out_indices=torch.zeros(5, dtype=torch.int64),
                         out_offsets=off[:3])
    both = torch.zeros(8, dtype=torch.int64)
    with pytest.raises(ValueError, match="out_indices must be its input .in place. or not overlap"):
        ce.check_indices(both[:6], off, num_rows=7, repair=True, out_indices=both[2:], out_offsets=off[:3])
    with pytest.raises(ValueError, match="out_offsets must have its input's 4 entries"):
        ce.check_indices(idx, off, num_rows=7, repair=True, out_offsets=off[:3], report=torch.zeros(4))
    with pytest.raises(ValueError, match="report must be an int64 tensor of 4 words"):
        ce.check_indices(idx, off, num_rows=7, report=torch.zeros(4))
    with pytest.raises(ValueError, match="report must be an int64 tensor of 4 words"):
        ce.check_indices(idx, off, num_rows=7, report=torch.zeros(3, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ce.check_indices(idx, off, num_rows=7, report=torch.zeros(4, dtype=torch.int64))


def test_the_workspace_query_is_host_arithmetic(ce):
    assert ce.check_indices_workspace_bytes(1, 0) == 768 and ce.check_indices_workspace_bytes(3, 5, num_hots=7) == 0
    small, three_tiles = ce.check_indices_workspace_bytes(3, 5), ce.check_indices_workspace_bytes(3, 1023)
    assert small == three_tiles == 768                      # two per-tile arrays and the cuts, 256 bytes each
    assert ce.check_indices_workspace_bytes(1023, 2 ** 21) == 2 * 1024 * 8 + 1024 * 8      # at most 1,024 tiles
    for batch in (0, 5, 1023, 1024, 2 ** 20 - 1, 2 ** 20, 2 ** 21 + 5, 2 ** 31 - 1):      # ... and the library agrees
        need = ctypes.c_size_t(0)
        ce._lib.lib().cuembed_check_indices(None, 1, None, 1, 0, None, 1, 1, batch, 0, None, None, None, None,
                                            ctypes.byref(need), None)
        assert ce.check_indices_workspace_bytes(1, batch) == need.value, batch
    with pytest.raises(ValueError):
        ce.check_indices_workspace_bytes(1024, 1)
    with pytest.raises(ValueError):
        ce.check_indices_workspace_bytes(3, 2 ** 30)


@pytest.mark.parametrize("call,names", [
    ("None,0,None,0,0,None,7,1,1,0,None,None,None,None,None,None", "lwork"),
    ("None,0,None,0,0,256,0,1024,1,0,None,None,None,None,N,None", "num_tables"),
    ("None,0,None,0,-1,None,7,1,1,0,None,None,None,None,N,None", "nnz >= 0"),
    ("None,0,None,0,0,None,0,1,1,0,None,None,None,None,N,None", "num_rows >= 1"),
    ("None,0,None,0,0,None,7,2,1,0,None,None,None,None,N,None", "row_base"),
    ("None,0,None,0,5,None,7,1,3,2,None,None,None,None,N,None", "bags * num_hots"),
    ("None,1,None,0,2**31,None,7,1,3,0,None,None,None,None,N,None", "INT32_MAX"),
    ("None,0,None,0,0,None,7,1,1,0,None,None,None,256,N,None", "report"),
    ("None,0,None,0,4,None,7,1,1,0,256,None,None,256,N,None", "indices != nullptr"),
    ("256,0,None,0,4,None,7,1,1,0,256,None,None,256,N,None", "offsets != nullptr"),
    ("256,0,256,0,4,None,7,1,2,2,256,None,None,256,N,None", "offsets == nullptr"),
    ("256,0,256,0,4,None,7,1,1,0,256,264,None,256,N,None", "apart(indices"),
    ("256,0,256,0,4,None,7,1,1,0,256,None,None,256,SMALL,None", "lwork >= plan.total"),
    ("256,2,256,0,4,None,7,1,1,0,256,None,None,256,N,None", "unsupported type code"),
])
def test_the_c_abi_aborts_on_misuse_before_any_launch(call, names):
    """CUEMBED_ASSERT: message on stderr + abort, in a child process.  The pointers are never dereferenced (256 is no
    address of anything): every check precedes every launch."""
    from cuembed_amd import build
    code = ("import ctypes\n"
            "from cuembed_amd import _lib\n"
            "L=_lib.lib()\n"
            "N=ctypes.byref(ctypes.c_size_t(1<<20))\n"
            "SMALL=ctypes.byref(ctypes.c_size_t(8))\n"
            "L.cuembed_check_indices(%s)\n" % call)
    assert os.path.exists(build.LIB_PATH)
    r = subprocess.run(["python3", "-c", code], stderr=subprocess.PIPE, text=True, cwd=ROOT)
    assert r.returncode != 0
    assert "Check failed" in r.stderr and names in r.stderr, r.stderr


# ---- the model's own properties --------------------------------------------------------------------------------------

def garbage_offsets(rng, n, nnz):
    kind = rng.integers(0, 4)
    if kind == 0:
        return np.sort(rng.integers(0, nnz + 1, n + 1))                                   # valid
    if kind == 1:
        return rng.integers(-nnz - 3, 2 * nnz + 3, n + 1)
    if kind == 2:
        return rng.integers(np.iinfo(np.int64).min, np.iinfo(np.int64).max, n + 1, endpoint=True)
    o = np.sort(rng.integers(0, nnz + 1, n + 1))
    o[rng.integers(0, n + 1)] = rng.choice([-1, nnz + 1, np.iinfo(np.int64).min, np.iinfo(np.int64).max])
    return o


def test_the_model_keeps_its_promises_on_random_garbage():
    rng = np.random.default_rng(5)
    seen_valid = seen_bad = 0
    for trial in range(300):
        T, batch = int(rng.integers(1, 4)), int(rng.integers(0, 7))
        n, nnz = T * batch, int(rng.integers(0, 40))
        o = garbage_offsets(rng, n, nnz).astype(np.int64)
        r = M.repair_offsets(o, nnz)
        bad = M.bad_offsets(o, nnz)
        assert M.offsets_valid(r, nnz), "the repaired offsets are always valid"
        assert np.array_equal(r, o) == M.offsets_valid(o, nnz), "the repair is the identity exactly on valid input"
        assert (bad.sum() == 0) == M.offsets_valid(o, nnz), "bad == 0 iff valid"
        assert np.array_equal(M.repair_offsets(r, nnz), r) and not M.bad_offsets(r, nnz).any()
        seen_valid += M.offsets_valid(o, nnz)
        seen_bad += not M.offsets_valid(o, nnz)
        rows = rng.integers(1, 9, T)
        ids = rng.integers(-3, 12, nnz)
        report, fixed, fixed_o = M.check(ids, o, rows, batch)
        assert np.array_equal(fixed_o, r) and report[2] == bad.sum()
        assert report[3] == (np.flatnonzero(bad)[0] if bad.any() else -1)
        again, same, _ = M.check(fixed, fixed_o, rows, batch)
        assert again.tolist() == [0, -1, 0, -1] and np.array_equal(same, fixed), "the repaired batch is clean"
        table, checked = M.table_of_positions(nnz, rows, batch, 0, r)
        for p in range(nnz):        # the definition, position by position
            inside = r[0] <= p < r[n]
            assert checked[p] == inside
            if inside:
                t = table[p]
                assert r[t * batch] <= p < r[(t + 1) * batch]
                assert (fixed[p] == ids[p]) == (0 <= ids[p] < rows[t]) or ids[p] == 0
            else:
                assert fixed[p] == ids[p]
    assert seen_valid >= 30 and seen_bad >= 100


def test_the_model_on_a_hand_written_batch():
    """The batch of tests/cpp/index_check_kat.hip."""
    report, ids, offsets = M.check(np.array([10, 11, 4, 5, -1, 6, 7, 0, np.iinfo(np.int32).min, 3], dtype=np.int32),
                                   np.array([0, 2, 2, 5, 4, 9, 12], dtype=np.int32), (11, 5, 7), 2)
    assert report.tolist() == [5, 1, 2, 4]
    assert ids.tolist() == [10, 0, 4, 0, 0, 6, 0, 0, 0, 3] and ids.dtype == np.int32
    assert offsets.tolist() == [0, 2, 2, 5, 5, 9, 10] and offsets.dtype == np.int32
    report, ids, none = M.check(np.array([0, 7, 6, -5, np.iinfo(np.int64).max, 1]), None, (7,), 3, num_hots=2)
    assert report.tolist() == [3, 1, 0, -1] and ids.tolist() == [0, 0, 6, 0, 0, 1] and none is None
