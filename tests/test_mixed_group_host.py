"""The mixed-width grouped forward without a GPU: MixedTableGroup on CPU tensors (column bases, D, lane bytes and its
refusals), the descriptor and the launch shape against a Python recomputation of the same arithmetic, every refusal of a
call raised before any launch (the tensors here live on the CPU: a call that got as far as the device check raises
RuntimeError "no CPU fallback"), and the names at every layer."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = (5000, 17, 300, 64)
DTYPES = (torch.float32, torch.float16, torch.bfloat16)
GROUPS = [(128, 16, 64, 32), (36, 4, 128), (6, 2, 10), (512, 8), (514, 4), (36, 36, 36), (128,)]
BATCHES = (0, 1, 5, 1023)
BLOCK = 256


@pytest.fixture(scope="module")
def ce():
    import cuembed_amd
    return cuembed_amd


def cpu_tables(widths, dtype=torch.float32):
    return [torch.zeros(ROWS[t], w, dtype=dtype) for t, w in enumerate(widths)]


def lane_bytes_model(widths, itemsize, pointer_bits=0):
    """The widest of 16 / 8 / 4 that every pointer, D * itemsize, every column base and every row pitch allow."""
    bits, column = pointer_bits, 0
    for w in widths:
        column += w * itemsize
        bits |= (w * itemsize) | column
    return 16 if bits % 16 == 0 else (8 if bits % 8 == 0 else 4)


def descriptor_model(widths, itemsize, lane, batch):
    """(grid, words): per table (width, column base, lanes per bag, first workgroup); then (0, D, 0, grid)."""
    n = lane // itemsize
    words, column, blocks, most = [], 0, 0, 0
    for w in widths:
        lanes = min(w // n, BLOCK)
        bags = BLOCK // lanes
        words += [w, column, lanes, blocks]
        column += w
        blocks += -(-batch // bags)
        most = max(most, bags)
    return blocks, words + [0, column, 0, blocks], most


# ---- the group ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("widths", GROUPS, ids=lambda w: "w" + "_".join(map(str, w)))
def test_a_group_of_cpu_tensors_can_be_inspected(ce, widths):
    for dtype in DTYPES:
        if dtype != torch.float32 and (514 in widths):
            continue
        group = ce.MixedTableGroup(cpu_tables(widths, dtype))
        T = len(widths)
        assert group.num_tables == len(group) == T and group.widths == widths and group.dtype == dtype
        assert group.column_base == tuple(sum(widths[:t]) for t in range(T + 1))
        assert group.embedding_dim == sum(widths)
        assert group.row_counts == ROWS[:T] and group.row_base == tuple(sum(ROWS[:t]) for t in range(T + 1))
        assert group.row_base_device.tolist() == list(group.row_base)
        assert group.table_ptrs.tolist() == [t.data_ptr() for t in group.tables] == list(group.host_ptrs)
        bits = 0
        for p in group.host_ptrs:
            bits |= p
        assert group.lane_bytes() == lane_bytes_model(widths, dtype.itemsize, bits)
        for out_ptr in (0, 4096, 4096 + 8, 4096 + 4):
            assert group.lane_bytes(out_ptr) == lane_bytes_model(widths, dtype.itemsize, bits | out_ptr)
        with pytest.raises(ValueError, match="4-byte aligned"):
            group.lane_bytes(4096 + 2)


def test_lane_bytes_of_the_groups_on_aligned_buffers():
    """What the widths alone allow (the table in the GPU test's head)."""
    want = {((128, 16, 64, 32), 2): 16, ((36, 4, 128), 2): 8, ((36, 4, 128), 4): 16, ((6, 2, 10), 2): 4, ((6, 2, 10), 4): 8,
            ((512, 8), 2): 16, ((514, 4), 4): 8, ((36, 36, 36), 2): 8, ((36, 36, 36), 4): 16, ((128,), 2): 16}
    for (widths, itemsize), lane in want.items():
        assert lane_bytes_model(widths, itemsize) == lane, (widths, itemsize)


def test_what_a_group_refuses(ce):
    with pytest.raises(ValueError, match="at least one table"):
        ce.MixedTableGroup([])
    with pytest.raises(TypeError, match="torch.Tensor"):
        ce.MixedTableGroup([torch.zeros(3, 4), "table"])
    with pytest.raises(TypeError, match="one dtype per group"):
        ce.MixedTableGroup([torch.zeros(3, 4), torch.zeros(3, 8, dtype=torch.float16)])
    with pytest.raises(TypeError, match="float32, float16 or bfloat16"):
        ce.MixedTableGroup([torch.zeros(3, 16, dtype=torch.uint8)])
    with pytest.raises(ValueError, match="one device per group"):
        ce.MixedTableGroup([torch.zeros(3, 4), torch.zeros(3, 8, device="meta")])
    with pytest.raises(ValueError, match="must be contiguous"):
        ce.MixedTableGroup([torch.zeros(3, 4), torch.zeros(3, 16)[:, ::2]])
    with pytest.raises(ValueError, match="multiple of 4 bytes"):
        ce.MixedTableGroup([torch.zeros(3, 4, dtype=torch.float16), torch.zeros(3, 3, dtype=torch.float16)])
    with pytest.raises(ValueError, match=r"\[rows, width\]"):
        ce.MixedTableGroup([torch.zeros(3, 4, 2)])
    # the same-width group keeps its error
    with pytest.raises(ValueError, match="one width per group"):
        ce.TableGroup([torch.zeros(3, 4), torch.zeros(3, 8)])


# ---- the descriptor and the launch shape ---------------------------------------------------------------------------------

@pytest.mark.parametrize("widths", GROUPS, ids=lambda w: "w" + "_".join(map(str, w)))
def test_descriptor_and_launch_shape_are_the_documented_arithmetic(ce, widths):
    L = ce._lib.lib()
    T = len(widths)
    assert L.cuembed_mixed_group_descriptor_bytes(T) == 16 * (T + 1)
    for dtype in DTYPES:
        itemsize = dtype.itemsize
        if any((w * itemsize) % 4 for w in widths) or (itemsize == 2 and 514 in widths):
            continue
        group = ce.MixedTableGroup(cpu_tables(widths, dtype))
        aligned = lane_bytes_model(widths, itemsize)
        for batch in BATCHES:
            for lane in (16, 8, 4):
                if lane > aligned:
                    continue
                grid, words, most = descriptor_model(widths, itemsize, lane, batch)
                blob = (ctypes.c_int32 * (4 * (T + 1)))(*([-1] * (4 * (T + 1))))
                got = L.cuembed_fill_mixed_group_descriptor((ctypes.c_int * T)(*widths), T, itemsize, lane, batch, BLOCK,
                                                            blob)
                assert (got, list(blob)) == (grid, words), (dtype, batch, lane)
                if lane <= group.lane_bytes():
                    assert group.descriptor_words(batch, lane) == (grid, words)
                # the launch shape for pointers that allow exactly `lane` bytes
                for hot, index_dtype, weighted in ((0, torch.int32, False), (7, torch.int32, True), (26, torch.int64, False)):
                    shape = ce.mixed_group_launch_shape(dtype, index_dtype, widths, batch, hot, weighted,
                                                        pointer_bits=0 if lane == 16 else 4096 + lane)
                    stage = most * hot * (index_dtype.itemsize + (itemsize if weighted else 0))
                    staged = hot > 0 and stage <= 16 * 1024
                    assert shape == dict(elems_per_lane=lane // itemsize, block_threads=BLOCK, grid=grid,
                                         embedding_dim=sum(widths), lds_bytes=stage if staged else 0, staged=staged,
                                         max_bags_per_block=most), (dtype, batch, lane, hot)


def test_the_wide_row_takes_the_whole_block_and_a_second_pass(ce):
    """fp32 W = 514 at 8-byte lanes: 257 row lanes, 256 lanes per bag (the column loop), one bag per workgroup."""
    grid, words = ce.MixedTableGroup(cpu_tables((514, 4))).descriptor_words(1023, 8)
    assert words[:8] == [514, 0, 256, 0, 4, 514, 2, 1023] and grid == 1023 + -(-1023 // 128)


def test_launch_shape_refuses_nonsense(ce):
    with pytest.raises(TypeError):
        ce.mixed_group_launch_shape(torch.int8, torch.int32, (4,), 1)
    with pytest.raises(TypeError):
        ce.mixed_group_launch_shape(torch.float32, torch.float32, (4,), 1)
    for widths, batch in (((), 1), ((3,), -1), ((0,), 1), ((4,), 2 ** 31)):
        with pytest.raises(ValueError):
            ce.mixed_group_launch_shape(torch.float32, torch.int32, widths, batch)
    with pytest.raises(ValueError):
        ce.mixed_group_launch_shape(torch.float16, torch.int32, (3,), 1)
    with pytest.raises(ValueError):
        ce.mixed_group_launch_shape(torch.float32, torch.int32, (4,), 1, pointer_bits=2)


# ---- the call's refusals, all before any launch -----------------------------------------------------------------------------

def test_every_refusal_precedes_the_launch(ce):
    widths, batch = (36, 4, 128), 2
    group = ce.MixedTableGroup(cpu_tables(widths))
    idx = torch.zeros(6, dtype=torch.int64)
    off = torch.zeros(3 * batch + 1, dtype=torch.int64)
    call = ce.embedding_forward_mixed_group
    with pytest.raises(ValueError, match="no concat and no max"):
        call(group, idx, off, mode="concat")
    with pytest.raises(ValueError, match="no concat and no max"):
        call(group, idx, off, mode="max")
    with pytest.raises(ValueError, match="row_loads"):
        call(group, idx, off, row_loads="nt")
    with pytest.raises(ValueError, match="row_loads_device is not taken"):
        call(group, idx, off, row_loads_device=torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match="sample_order is not taken"):
        call(group, idx, off, sample_order=torch.zeros(6, dtype=torch.int32))
    with pytest.raises(TypeError, match="indices must be a torch.Tensor"):
        call(group, [0, 1], off)
    with pytest.raises(TypeError, match="int32 or int64"):
        call(group, idx.float(), off)
    with pytest.raises(ValueError, match="either CSR"):
        call(group, idx, off, num_hots=2)
    with pytest.raises(ValueError, match="either CSR"):
        call(group, idx)
    with pytest.raises(ValueError, match="num_tables \\* batch_size \\+ 1"):
        call(group, idx, off[:-1])
    with pytest.raises(ValueError, match="num_tables \\* batch_size \\* num_hots"):
        call(group, idx, num_hots=4, batch_size=1)
    with pytest.raises(TypeError, match="weights must be torch.float32"):
        call(group, idx, off, weights=torch.zeros(6, dtype=torch.float16))
    with pytest.raises(ValueError, match="one entry per index"):
        call(group, idx, off, weights=torch.zeros(5))
    with pytest.raises(ValueError, match=r"out must be a contiguous torch.float32 tensor \[batch_size, embedding_dim\]"):
        call(group, idx, off, out=torch.zeros(batch, 3, 168))                  # the same-width group's shape
    with pytest.raises(ValueError, match="out must be"):
        call(group, idx, off, out=torch.zeros(batch, 168, dtype=torch.float16))
    needs_grad = ce.MixedTableGroup([t.requires_grad_(True) for t in cpu_tables(widths)])
    with pytest.raises(RuntimeError, match="requires grad"):
        call(needs_grad, idx, off)
    with pytest.raises(RuntimeError, match="weights require grad"):
        call(group, idx, off, weights=torch.zeros(6, requires_grad=True))
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):
        call(needs_grad, idx, off)
    # a call in order gets as far as the device check -- CSR, fixed hotness, and through the module
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        call(group, idx, off, weights=torch.zeros(6), mode="mean", row_loads="streaming", out=torch.zeros(batch, 168))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        call(group, idx, num_hots=1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ce.MixedEmbeddingBagGroup(group)(idx.view(3, 2, 1))


def test_the_module_and_the_index_check_take_a_mixed_group(ce):
    tables = cpu_tables((36, 4, 128))
    for mode in (None, "raise", "repair"):
        bags = ce.MixedEmbeddingBagGroup(tables, mode="mean", bounds_check=mode)
        assert bags.bounds_check == mode and bags.last_check is None and bags.embedding_dim == 168 and bags.num_tables == 3
    with pytest.raises(ValueError, match="bounds_check"):
        ce.MixedEmbeddingBagGroup(tables, bounds_check="clamp")
    with pytest.raises(ValueError, match="mode"):
        ce.MixedEmbeddingBagGroup(tables, mode="concat")
    # check_indices gets as far as the device check with a mixed group, and a TableGroup is treated as before
    idx, off = torch.zeros(6, dtype=torch.int64), torch.zeros(7, dtype=torch.int32)
    for group in (ce.MixedTableGroup(tables), ce.TableGroup([torch.zeros(n, 4) for n in ROWS[:3]])):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ce.check_indices(idx, off, group=group)
    with pytest.raises(ValueError, match="one width per group"):
        ce.check_indices(idx, off, group=tables)        # a plain list is still a same-width group


# ---- the names ---------------------------------------------------------------------------------------------------------

def test_the_names_exist_at_every_layer(ce):
    include = os.path.join(ROOT, "cuembed_amd", "csrc", "cuembed", "include")
    with open(os.path.join(include, "mixed_group_lookup.hpp")) as f:
        host = f.read()
    assert re.search(r"template <typename InputT, typename OutputT, typename IndexT, typename OffsetT>\s*"
                     r"void EmbeddingForwardMixedGroup\(", host)
    for name in ("MixedGroupDescriptorBytes", "FillMixedGroupDescriptor"):
        assert re.search(r"inline \w+ %s\(" % name, host), name
    assert os.path.exists(os.path.join(include, "mixed_group_gather_kernels.hpp"))
    pre = subprocess.run(["gcc", "-std=c99", "-E", "-P", "-x", "c", os.path.join(ROOT, "include", "cuembed_amd.h")],
                         check=True, stdout=subprocess.PIPE, text=True).stdout
    counts = {"cuembed_embedding_forward_mixed_group": 17, "cuembed_mixed_group_descriptor_bytes": 1,
              "cuembed_fill_mixed_group_descriptor": 7, "cuembed_mixed_group_launch_shape": 9}
    from cuembed_amd import build
    assert "c_api_mixed_group.hip" in build.UNITS and callable(build.build_mixed_group_test)
    L = ctypes.CDLL(build.build())
    declared = ce._lib.lib()
    for name, args in counts.items():
        proto = re.search(r"\b%s\s*\(([^)]*)\)" % name, pre)
        assert proto, name + " is declared in plain C"
        assert len(proto.group(1).split(",")) == args, name
        assert hasattr(L, name), name + " is exported"
        assert len(getattr(declared, name).argtypes) == args, name + " has its argtypes"
    vp, i = ctypes.c_void_p, ctypes.c_int
    assert list(declared.cuembed_embedding_forward_mixed_group.argtypes) == [vp, vp, vp, vp, i, i, vp, i, vp, i, vp, i, i, i,
                                                                             vp, i, vp]
    assert declared.cuembed_embedding_forward_mixed_group.restype is None
    assert declared.cuembed_mixed_group_descriptor_bytes.restype is ctypes.c_size_t
    assert declared.cuembed_fill_mixed_group_descriptor.restype is i
    with open(os.path.join(ROOT, "CMakeLists.txt")) as f:
        assert "c_api_mixed_group.hip" in f.read()
    from cuembed_amd import cuembed_pyt  # noqa: F401  (loads the ops)
    schema = str(torch.ops.cuembed_pyt.cuemb_embedding_mixed_group.default._schema)
    assert schema.endswith("-> Tensor") and "Tensor descriptor" in schema and "int lane_bytes" in schema
    assert "sample_order" not in schema
    for name in ("MixedTableGroup", "MixedEmbeddingBagGroup", "embedding_forward_mixed_group", "mixed_group_launch_shape"):
        assert callable(getattr(ce, name)), name


def test_the_python_backend_defines_the_same_op():
    """CUEMBED_PYT_BACKEND=python registers the op from Python (a fresh process: the backend is chosen at import)."""
    import sys
    from cuembed_amd import cuembed_pyt  # noqa: F401
    native = str(torch.ops.cuembed_pyt.cuemb_embedding_mixed_group.default._schema)
    code = ("import sys, torch\nsys.path.insert(0, %r)\nfrom cuembed_amd import cuembed_pyt as P\n"
            "assert P.BACKEND == 'python'\nprint(torch.ops.cuembed_pyt.cuemb_embedding_mixed_group.default._schema)\n" % ROOT)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, CUEMBED_PYT_BACKEND="python"),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == native, r.stdout


def test_the_c_abi_aborts_on_misuse_before_any_launch():
    """CUEMBED_ASSERT: message on stderr + abort, in a child process.  The pointers are never dereferenced (256 is no
    address of anything): a sample order does not exist in this ABI, and a width that no lane divides, a descriptor that
    is missing and a CSR call with a hotness are refused before any launch."""
    import sys
    calls = {
        "row bytes": "L.cuembed_fill_mixed_group_descriptor((ctypes.c_int*1)(3), 1, 2, 4, 5, 256, (ctypes.c_int*8)())",
        "lane too wide": "L.cuembed_fill_mixed_group_descriptor((ctypes.c_int*2)(4, 2), 2, 4, 16, 5, 256, (ctypes.c_int*12)())",
        "no descriptor": "L.cuembed_embedding_forward_mixed_group(P, P, (ctypes.c_int*1)(4), None, 1, 0, 256, 0, 256, 0, None, "
                         "5, 0, 0, 256, -1, None)",
        "csr and hotness": "L.cuembed_embedding_forward_mixed_group(P, P, (ctypes.c_int*1)(4), 256, 1, 0, 256, 0, 256, 0, None, "
                           "5, 3, 0, 256, -1, None)",
        "concat": "L.cuembed_embedding_forward_mixed_group(P, P, (ctypes.c_int*1)(4), 256, 1, 0, 256, 0, 256, 0, None, "
                  "5, 0, 2, 256, -1, None)",
    }
    for name, call in calls.items():
        code = ("import ctypes\nfrom cuembed_amd import _lib\nL=_lib.lib()\nP=(ctypes.c_void_p*1)(256)\n" + call +
                "\nprint('returned')\n")
        r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           text=True, timeout=120)
        assert r.returncode != 0 and "returned" not in r.stdout and "Check failed" in r.stdout, (name, r.stdout)
