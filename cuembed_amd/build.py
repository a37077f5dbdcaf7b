"""Builds libcuembed_amd.so (HIP kernels + C ABI) for gfx950 with hipcc.

    python -m cuembed_amd.build [--force]

The translation units (UNITS) are compiled in parallel and linked into
cuembed_amd/lib/libcuembed_amd.so (in-tree, so the file travels with the repo
snapshot to the GPU box).  hipcc cross-compiles without a GPU present.
"""
import hashlib
import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG)
CSRC = os.path.join(PKG, "csrc")
LIB_DIR = os.path.join(PKG, "lib")
LIB_PATH = os.path.join(LIB_DIR, "libcuembed_amd.so")
HARNESS_PATH = os.path.join(LIB_DIR, "libcuembed_harness.so")
OBJ_DIR = os.path.join(PKG, "build")
UNITS = ["c_api_forward.hip", "c_api_backward.hip", "c_api_transforms.hip", "c_api_exchange.hip",
         "c_api_optimizer.hip", "c_api_optimizer_stochastic.hip", "c_api_optimizer_adam.hip",
         "c_api_optimizer_adam_stochastic.hip", "c_api_optimizer_placed_stochastic.hip",
         "c_api_optimizer_adam_placed_stochastic.hip", "c_api_quantized.hip", "c_api_grouped.hip",
         "c_api_grouped_backward.hip", "c_api_row_cache.hip", "c_api_optimizer_grouped.hip",
         "c_api_optimizer_grouped_stochastic.hip", "c_api_index_check.hip", "c_api_mixed_group.hip",
         "c_api_mixed_group_backward.hip"]
ARCH = "gfx950"

HIPCC_FLAGS = [
    "--offload-arch=" + ARCH, "-O3", "-std=c++17", "-fPIC",
    # float atomics as hardware instructions (global_atomic_add_f32 / pk_add_f16)
    "-munsafe-fp-atomics",
    "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
] + os.environ.get("CUEMBED_HIPCC_EXTRA", "").split()   # experiments only (e.g. -DCUEMBED_TUNE_...): part of the build key


def _hipcc():
    exe = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(exe):
        raise RuntimeError("hipcc not found; a ROCm toolchain is required to build cuembed_amd")
    return exe


def _digest_files(paths, extra=""):
    h = hashlib.sha256()
    h.update(extra.encode())
    for p in sorted(set(paths)):
        if os.path.exists(p):
            with open(p, "rb") as fh:
                h.update(os.path.relpath(p, ROOT).encode())
                h.update(fh.read())
        else:
            h.update(("missing:" + os.path.relpath(p, ROOT)).encode())
    return h.hexdigest()


def _deps_of(obj):
    """Dependencies recorded by the last compile of `obj` (hipcc -MD), repo files only."""
    dep = obj[:-2] + ".d"
    if not os.path.exists(dep):
        return None
    with open(dep) as f:
        txt = f.read().replace("\\\n", " ")
    files = txt.split(":", 1)[1].split() if ":" in txt else []
    out = []
    for x in files:  # keep repo files only, re-rooted (the tree may have moved since the compile)
        for marker in ("/cuembed_amd/csrc/", "/include/cuembed_amd.h"):
            k = x.find(marker)
            if k >= 0:
                out.append(os.path.join(ROOT, x[k + 1:]))
                break
    return out


def build(force=False, verbose=False):
    """Compile what changed (per translation unit, by content hash of the unit and the repo
    headers it includes).  Returns the path of the shared library."""
    os.makedirs(LIB_DIR, exist_ok=True)
    os.makedirs(OBJ_DIR, exist_ok=True)
    hipcc = _hipcc()
    flags_key = " ".join(HIPCC_FLAGS).replace(ROOT, "<root>")

    def unit_state(unit):
        obj = os.path.join(OBJ_DIR, unit.replace(".hip", ".o"))
        stamp = obj[:-2] + ".stamp"
        deps = _deps_of(obj)
        fresh = False
        if not force and deps is not None and os.path.exists(obj) and os.path.exists(stamp):
            with open(stamp) as f:
                fresh = f.read().strip() == _digest_files(deps, flags_key)
        return obj, stamp, fresh

    def compile_one(unit):
        obj, stamp, fresh = unit_state(unit)
        if fresh:
            return obj, False
        cmd = [hipcc] + HIPCC_FLAGS + ["-MD", "-MF", obj[:-2] + ".d", "-c", os.path.join(CSRC, unit),
                                       "-o", obj]
        if verbose:
            print(" ".join(cmd), flush=True)
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed for %s:\n%s" % (unit, r.stdout))
        with open(stamp, "w") as f:
            f.write(_digest_files(_deps_of(obj) or [os.path.join(CSRC, unit)], flags_key))
        return obj, True

    harness_srcs = [os.path.join(CSRC, "utils", "synthetic_inputs.cpp"),
                    os.path.join(CSRC, "utils", "datagen.hpp")]
    harness_stamp = os.path.join(LIB_DIR, "libcuembed_harness.stamp")

    def compile_harness(_):
        # host-only synthetic-workload generator (libstdc++ <random>), plain g++
        digest = _digest_files(harness_srcs)
        if not force and os.path.exists(HARNESS_PATH) and os.path.exists(harness_stamp):
            with open(harness_stamp) as f:
                if f.read().strip() == digest:
                    return None
        cmd = [shutil.which("g++") or "g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I" + CSRC,
               harness_srcs[0], "-o", HARNESS_PATH]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            raise RuntimeError("g++ failed for the harness library:\n" + r.stdout)
        with open(harness_stamp, "w") as f:
            f.write(digest)
        return None

    with ThreadPoolExecutor(max_workers=len(UNITS) + 1) as ex:
        harness_job = ex.submit(compile_harness, None)
        results = list(ex.map(compile_one, UNITS))
        harness_job.result()
    objs = [o for o, _ in results]
    if any(changed for _, changed in results) or not os.path.exists(LIB_PATH):
        cmd = [hipcc, "--offload-arch=" + ARCH, "-shared", "-fPIC", "-o", LIB_PATH] + objs
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            raise RuntimeError("link failed:\n" + r.stdout)
    build_torch_binding(force=force)
    return LIB_PATH


TORCH_BINDING_PATH = os.path.join(LIB_DIR, "libcuembed_pyt.so")


def build_torch_binding(force=False):
    """Compiles cuembed_amd/csrc/torch_binding.cpp (TORCH_LIBRARY / TORCH_LIBRARY_IMPL, no device code) with
    the host compiler against the installed torch and links it to libcuembed_amd.so.  Needs build() first."""
    import torch
    from torch.utils import cpp_extension
    src = os.path.join(CSRC, "torch_binding.cpp")
    stamp = os.path.join(LIB_DIR, "libcuembed_pyt.stamp")
    digest = _digest_files([src, os.path.join(ROOT, "include", "cuembed_amd.h")], torch.__version__)
    if not force and os.path.exists(TORCH_BINDING_PATH) and os.path.exists(stamp):
        with open(stamp) as f:
            if f.read().strip() == digest:
                return TORCH_BINDING_PATH
    torch_lib = cpp_extension.library_paths()[0]
    cmd = [shutil.which("g++") or "g++", "-O2", "-std=c++17", "-fPIC", "-shared",
           "-D__HIP_PLATFORM_AMD__=1", "-DUSE_ROCM=1",      # what torch's own headers key on under ROCm
           "-D_GLIBCXX_USE_CXX11_ABI=%d" % int(torch._C._GLIBCXX_USE_CXX11_ABI)]
    cmd += ["-I" + p for p in cpp_extension.include_paths()] + ["-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include")]
    cmd += [src, "-o", TORCH_BINDING_PATH, "-L" + torch_lib, "-ltorch", "-ltorch_cpu", "-lc10", "-lc10_hip",
            "-ltorch_hip", "-L" + LIB_DIR, "-lcuembed_amd", "-Wl,-rpath,$ORIGIN", "-Wl,-rpath," + torch_lib]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError("g++ failed for the torch binding:\n" + r.stdout)
    with open(stamp, "w") as f:
        f.write(digest)
    return TORCH_BINDING_PATH


def _build_program(what, flags, force, error_name=None, extra_srcs=(), extra_deps=(), link=()):
    """Compiles one stand-alone program against the header-only API: the .hip file `what` (a path under ROOT) and
    `extra_srcs` with `flags`, to the executable of the same name without the suffix, unless the stamp next to it holds
    the digest of the sources, `extra_deps` and every header of the header-only API.  `error_name` names the program in
    the error message, where its path does not.  Returns the path of the executable."""
    src = os.path.join(ROOT, what)
    exe = src[:-len(".hip")]
    stamp = exe + ".stamp"
    deps = [src] + list(extra_srcs) + list(extra_deps)
    for dirpath, _, files in os.walk(os.path.join(CSRC, "cuembed", "include")):
        deps += [os.path.join(dirpath, f) for f in files]
    digest = _digest_files(deps)
    if not force and os.path.exists(exe) and os.path.exists(stamp):
        with open(stamp) as f:
            if f.read().strip() == digest:
                return exe
    cmd = [_hipcc(), "--offload-arch=" + ARCH] + flags + ["-I" + CSRC, src] + list(extra_srcs) + list(link) + ["-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed for %s:\n" % (error_name or what) + r.stdout)
    with open(stamp, "w") as f:
        f.write(digest)
    return exe


_O2 = ["-O2", "-std=c++17"]
_O2_ATOMICS = _O2 + ["-munsafe-fp-atomics"]      # float atomics as hardware instructions, as in the library


def build_header_api_test(force=False):
    """Compiles tests/cpp/header_api_kat.hip against the header-only API (the C++ side of the
    drop-in boundary).  Returns the path of the executable."""
    return _build_program("tests/cpp/header_api_kat.hip", _O2_ATOMICS, force, error_name="the header-only API test")


def build_sparse_update_test(force=False):
    """Compiles tests/cpp/sparse_update_kat.hip: cuembed::SparseRowUpdate through the header-only API against a host
    recomputation on exactly representable data.  Needs a GPU to RUN (tests/test_gpu_cpp_sparse_update.py)."""
    return _build_program("tests/cpp/sparse_update_kat.hip", _O2, force)


def build_stochastic_rounding_test(force=False):
    """Compiles tests/cpp/stochastic_rounding_kat.hip: cuembed::SparseRowUpdate with stochastic rounding through the
    header-only API against a host recomputation with the same rounding functions.  Needs a GPU to RUN
    (tests/test_gpu_cpp_stochastic_rounding.py)."""
    return _build_program("tests/cpp/stochastic_rounding_kat.hip", _O2, force)


def build_sparse_adam_test(force=False):
    """Compiles tests/cpp/sparse_adam_kat.hip: cuembed::SparseRowAdam and cuembed::AdamClockAdvance through the
    header-only API against expected values written in the source (exactly representable data).  Needs a GPU to RUN
    (tests/test_gpu_cpp_sparse_adam.py)."""
    return _build_program("tests/cpp/sparse_adam_kat.hip", _O2, force)


def build_row_cache_state_test(force=False):
    """Compiles tests/cpp/row_cache_state_kat.hip: cuembed::RowCachePrefetch / RowCacheFlush with a state plane and
    cuembed::SparseRowUpdate with state_ids through the header-only API against a host recomputation on exactly
    representable data.  Needs a GPU to RUN (tests/test_gpu_cpp_row_cache_state.py)."""
    return _build_program("tests/cpp/row_cache_state_kat.hip", _O2_ATOMICS, force)


def build_row_cache_adam_test(force=False):
    """Compiles tests/cpp/row_cache_adam_kat.hip: cuembed::RowCachePrefetch / RowCacheFlush with two state planes,
    cuembed::TranslateIndicesForRowCachePlanes and cuembed::SparseRowAdam with placed moments through the header-only API
    against a host recomputation on exactly representable data.  Needs a GPU to RUN (tests/test_gpu_cpp_row_cache_adam.py)."""
    return _build_program("tests/cpp/row_cache_adam_kat.hip", _O2_ATOMICS, force)


def build_row_cache_stochastic_test(force=False):
    """Compiles tests/cpp/row_cache_stochastic_kat.hip: cuembed::RowCachePrefetch / RowCacheFlush with one and two state
    planes, cuembed::TranslateIndicesForRowCachePlanes and cuembed::SparseRowUpdate / SparseRowAdam with row_names
    (stochastic rounding behind the cache) through the header-only API against a host recomputation with
    stochastic_rounding.hpp's host functions.  Needs a GPU to RUN (tests/test_gpu_cpp_row_cache_stochastic.py)."""
    return _build_program("tests/cpp/row_cache_stochastic_kat.hip", _O2_ATOMICS, force)


def build_grouped_train_test(force=False):
    """Compiles tests/cpp/grouped_train_kat.hip: cuembed::EmbeddingWeightGradGrouped and cuembed::GroupedMeanScale through
    the header-only API on a three-table group against a host recomputation on exactly representable data.  Needs a GPU
    to RUN (tests/test_gpu_cpp_grouped_train.py)."""
    return _build_program("tests/cpp/grouped_train_kat.hip", _O2_ATOMICS, force)


def build_grouped_sparse_update_test(force=False):
    """Compiles tests/cpp/grouped_sparse_update_kat.hip: cuembed::SparseRowUpdateGrouped / SparseRowAdamGrouped through the
    header-only API on a three-table group against cuembed::SparseRowUpdate / SparseRowAdam per table, bit for bit, on
    hashed data.  Needs a GPU to RUN (tests/test_gpu_cpp_grouped_sparse_update.py)."""
    return _build_program("tests/cpp/grouped_sparse_update_kat.hip", _O2, force)


def build_grouped_stochastic_rounding_test(force=False):
    """Compiles tests/cpp/grouped_stochastic_rounding_kat.hip: cuembed::SparseRowUpdateGrouped / SparseRowAdamGrouped with
    stochastic rounding and one seed per table through the header-only API on a three-table group, against a host
    recomputation with stochastic_rounding.hpp's host functions on exactly representable data.  Needs a GPU to RUN
    (tests/test_gpu_cpp_grouped_stochastic_rounding.py)."""
    return _build_program("tests/cpp/grouped_stochastic_rounding_kat.hip", _O2, force)


def build_index_check_test(force=False):
    """Compiles tests/cpp/index_check_kat.hip: cuembed::CheckIndices through the header-only API on a small hand-written
    batch (a three-table CSR group and a fixed-hotness table) with the answers written in the source.  Needs a GPU to RUN
    (tests/test_gpu_cpp_index_check.py)."""
    return _build_program("tests/cpp/index_check_kat.hip", _O2, force)


def build_mixed_group_test(force=False):
    """Compiles tests/cpp/mixed_group_kat.hip: cuembed::EmbeddingForwardMixedGroup through the header-only API on a
    hand-written three-table group of widths 4, 8 and 2 (CSR with an empty bag, then fixed hotness) with the answers
    written in the source.  Needs a GPU to RUN (tests/test_gpu_cpp_mixed_group.py)."""
    return _build_program("tests/cpp/mixed_group_kat.hip", _O2, force)


def build_mixed_group_backward_test(force=False):
    """Compiles tests/cpp/mixed_group_backward_kat.hip: cuembed::GroupedBackwardKeys, cuembed::Transpose,
    cuembed::EmbeddingBackwardMixedGroup and cuembed::MixedGroupMeanScale through the header-only API on a hand-written
    three-table group of widths 4, 8 and 2 with the answers written in the source, sentinel-filled outputs and the
    capacity check.  Needs a GPU to RUN (tests/test_gpu_cpp_mixed_group_backward.py)."""
    return _build_program("tests/cpp/mixed_group_backward_kat.hip", _O2_ATOMICS, force)


def build_sort_unit_test(force=False):
    """Compiles tests/cpp/sort_route_unit.hip: host-side unit tests of the sort's integer building blocks (buffer
    routing, implicit payload division, tile maps, workspace plans).  The program makes no HIP call: it runs on the CPU."""
    return _build_program("tests/cpp/sort_route_unit.hip", ["-O1", "-std=c++17"], force)


def build_device_blocks_test(force=False):
    """Compiles tests/cpp/device_blocks_unit.hip: unit tests of the gather / scatter building blocks (addressing, column
    slices, Pack / Arith / RowPool, FinishPooledRow, the backward's RunSum, staging and chaining) instantiated in small kernels and compared with host
    recomputation, bit for bit.  Needs a GPU to RUN (tests/test_gpu_device_blocks.py)."""
    return _build_program("tests/cpp/device_blocks_unit.hip", ["-O3", "-std=c++17", "-munsafe-fp-atomics"], force)


def build_manual_benchmark(force=False):
    """Compiles benchmarks/manual_benchmark.hip (C++ harness on the header-only API)."""
    gen = os.path.join(CSRC, "utils", "synthetic_inputs.cpp")
    return _build_program("benchmarks/manual_benchmark.hip", ["-O3", "-std=c++17", "-munsafe-fp-atomics"], force,
                          extra_srcs=[gen], extra_deps=[os.path.join(CSRC, "utils", "datagen.hpp")],
                          link=["-ldl"])     # (-ldl: --check_result loads the CPU checker with dlopen)


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
