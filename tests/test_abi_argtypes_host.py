"""The ctypes binding against the header, parameter by parameter: a c_int argtype on an int64_t parameter truncates a
row count or a row id silently -- the host-side twin of a 32-bit offset in a kernel.  include/cuembed_amd.h is
preprocessed and its prototypes parsed; cuembed_amd/_lib.py's _declare() runs on a recorder (no library is loaded).

    every generic entry point of the header is bound, and nothing else is;
    the type-suffixed instantiations (cuembed_embedding_forward_f32_i32_o32, ...: the C caller's entry points, whose
        arguments the C compiler checks) are exactly the declared names that are not bound;
    argtypes has one entry per parameter, of the parameter's class: a pointer (c_void_p, or POINTER of the pointee's
        type), int, int64_t, uint32_t / unsigned, uint64_t / size_t, float, double; restype likewise.
"""
import ctypes
import functools
import os
import re
import subprocess
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cuembed_amd.h")
TYPED = re.compile(r"_(f32|f16|bf16|i32|i64|o32|o64)$")

#: C scalar type -> the ctypes classes that pass it unchanged (LP64: size_t and uint64_t are one class)
SCALARS = {
    "int": (ctypes.c_int,), "int32_t": (ctypes.c_int, ctypes.c_int32), "int64_t": (ctypes.c_int64,),
    "unsigned": (ctypes.c_uint, ctypes.c_uint32), "unsigned int": (ctypes.c_uint, ctypes.c_uint32),
    "uint32_t": (ctypes.c_uint, ctypes.c_uint32), "uint64_t": (ctypes.c_uint64,), "size_t": (ctypes.c_size_t,),
    "uint16_t": (ctypes.c_uint16,), "float": (ctypes.c_float,), "double": (ctypes.c_double,),
}


@functools.lru_cache(maxsize=None)
def prototypes():
    """{name: (return type, [parameter type, ...])} of the preprocessed header, types as normalised C text."""
    pre = subprocess.run(["gcc", "-E", "-P", HEADER], check=True, stdout=subprocess.PIPE, text=True).stdout
    pre = re.sub(r"\s+", " ", pre)
    found = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w \*]*?)\b(cuembed_[a-z0-9_]+) ?\(([^()]*)\) ?;", pre):
        params = params.strip()
        kinds = [] if params in ("", "void") else [_type_of(p) for p in params.split(",")]
        assert name not in found, name
        found[name] = (_normalise(ret), kinds)
    return found


def _normalise(text):
    text = re.sub(r"\bconst\b", " ", text).replace("*", " * ")
    return " ".join(text.split()).replace(" *", "*")


def _type_of(param):
    """A parameter's type without its name: 'const int64_t* ids' -> 'int64_t*', 'unsigned threshold' -> 'unsigned'."""
    text = _normalise(param)
    m = re.match(r"^(.*?[\w\*])\s+(\w+)$", text)
    if m and (m.group(1).rstrip("*").strip() in SCALARS or m.group(1).rstrip("* ").strip() in
              ("void", "char", "cuembed_stream_t")):
        text = m.group(1)
    return text.replace(" *", "*")


@functools.lru_cache(maxsize=None)
def bound():
    """{name: (restype, argtypes)} as _declare() sets them."""
    from cuembed_amd import _lib

    class Recorder:
        def __init__(self):
            self.functions = {}

        def __getattr__(self, name):
            if name.startswith("cuembed_"):
                return self.functions.setdefault(name, types.SimpleNamespace())
            raise AttributeError(name)

    rec = Recorder()
    _lib._declare(rec)
    return {n: (getattr(f, "restype", "unset"), getattr(f, "argtypes", "unset")) for n, f in rec.functions.items()}


def matches(c_type, ctype):
    """Whether a ctypes class passes a value of the C type unchanged."""
    if c_type == "cuembed_stream_t" or c_type.endswith("*"):
        if c_type == "char*" and ctype is ctypes.c_char_p:
            return True
        if ctype is ctypes.c_void_p:
            return True
        pointee = c_type[:-1]
        return (pointee in SCALARS and isinstance(ctype, type) and issubclass(ctype, ctypes._Pointer) and
                ctype._type_ in SCALARS[pointee])
    return c_type in SCALARS and ctype in SCALARS[c_type]


def test_the_parser_reads_the_header():
    protos = prototypes()
    assert len(protos) >= 95
    assert protos["cuembed_peek_last_error"] == ("int", [])
    assert protos["cuembed_version"] == ("char*", [])
    ret, params = protos["cuembed_translate_indices_for_row_cache"]
    assert ret == "void" and params.count("int64_t") == 3 and params[-1] == "cuembed_stream_t"
    assert protos["cuembed_transpose_sample_block_length"] == ("int64_t", ["int64_t", "int"])
    known = set(SCALARS) | {"cuembed_stream_t"}
    for name, (ret, params) in protos.items():
        assert ret in ("void", "char*") or ret in SCALARS, (name, ret)
        for p in params:
            assert p in known or (p.endswith("*") and (p.rstrip("*") in known or p.rstrip("*") in ("void", "char"))), (name, p)
    # the classes are distinct where it matters: an int is not an int64_t, a float not a double
    assert not matches("int64_t", ctypes.c_int) and not matches("int", ctypes.c_int64)
    assert not matches("double", ctypes.c_float) and not matches("uint64_t", ctypes.c_uint)
    assert not matches("int64_t*", ctypes.POINTER(ctypes.c_int)) and matches("size_t*", ctypes.POINTER(ctypes.c_size_t))


def test_bound_and_declared_functions_are_the_same_set():
    protos, binding = prototypes(), bound()
    typed = {n for n in protos if TYPED.search(n)}
    generic = set(protos) - typed
    assert len(typed) >= 34 and len(generic) >= 61
    assert sorted(set(binding) - set(protos)) == [], "bound, but not declared in the header"
    assert sorted(generic - set(binding)) == [], "declared in the header, but not bound"
    assert sorted(typed & set(binding)) == []


@pytest.mark.parametrize("name", sorted(n for n in prototypes() if not TYPED.search(n)))
def test_argtypes_match_the_prototype(name):
    ret, params = prototypes()[name]
    restype, argtypes = bound()[name]
    assert restype != "unset" and argtypes != "unset", "restype and argtypes must both be set"
    if ret == "void":
        assert restype is None
    elif ret == "char*":
        assert restype is ctypes.c_char_p
    else:
        assert matches(ret, restype), (ret, restype)
    assert len(argtypes) == len(params), (len(argtypes), params)
    for k, (c_type, ctype) in enumerate(zip(params, argtypes)):
        assert matches(c_type, ctype), "parameter %d: %s is bound as %s" % (k, c_type, getattr(ctype, "__name__", ctype))
