"""Two builds of the library in ONE process on the SAME tensors, taking turns -- what the *_two_builds.py tools share.
Each side swaps the loaded library under cuembed_amd and makes the same call, so a comparison carries no
between-process spread.  A shape is accepted when the medians differ by no more than the larger of the two sides'
spreads (max - min over the rounds)."""
import ctypes
import os

import torch

from cuembed_amd import _lib
import benchmarks.quantized_forward_benchmark as B

CRITERION = "|median(new) - median(parent)| <= max(spread(new), spread(parent))"


def load(other_library):
    """{"parent": the other build, "new": this tree's}."""
    new = _lib.lib()
    par = ctypes.CDLL(os.path.abspath(other_library))
    _lib._declare(par)
    return {"parent": par, "new": new}


def side(libs, name, call):
    def fn():
        _lib._lib = libs[name]
        call()
    return fn


def alternate(libs, call, calls, rounds, warmup):
    got = B.alternate(torch, {name: side(libs, name, call) for name in libs}, calls, rounds, warmup)
    _lib._lib = libs["new"]
    return got


def compare(libs, shapes, key, call, result, calls=100, rounds=9, warmup=5, same_bits=True):
    """Times `call` on both builds into shapes[key].  `result`: the tensor (or tensors) the call writes; with
    same_bits the two builds must leave the same bits there."""
    results = result if isinstance(result, (list, tuple)) else [result]
    if same_bits:
        bits = {}
        for name in libs:
            side(libs, name, call)()
            bits[name] = [r.clone() for r in results]
        for p, n in zip(bits["parent"], bits["new"]):
            assert torch.equal(p.view(torch.uint8), n.view(torch.uint8)), key
    got = alternate(libs, call, calls, rounds, warmup)
    got["same_bits_asserted"] = bool(same_bits)
    got["difference_of_medians_ms"] = got["new"]["ms"] - got["parent"]["ms"]
    got["accepted"] = abs(got["difference_of_medians_ms"]) <= max(got["new"]["spread"], got["parent"]["spread"])
    shapes[key] = got
    print(key, {k: (round(s["ms"], 4), round(s["spread"], 4)) for k, s in got.items() if isinstance(s, dict)},
          "accepted" if got["accepted"] else "BEYOND THE SPREAD", flush=True)
    return got
