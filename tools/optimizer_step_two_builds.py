#!/usr/bin/env python3
"""Two builds of the library in ONE process on the SAME tensors, taking turns: the sparse optimizer step at C4 without
the between-process spread that a comparison of separate benchmark runs carries (docs/EXPERIMENTS.md, "One walk for the
five rules").  Each side swaps the loaded library under cuembed_amd.ops and makes the same call.

    python tools/optimizer_step_two_builds.py OTHER_LIBCUEMBED_AMD_SO [--out FILE]
"""
import json, os, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if len(sys.argv) < 2:
    sys.exit(__doc__)
sys.path.insert(0, ROOT)
import cuembed_amd as ce
from cuembed_amd import harness
import benchmarks.optimizer_step_benchmark as B
from tools import two_builds

LIBS = two_builds.load(sys.argv[1])     # "parent": the other build; "new": this tree's
ncat, W, H, batch = 10_000_000, 256, 64, 65536
dev = torch.device("cuda")
out = {"device": torch.cuda.get_device_name(0), "calls_per_round": 100, "rounds": 5, "sides": {}}
for dtype, rule, stochastic in ((torch.float32, "adagrad", False), (torch.float16, "adagrad", False),
                                (torch.bfloat16, "rowwise_adagrad", True), (torch.float16, "rowwise_adam", False),
                                (torch.float16, "adam", False)):
    table = torch.empty((ncat, W), dtype=dtype, device=dev).uniform_(-1, 1)
    idx = torch.from_numpy(harness.generate_indices(ncat, batch, H, alpha=1.15)).to(dev).view(batch, H)
    gy = (torch.rand((batch, W), device=dev) * 2 - 1).mul_(2.0 ** -6).to(dtype)
    t_idx, t_sid, _, remap = ce.transpose_fixed_hotness(idx, batch, H, num_categories=ncat, remapped=True)
    n = int(remap[-1].item()) + 1
    rows, ids = ce.embedding_backward(gy, n, t_idx, t_sid, remap)
    last_id = remap[-1:].clone()
    del t_idx, t_sid, remap, idx, gy
    kw = dict(stochastic_rounding=True, seed=5, step=1) if stochastic else {}
    if rule.endswith("adam"):
        m = torch.zeros((ncat, W), dtype=torch.float32, device=dev)
        v = torch.zeros((ncat,) if rule == "rowwise_adam" else (ncat, W), dtype=torch.float32, device=dev)
        call = lambda: ce.sparse_row_adam(table, ids, rows, exp_avg=m, exp_avg_sq=v, lr=1e-3, bias_factor=0.3,
                                          rowwise=rule == "rowwise_adam", last_id=last_id, **kw)
    else:
        state = torch.zeros((ncat, W) if rule == "adagrad" else (ncat,), dtype=torch.float32, device=dev)
        call = lambda: ce.sparse_row_update(table, ids, rows, rule=rule, lr=1e-3, state=state, last_id=last_id, **kw)

    got = two_builds.alternate(LIBS, call, 100, 5, 5)
    key = "C4 %s %s%s" % (str(dtype).replace("torch.", ""), rule, " stochastic" if stochastic else "")
    got["separable"] = B.faster(got["parent"], got["new"]) or B.faster(got["new"], got["parent"])
    out["sides"][key] = got
    print(key, {k: (round(s["ms"], 4), round(s["min"], 4), round(s["max"], 4)) for k, s in got.items() if k != "separable"},
          "separable" if got["separable"] else "within the spread", flush=True)
    del table, rows, ids, call
    if rule.endswith("adam"):
        del m, v
    else:
        del state
    torch.cuda.empty_cache()
if "--out" in sys.argv:
    with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
        json.dump(out, f, indent=1)
