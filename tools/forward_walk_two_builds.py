#!/usr/bin/env python3
"""Two builds of the library in ONE process on the SAME tensors, taking turns: the plain and the quantized forward
without the between-process spread that a comparison of separate benchmark runs carries (the method of
tools/forward_bisect.py and tools/optimizer_step_two_builds.py; docs/EXPERIMENTS.md, "One sample walk for the plain
and the quantized forward").  Each side swaps the loaded library under cuembed_amd and makes the same call.  Shapes: C2
fp16 at alpha 1.15 and 0, the C3 CSR weighted fp32 shape of bench.py, the quantized C2 shape of
benchmarks/quantized_forward_benchmark.py.  A shape is accepted when the medians differ by no more than the larger of
the two sides' spreads (max - min over the rounds).

    python tools/forward_walk_two_builds.py OTHER_LIBCUEMBED_AMD_SO [--out FILE]
"""
import json, os, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if len(sys.argv) < 2:
    sys.exit(__doc__)
sys.path.insert(0, ROOT)
import cuembed_amd as ce
from cuembed_amd import harness
import bench
from tools import two_builds

LIBS = two_builds.load(sys.argv[1])     # "parent": the other build; "new": this tree's
CALLS, ROUNDS, WARMUP = 100, 9, 5
dev = torch.device("cuda")
out = {"tool": "tools/forward_walk_two_builds.py", "device": torch.cuda.get_device_name(0), "calls_per_round": CALLS,
       "rounds": ROUNDS, "criterion": two_builds.CRITERION, "shapes": {}}


def compare(key, call, result):
    two_builds.compare(LIBS, out["shapes"], key, call, result, CALLS, ROUNDS, WARMUP)


ncat, W, H, batch = 10_000_000, 256, 64, 65536
table = torch.empty((ncat, W), dtype=torch.float16, device=dev).uniform_(-1, 1)
y = torch.empty((batch, W), dtype=torch.float16, device=dev)
for alpha in (1.15, 0.0):
    idx = torch.from_numpy(harness.generate_indices(ncat, batch, H, alpha=alpha)).to(dev)
    compare("C2 fp16 alpha=%.2f" % alpha, lambda: ce.embedding_forward(table, idx, num_hots=H, out=y), y)
    if alpha == 1.15:
        q = ce.quantize_rows(table)
        compare("C2 quantized alpha=1.15", lambda: ce.embedding_forward_quantized(q, idx, num_hots=H, out=y), y)
        del q
del table, y, idx
torch.cuda.empty_cache()

cfg = dict(bench.WORKLOADS["c3"])
table = bench.fill_table(torch, cfg["rows"], cfg["width"], torch.float32, dev, seed=4321)
hb, _ = bench.make_batches(harness, np, cfg, cfg["alpha"], 1, 0, 1, np.int32, shared=False)
b = {k: (None if v is None else torch.from_numpy(v).to(dev)) for k, v in hb[0].items()}
y = torch.empty((cfg["batch"], cfg["width"]), dtype=torch.float32, device=dev)
compare("C3 fp32 weighted CSR", lambda: ce.embedding_forward(table, b["indices"], b["offsets"], b["weights"],
                                                             batch_size=cfg["batch"], num_hots=0, mode="sum", out=y), y)
if "--out" in sys.argv:
    with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
