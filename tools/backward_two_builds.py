#!/usr/bin/env python3
"""Two builds of the library in ONE process on the SAME tensors, taking turns: EmbeddingBackward without the
between-process spread that a comparison of separate benchmark runs carries (tools/two_builds.py has the method and
the acceptance rule; docs/EXPERIMENTS.md, "One LDS layout and named phases for the backward").  Shapes: the C4
compressed backward of bench.py in fp16 and fp32, the same on a sample-blocked order (uncoalesced and blocked-coalesced),
C4 weighted, uniform indices at W = 32, B = 131,072 (the window-of-8 path), reference_sums in fp16 at C4.  grad_y holds
-1, 0, 1 and the weights 0.5 / 0.25, so every sum is exact and the two builds must leave the same bits on every shape.

    python tools/backward_two_builds.py OTHER_LIBCUEMBED_AMD_SO [--out FILE]
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
from tools import two_builds

LIBS = two_builds.load(sys.argv[1])     # "parent": the other build; "new": this tree's
CALLS, ROUNDS, WARMUP = 50, 9, 5
dev = torch.device("cuda")
out = {"tool": "tools/backward_two_builds.py", "device": torch.cuda.get_device_name(0), "calls_per_round": CALLS,
       "rounds": ROUNDS, "criterion": two_builds.CRITERION, "shapes": {}}


def compare(key, call, grad, inverse, calls=CALLS):
    two_builds.compare(LIBS, out["shapes"], key, call, [grad, inverse], calls, ROUNDS, WARMUP)


def buffers(rows, W, dtype):
    return torch.empty((rows, W), dtype=dtype, device=dev), torch.empty((rows,), dtype=torch.int32, device=dev)


ncat, W, H, B = 10_000_000, 256, 64, 65536
idx = torch.from_numpy(harness.generate_indices(ncat, B, H, alpha=1.15, index=np.int32)).to(dev)
weights = torch.where(torch.randint(0, 2, (B * H,), device=dev) == 0, 0.5, 0.25)
t_idx, t_sid, t_w = ce.transpose_fixed_hotness(idx, B, H, weights.half(), num_categories=ncat)
remap = ce.compute_compressed_grad_indices(t_idx)
nu = int(remap[-1].item()) + 1
P = max(2, ce.recommended_sample_blocks(torch.float16, W, B, B * H))
b_idx, b_sid, _ = ce.transpose_fixed_hotness(idx, B, H, num_categories=ncat, sample_blocks=P)
pairs, table, _ = ce.compute_compressed_grad_indices_blocked(b_idx, P)
u_remap = ce.compute_compressed_grad_indices(b_idx)
nub = int(u_remap[-1].item()) + 1
for dtype in (torch.float16, torch.float32):
    name = str(dtype).replace("torch.", "")
    gy = torch.randint(-1, 2, (B, W), device=dev).to(dtype)
    g, i = buffers(nu, W, dtype)
    compare("C4 %s compressed" % name, lambda: ce.embedding_backward(gy, nu, t_idx, t_sid, remap, grad_embedding=g,
                                                                     inverse_mapping=i), g, i)
    compare("C4 %s sample blocks %d, blocked-coalesced" % (name, P), lambda: ce.embedding_backward(
        gy, nu, b_idx, b_sid, pairs, grad_embedding=g, inverse_mapping=i, sample_blocks=P, block_row_ids=table), g, i)
    gu, iu = buffers(nub, W, dtype)
    compare("C4 %s sample blocks %d, uncoalesced" % (name, P), lambda: ce.embedding_backward(
        gy, nub, b_idx, b_sid, u_remap, grad_embedding=gu, inverse_mapping=iu), gu, iu)
    if dtype == torch.float16:
        compare("C4 float16 weighted", lambda: ce.embedding_backward(gy, nu, t_idx, t_sid, remap, t_w, grad_embedding=g,
                                                                     inverse_mapping=i), g, i)
        compare("C4 float16 reference_sums", lambda: ce.embedding_backward(
            gy, nu, t_idx, t_sid, remap, grad_embedding=g, inverse_mapping=i, reference_sums=True), g, i, calls=10)
    del gy, g, i, gu, iu
del idx, t_idx, t_sid, t_w, remap, b_idx, b_sid, pairs, table, u_remap
torch.cuda.empty_cache()

ncat, W, H, B = 10_000_000, 32, 1, 131072           # unsliced: the window of 8
idx = torch.from_numpy(harness.generate_indices(ncat, B, H, alpha=0.0, index=np.int32)).to(dev)
t_idx, t_sid, _ = ce.transpose_fixed_hotness(idx, B, H, num_categories=ncat)
remap = ce.compute_compressed_grad_indices(t_idx)
nu = int(remap[-1].item()) + 1
gy = torch.randint(-1, 2, (B, W), device=dev).to(torch.float32)
g, i = buffers(nu, W, torch.float32)
assert ce.backward_launch_shape(torch.float32, torch.int32, W, B * H)["column_slices"] == 1
compare("uniform float32 W=32 B=131072", lambda: ce.embedding_backward(gy, nu, t_idx, t_sid, remap, grad_embedding=g,
                                                                       inverse_mapping=i), g, i)
if "--out" in sys.argv:
    with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
