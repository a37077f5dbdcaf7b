#!/usr/bin/env python3
"""Times the Adam family of the sparse optimizer step (cuembed_amd.ops.sparse_row_adam through
cuembed_amd.optim.SparseAdamUpdater) on one GPU, at the shape of benchmarks/optimizer_step_benchmark.py: the library's own
coalesced gradient of C4 (10 M x 256 fp16 table, batch 65,536, hotness 64, alpha 1.15).

In ONE process, on the same gradient and the same table, taking turns round by round:

    sgd, adagrad            SparseUpdater.apply                      (the yardsticks of this run)
    adam, rowwise_adam      SparseAdamUpdater.apply                  (clock launch + update)
    torch_sparse_adam       torch.optim.SparseAdam.step() on the same coalesced sparse gradient (moments in the table's
                            dtype; what a user runs without this module)

and reports, next to every time, the algorithmic bytes (from shapes) / time, and the ratios against Adagrad OF THE SAME
RUN with the ratio of the bytes moved: per fp16 element Adam moves 2 (g) + 4 (w, read and written) + 16 (m and v, read and
written) = 22 bytes against Adagrad's 14, so about 1.57 is expected; row-wise Adam moves 14 plus 8 bytes per row.

    python benchmarks/adam_step_benchmark.py --out profiles/sparse_adam_timing.json [--commit ID]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from optimizer_step_benchmark import FLOAT4_COPY_TBS, alternate, commit_id, faster, update_bytes  # noqa: E402


def step_bytes(n, width, elem_size, index_size, rule):
    """Bytes one step has to move for n gradient rows: ids, gradient rows, table rows read and written, state read and
    written."""
    if rule in ("sgd", "adagrad"):
        return update_bytes(n, width, elem_size, index_size, rule)
    state = {"adam": 8 * width, "rowwise_adam": 4 * width + 4}[rule]
    return n * (index_size + 3 * width * elem_size + 2 * state)


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--rows", type=int, default=10_000_000)
    p.add_argument("--width", type=int, default=256)
    p.add_argument("--hotness", type=int, default=64)
    p.add_argument("--alpha", type=float, default=1.15)
    p.add_argument("--batch", type=int, default=65536)
    p.add_argument("--calls", type=int, default=100, help="timed calls per round")
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--no-torch", action="store_true", help="leave torch.optim.SparseAdam out")
    p.add_argument("--out", default=None, help="write the JSON here as well")
    p.add_argument("--commit", default=None, help="commit the tree was built from (default: git rev-parse)")
    a = p.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("adam_step_benchmark: needs a GPU (there is nothing to time without one)")
    import cuembed_amd as ce
    from cuembed_amd import harness, optim
    torch.manual_seed(1)
    dev = torch.device("cuda")
    dtype = torch.float16
    ncat, W, H, batch = a.rows, a.width, a.hotness, a.batch
    table = torch.empty((ncat, W), dtype=dtype, device=dev).uniform_(-1, 1)
    idx = torch.from_numpy(harness.generate_indices(ncat, batch, H, alpha=a.alpha)).to(dev).view(batch, H)
    gy = (torch.rand((batch, W), device=dev) * 2 - 1).mul_(2.0 ** -6).to(dtype)
    t_idx, t_sid, _, remap = ce.transpose_fixed_hotness(idx, batch, H, num_categories=ncat, remapped=True)
    n = int(remap[-1].item()) + 1
    rows, ids = ce.embedding_backward(gy, n, t_idx, t_sid, remap)
    last_id = remap[-1:].clone()
    del t_idx, t_sid, remap, idx, gy
    lr = 1e-3
    sides = {}
    for rule in ("sgd", "adagrad"):
        sides[rule] = lambda up=optim.SparseUpdater(table, rule, lr): up.apply(ids, rows, last_id=last_id)
    for rule in ("adam", "rowwise_adam"):
        up = optim.SparseAdamUpdater(table, lr, rowwise=rule == "rowwise_adam")
        sides[rule] = lambda up=up: up.apply(ids, rows, last_id=last_id)
    torch_error = None
    if not a.no_torch:
        try:
            param = torch.nn.Parameter(table, requires_grad=True)
            param.grad = torch.sparse_coo_tensor(ids.long().unsqueeze(0), rows, size=(ncat, W), is_coalesced=True)
            t_opt = torch.optim.SparseAdam([param], lr=lr)
            t_opt.step()
            torch.cuda.synchronize()
            sides["torch_sparse_adam"] = t_opt.step
        except Exception as e:  # noqa: BLE001 - reported, not hidden: the library's sides are still timed
            torch_error = "%s: %s" % (type(e).__name__, e)
    got = alternate(torch, sides, a.calls, a.rounds, a.warmup)
    elem, index = table.element_size(), ids.element_size()
    for rule, side in got.items():
        if rule in ("sgd", "adagrad", "adam", "rowwise_adam"):
            side["algorithmic_bytes"] = step_bytes(n, W, elem, index, rule)
            side["tb_per_s"] = side["algorithmic_bytes"] / (side["ms"] * 1e-3) / 1e12
            side["share_of_float4_copy"] = side["tb_per_s"] / FLOAT4_COPY_TBS
    adagrad = got["adagrad"]
    ratios = {}
    for rule in ("adam", "rowwise_adam"):
        ratios[rule] = dict(time_ratio_to_adagrad=got[rule]["ms"] / adagrad["ms"],
                            byte_ratio_to_adagrad=got[rule]["algorithmic_bytes"] / adagrad["algorithmic_bytes"])
        ratios[rule]["time_ratio_over_byte_ratio"] = (ratios[rule]["time_ratio_to_adagrad"]
                                                      / ratios[rule]["byte_ratio_to_adagrad"])
    if "torch_sparse_adam" in got:
        ratios["adam"]["speedup_over_torch_sparse_adam"] = got["torch_sparse_adam"]["ms"] / got["adam"]["ms"]
        ratios["adam"]["faster_than_torch_beyond_the_spread"] = faster(got["adam"], got["torch_sparse_adam"])
    report = dict(tool="benchmarks/adam_step_benchmark.py", commit=commit_id(a.commit),
                  device=torch.cuda.get_device_name(0), torch=torch.__version__, calls_per_round=a.calls, rounds=a.rounds,
                  float4_copy_tb_per_s=FLOAT4_COPY_TBS, shape="C4" if (batch, ncat, W, H) == (65536, 10_000_000, 256, 64)
                  else "B=%d" % batch, dtype="float16", rows=ncat, width=W, batch=batch, hotness=H, alpha=a.alpha,
                  gradient_rows=n, update=got, against_adagrad_of_this_run=ratios, torch_sparse_adam_error=torch_error)
    for rule, side in got.items():
        line = "%-18s %.4f ms (spread %.4f)" % (rule, side["ms"], side["spread"])
        if "tb_per_s" in side:
            line += ", %.2f TB/s = %.0f %% of the float4 copy" % (side["tb_per_s"], 100 * side["share_of_float4_copy"])
        if rule in ratios:
            line += "; %.2fx Adagrad's time for %.2fx its bytes" % (ratios[rule]["time_ratio_to_adagrad"],
                                                                     ratios[rule]["byte_ratio_to_adagrad"])
        print(line, flush=True)
    if torch_error:
        print("torch.optim.SparseAdam could not be timed: " + torch_error, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(report, indent=1) + "\n")
    print(json.dumps(dict(summary=dict(update_ms={k: v["ms"] for k, v in got.items()}, against_adagrad=ratios))))


if __name__ == "__main__":
    main()
