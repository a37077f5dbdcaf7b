#!/usr/bin/env python3
"""Times what trains a group beyond sum pooling with table gradients, on one GPU:

    weight gradient   embedding_weight_grad_grouped (ONE launch for T tables) against a loop of T calls of
                      embedding_weight_grad, each on grad_y[:, t, :].contiguous() (made once, outside the timing: a
                      caller of T separate lookups has its gradients like this);
    mean step         forward, backward and SGD on a one-storage group with mode="mean" (embedding_forward_grouped,
                      embedding_backward_grouped, one sparse_row_update on group.flat) against the same step with
                      mode="sum": the difference is what the scale launch costs.

The sides alternate in one process on the same tensors, `--rounds` rounds of `--calls` calls each between one pair of
device events ("eager") and again as replays of a captured HIP graph ("graph").  Every figure is the median over the
rounds with min and max; a side is called faster only when its slowest round beats the other side's fastest.

Shape families (those of grouped_forward_benchmark.py):
    launch-bound      T = 26, W = 128, fp16,  1 M rows per table, B = 2,048, CSR bags of U[0, 40] lookups
    bandwidth-bound   T = 4,  W = 256, fp16, 10 M rows per table, B = 16,384, hotness 64, alpha = 1.15

    python benchmarks/grouped_train_modes_benchmark.py --out profiles/grouped_train_modes_timing.json [--commit ID --parent ID]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "benchmarks"))

from grouped_forward_benchmark import alternate, captured, commit_id, faster  # noqa: E402


def parent_id(given):
    if given:
        return given
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD~1"], stdout=subprocess.PIPE,
                              stderr=subprocess.DEVNULL, text=True, check=True).stdout.strip()
    except Exception:  # noqa: BLE001 - a source tree without its history
        return "unknown"


def run_family(torch, a, name, row_counts, width, batch, idx, offsets, hot):
    """idx: the group's ids (CSR: [nnz]; fixed: [T, B, H]); offsets: [T * B + 1] or None."""
    import cuembed_amd as ce
    T = len(row_counts)
    dtype, lr = torch.float16, 2.0 ** -20
    group = ce.TableGroup.allocate(row_counts, width, dtype=dtype)
    group.flat.uniform_(-1, 1)
    grad_y = torch.empty((batch, T, width), dtype=dtype, device="cuda").uniform_(-1, 1)
    grad_t = [grad_y[:, t].contiguous() for t in range(T)]
    out = torch.empty((batch, T, width), dtype=dtype, device="cuda")
    grad_w = torch.empty((idx.numel(),), dtype=dtype, device="cuda")
    pieces = []                                                # the single-table problems, sliced once
    for t in range(T):
        if offsets is None:
            pieces.append((idx[t].reshape(-1), None))
        else:
            off = offsets[t * batch:(t + 1) * batch + 1]
            lo, hi = int(off[0]), int(off[-1])
            pieces.append((idx[lo:hi], (off - off[0]).contiguous()))

    def weight_grad_grouped():
        return ce.embedding_weight_grad_grouped(group, grad_y, idx, offsets, num_hots=hot, out=grad_w)

    def weight_grad_loop():
        return [ce.embedding_weight_grad(group.tables[t], pieces[t][0], grad_t[t], offsets=pieces[t][1], num_hots=hot,
                                         batch_size=batch) for t in range(T)]

    def step(mode):
        def run():
            ce.embedding_forward_grouped(group, idx, offsets, num_hots=hot, mode=mode, out=out)
            g = ce.embedding_backward_grouped(group, grad_y, idx, offsets, num_hots=hot, mode=mode)
            ce.sparse_row_update(group.flat, g.ids, g.rows, rule="sgd", lr=lr, last_id=g.last_id)
        return run

    # the two weight gradients have the same bits: checked once, outside the timing
    same = bool(torch.equal(weight_grad_grouped().view(-1), torch.cat([p.view(-1) for p in weight_grad_loop()])))
    sides = {"weight grad grouped": weight_grad_grouped, "weight grad loop": weight_grad_loop,
             "step mean": step("mean"), "step sum": step("sum")}
    eager = alternate(torch, sides, a.calls, a.rounds, a.warmup)
    graph = alternate(torch, {k: captured(torch, fn) for k, fn in sides.items()}, a.calls, a.rounds, a.warmup)
    assert not ce.capacity_overflowed()
    r = dict(family=name, tables=T, width=width, batch_per_table=batch, hotness=hot or None, lookups=int(idx.numel()),
             total_rows=int(sum(row_counts)), weight_grad_same_bits_as_the_loop=same, eager=eager, graph=graph)
    for how, res in (("eager", eager), ("graph", graph)):
        r[how + "_verdict"] = {
            "weight_grad_grouped_beats_loop": faster(res["weight grad grouped"], res["weight grad loop"]),
            "weight_grad_loop_beats_grouped": faster(res["weight grad loop"], res["weight grad grouped"]),
            "step_sum_beats_mean": faster(res["step sum"], res["step mean"]),
            "scale_launch_ms": res["step mean"]["ms"] - res["step sum"]["ms"]}
        print("%-32s %-5s %s  %s" % (name, how, "  ".join("%s %.4f [%.4f, %.4f]" % (k, v["ms"], v["min"], v["max"])
                                                           for k, v in res.items()), r[how + "_verdict"]), flush=True)
    assert same, "the grouped weight gradient differs from the single-table calls"
    return r


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--calls", type=int, default=100, help="timed calls per round")
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--small_rows", type=int, default=1_000_000)
    p.add_argument("--large_rows", type=int, default=10_000_000)
    p.add_argument("--out", default=None, help="write the JSON here as well")
    p.add_argument("--commit", default=None, help="commit the tree was built from (default: git rev-parse)")
    p.add_argument("--parent", default=None, help="its parent commit (default: git rev-parse HEAD~1)")
    a = p.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("grouped_train_modes_benchmark: needs a GPU (there is nothing to time without one)")
    from cuembed_amd import harness
    torch.manual_seed(1)
    report = dict(tool="benchmarks/grouped_train_modes_benchmark.py", commit=commit_id(a.commit), parent=parent_id(a.parent),
                  device=torch.cuda.get_device_name(0),
                  arch=getattr(torch.cuda.get_device_properties(0), "gcnArchName", None), torch=torch.__version__,
                  calls_per_round=a.calls, rounds=a.rounds, families=[])

    # ---- launch-bound: 26 tables, 2,048 ragged bags each
    T, W, B = 26, 128, 2048
    rng = np.random.default_rng(2)
    lengths = rng.integers(0, 41, T * B)
    offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)).cuda()
    idx = torch.from_numpy(rng.integers(0, a.small_rows, int(lengths.sum())).astype(np.int32)).cuda()
    report["families"].append(run_family(torch, a, "launch-bound fp16", (a.small_rows,) * T, W, B, idx, offsets, 0))
    torch.cuda.empty_cache()

    # ---- bandwidth-bound: 4 tables of 10 M rows, 16,384 samples of 64 lookups each
    T, W, B, H = 4, 256, 16384, 64
    ids = harness.generate_indices(a.large_rows, T * B, H, alpha=1.15).reshape(T, B, H)   # other samples per table
    idx = torch.from_numpy(np.ascontiguousarray(ids)).cuda()
    report["families"].append(run_family(torch, a, "bandwidth-bound fp16 alpha=1.15", (a.large_rows,) * T, W, B, idx, None, H))
    text = json.dumps(report, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(dict(summary=[dict(family=f["family"], eager={k: v["ms"] for k, v in f["eager"].items()},
                                        graph={k: v["ms"] for k, v in f["graph"].items()}) for f in report["families"]])))


if __name__ == "__main__":
    main()
