#!/usr/bin/env python3
"""Times the sparse optimizer step (cuembed_amd.ops.sparse_row_update / cuembed_amd.optim) on one GPU:

  update   the update alone on the library's own coalesced gradient, per rule: time, algorithmic bytes (from shapes:
           ids + gradient rows + 2 x table rows + 2 x state) / time, and that rate as a share of the 6.29 TB/s a float4
           copy reaches on the MI355X -- against torch.optim.SGD / torch.optim.Adagrad stepping the SAME coalesced
           sparse gradient on the same table (what a user runs without this module);
  step     the whole training step: forward + SparseUpdater.backward_and_apply against
           cuemb_embedding(sparse_grad=True) + backward + torch.optim.SGD.step(), eager; at small batches also the
           library's step replayed from a HIP graph (torch's side reads the row count back and cannot be captured).

Shapes: C4 (10 M x 256, batch 65,536, hotness 64, alpha 1.15) in fp16 and fp32, and the same table at batch 1,024.
One process; device events around `--calls` calls after a warm-up; the two sides alternate, `--rounds` rounds each;
every figure is the median over the rounds (200 calls each by default) with the spread (max - min) of the same side
next to it.  A side is called faster only when its slowest round beats the other side's fastest.

    python benchmarks/optimizer_step_benchmark.py --out profiles/sparse_update_timing.json [--commit ID]

--stochastic-rounding times something else: what stochastic rounding of the store costs.  The update alone on the same
gradient (C4 and batch 1,024; fp16 and bf16 tables; every rule), round-to-nearest and stochastic rounding taking turns
in one process, 50 calls a round by default; per pair the ratio of the medians and whether the two are separable beyond
the spread (the slowest round of one below the fastest of the other).

    python benchmarks/optimizer_step_benchmark.py --stochastic-rounding --out profiles/stochastic_rounding_timing.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FLOAT4_COPY_TBS = 6.29      # measured float4 copy rate of an MI355X (the streaming ceiling used as the yardstick)


def update_bytes(n, width, elem_size, index_size, rule):
    """Bytes the update has to move for n gradient rows: ids, gradient rows, table rows read and written, state read
    and written."""
    state = {"sgd": 0, "adagrad": 4 * width, "rowwise_adagrad": 4}[rule]
    return n * (index_size + 3 * width * elem_size + 2 * state)


def time_calls(torch, fn, calls):
    """Milliseconds per call: one pair of device events around `calls` calls."""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / calls


def alternate(torch, sides, calls, rounds, warmup):
    """sides: {name: fn}.  Warm every side up, then `rounds` rounds in which the sides take turns.  Returns
    {name: dict(ms=median, min=, max=, spread=, rounds=[...])}."""
    for fn in sides.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    samples = {name: [] for name in sides}
    for _ in range(rounds):
        for name, fn in sides.items():
            samples[name].append(time_calls(torch, fn, calls))
    return {name: dict(ms=statistics.median(v), min=min(v), max=max(v), spread=max(v) - min(v), rounds=v)
            for name, v in samples.items()}


def faster(a, b):
    """a beats b by more than the spread of either side's repeated runs."""
    return a["max"] < b["min"]


def commit_id(given):
    if given:
        return given
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stdout=subprocess.PIPE,
                              stderr=subprocess.DEVNULL, text=True, check=True).stdout.strip()
    except Exception:  # noqa: BLE001 - a source tree without its history
        return "unknown"


def run_rounding_shape(torch, a, name, dtype, batch):
    """The update alone with round-to-nearest and with stochastic rounding, alternating, per rule."""
    import cuembed_amd as ce
    from cuembed_amd import harness, optim
    ncat, W, H = a.rows, a.width, a.hotness
    dev = torch.device("cuda")
    table = torch.empty((ncat, W), dtype=dtype, device=dev).uniform_(-1, 1)
    idx = torch.from_numpy(harness.generate_indices(ncat, batch, H, alpha=a.alpha)).to(dev).view(batch, H)
    gy = (torch.rand((batch, W), device=dev) * 2 - 1).mul_(2.0 ** -6).to(dtype)
    t_idx, t_sid, _, remap = ce.transpose_fixed_hotness(idx, batch, H, num_categories=ncat, remapped=True)
    n = int(remap[-1].item()) + 1
    rows, ids = ce.embedding_backward(gy, n, t_idx, t_sid, remap)
    last_id = remap[-1:].clone()
    del t_idx, t_sid, remap, idx, gy
    result = dict(shape=name, dtype=str(dtype).replace("torch.", ""), rows=ncat, width=W, batch=batch, hotness=H,
                  alpha=a.alpha, gradient_rows=n, gradient_bytes=n * W * table.element_size(), update={})
    for rule in ("sgd", "adagrad", "rowwise_adagrad"):
        nearest = optim.SparseUpdater(table, rule, 1e-3)
        stochastic = optim.SparseUpdater(table, rule, 1e-3, stochastic_rounding=True, seed=0x5EED)
        sides = {"nearest": lambda up=nearest: up.apply(ids, rows, last_id=last_id),
                 "stochastic": lambda up=stochastic: up.apply(ids, rows, last_id=last_id)}
        got = alternate(torch, sides, a.calls, a.rounds, a.warmup)
        moved = update_bytes(n, W, table.element_size(), ids.element_size(), rule)
        for side in got.values():
            side["tb_per_s"] = moved / (side["ms"] * 1e-3) / 1e12
            side["share_of_float4_copy"] = side["tb_per_s"] / FLOAT4_COPY_TBS
        result["update"][rule] = dict(got, algorithmic_bytes=moved, ratio=got["stochastic"]["ms"] / got["nearest"]["ms"],
                                      separable_beyond_the_spread=faster(got["nearest"], got["stochastic"])
                                      or faster(got["stochastic"], got["nearest"]))
        del nearest, stochastic, sides
        torch.cuda.empty_cache()
    del table
    torch.cuda.empty_cache()
    return result


def run_shape(torch, a, name, dtype, batch):
    import cuembed_amd as ce
    from cuembed_amd import cuembed_pyt as P
    from cuembed_amd import harness, optim
    ncat, W, H = a.rows, a.width, a.hotness
    dev = torch.device("cuda")
    table = torch.empty((ncat, W), dtype=dtype, device=dev).uniform_(-1, 1)
    idx = torch.from_numpy(harness.generate_indices(ncat, batch, H, alpha=a.alpha)).to(dev).view(batch, H)
    flat = idx.view(-1)
    offsets = torch.arange(0, batch * H + 1, H, dtype=torch.int32, device=dev)
    gy = (torch.rand((batch, W), device=dev) * 2 - 1).mul_(2.0 ** -6).to(dtype)
    t_idx, t_sid, _, remap = ce.transpose_fixed_hotness(idx, batch, H, num_categories=ncat, remapped=True)
    n = int(remap[-1].item()) + 1
    rows, ids = ce.embedding_backward(gy, n, t_idx, t_sid, remap)
    last_id = remap[-1:].clone()
    del t_idx, t_sid, remap
    result = dict(shape=name, dtype=str(dtype).replace("torch.", ""), rows=ncat, width=W, batch=batch, hotness=H,
                  alpha=a.alpha, gradient_rows=n, gradient_bytes=n * W * table.element_size(), update={}, step={})
    lr = 1e-3

    # ---- the update alone, library against torch on the same tensors
    ids64 = ids.long()
    sparse = torch.sparse_coo_tensor(ids64.unsqueeze(0), rows, size=(ncat, W), is_coalesced=True)
    for rule in ("sgd", "adagrad", "rowwise_adagrad"):
        up = optim.SparseUpdater(table, rule, lr)
        sides = {"library": lambda up=up: up.apply(ids, rows, last_id=last_id)}
        if rule != "rowwise_adagrad":
            param = torch.nn.Parameter(table, requires_grad=True)
            param.grad = sparse
            t_opt = torch.optim.SGD([param], lr=lr) if rule == "sgd" else torch.optim.Adagrad([param], lr=lr, eps=1e-8)
            sides["torch"] = t_opt.step
        got = alternate(torch, sides, a.calls, a.rounds, a.warmup)
        moved = update_bytes(n, W, table.element_size(), ids.element_size(), rule)
        entry = dict(got, algorithmic_bytes=moved)
        entry["library"]["tb_per_s"] = moved / (got["library"]["ms"] * 1e-3) / 1e12
        entry["library"]["share_of_float4_copy"] = entry["library"]["tb_per_s"] / FLOAT4_COPY_TBS
        if "torch" in got:
            entry["library_faster_than_torch"] = faster(got["library"], got["torch"])
            entry["speedup"] = got["torch"]["ms"] / got["library"]["ms"]
        result["update"][rule] = entry
        del up, sides
        if rule != "rowwise_adagrad":
            del t_opt, param
        torch.cuda.empty_cache()
    del sparse, ids64

    # ---- the whole step: forward + backward + update
    out = torch.empty((batch, W), dtype=dtype, device=dev)
    up = optim.SparseUpdater(table, "sgd", lr)

    def library_step():
        ce.embedding_forward(table, flat, num_hots=H, out=out)
        up.backward_and_apply(gy, idx)

    param = torch.nn.Parameter(table, requires_grad=True)
    t_opt = torch.optim.SGD([param], lr=lr)

    def torch_step():
        param.grad = None
        P.cuemb_embedding(param, flat, offsets, sparse_grad=True).backward(gy)
        t_opt.step()

    sides = {"library": library_step, "torch_sgd_behind_sparse_grad": torch_step}
    graph = None
    if batch <= a.graph_batch:
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            library_step()
            torch.cuda.current_stream().synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=s):
                library_step()
        torch.cuda.synchronize()
        sides["library_hip_graph"] = graph.replay
    got = alternate(torch, sides, a.calls, a.rounds, a.warmup)
    got["library_faster_than_torch"] = faster(got["library"], got["torch_sgd_behind_sparse_grad"])
    result["step"] = got
    assert not ce.capacity_overflowed()
    del graph, up, param, t_opt, table
    torch.cuda.empty_cache()
    return result


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--rows", type=int, default=10_000_000)
    p.add_argument("--width", type=int, default=256)
    p.add_argument("--hotness", type=int, default=64)
    p.add_argument("--alpha", type=float, default=1.15)
    p.add_argument("--batches", type=int, nargs="+", default=[65536, 1024])
    p.add_argument("--graph_batch", type=int, default=4096, help="replay the library's step from a HIP graph up to this batch")
    p.add_argument("--calls", type=int, default=None, help="timed calls per round (default 200; 50 with --stochastic-rounding)")
    p.add_argument("--stochastic-rounding", action="store_true",
                   help="time the update with round-to-nearest against stochastic rounding instead (fp16 and bf16 tables)")
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--out", default=None, help="write the JSON here as well")
    p.add_argument("--commit", default=None, help="commit the tree was built from (default: git rev-parse)")
    a = p.parse_args()
    if a.calls is None:
        a.calls = 50 if a.stochastic_rounding else 200
    import torch
    if not torch.cuda.is_available():
        sys.exit("optimizer_step_benchmark: needs a GPU (there is nothing to time without one)")
    torch.manual_seed(1)
    report = dict(tool="benchmarks/optimizer_step_benchmark.py", commit=commit_id(a.commit),
                  device=torch.cuda.get_device_name(0), torch=torch.__version__, calls_per_round=a.calls, rounds=a.rounds,
                  float4_copy_tb_per_s=FLOAT4_COPY_TBS, shapes=[])
    for batch in a.batches if a.stochastic_rounding else ():
        for dtype in (torch.float16, torch.bfloat16):
            name = "C4" if (batch, a.rows, a.width, a.hotness) == (65536, 10_000_000, 256, 64) else "B=%d" % batch
            r = run_rounding_shape(torch, a, name, dtype, batch)
            report["shapes"].append(r)
            for rule, e in r["update"].items():
                print("%s %s update %-16s nearest %.4f ms (spread %.4f, %.0f %% of the float4 copy), stochastic %.4f ms "
                      "(spread %.4f, %.0f %%): ratio %.3f, separable beyond the spread: %s" % (
                          name, r["dtype"], rule, e["nearest"]["ms"], e["nearest"]["spread"],
                          100 * e["nearest"]["share_of_float4_copy"], e["stochastic"]["ms"], e["stochastic"]["spread"],
                          100 * e["stochastic"]["share_of_float4_copy"], e["ratio"], e["separable_beyond_the_spread"]),
                      flush=True)
    for batch in () if a.stochastic_rounding else a.batches:
        for dtype in ((torch.float16, torch.float32) if batch == max(a.batches) else (torch.float16,)):
            name = "C4" if (batch, a.rows, a.width, a.hotness) == (65536, 10_000_000, 256, 64) else "B=%d" % batch
            r = run_shape(torch, a, name, dtype, batch)
            report["shapes"].append(r)
            for rule, e in r["update"].items():
                line = "%s %s update %-16s library %.4f ms (spread %.4f), %.2f TB/s = %.0f %% of the float4 copy" % (
                    name, r["dtype"], rule, e["library"]["ms"], e["library"]["spread"], e["library"]["tb_per_s"],
                    100 * e["library"]["share_of_float4_copy"])
                if "torch" in e:
                    line += "; torch %.4f ms (spread %.4f): %.1fx, faster beyond the spread: %s" % (
                        e["torch"]["ms"], e["torch"]["spread"], e["speedup"], e["library_faster_than_torch"])
                print(line, flush=True)
            print("%s %s step: %s" % (name, r["dtype"], ", ".join(
                "%s %.4f ms (spread %.4f)" % (k, v["ms"], v["spread"]) for k, v in r["step"].items() if isinstance(v, dict))),
                flush=True)
    text = json.dumps(report, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    if a.stochastic_rounding:
        print(json.dumps(dict(summary=[dict(shape=s["shape"], dtype=s["dtype"],
                                            nearest_ms={k: v["nearest"]["ms"] for k, v in s["update"].items()},
                                            stochastic_ms={k: v["stochastic"]["ms"] for k, v in s["update"].items()})
                                       for s in report["shapes"]])))
        return
    print(json.dumps(dict(summary=[dict(shape=s["shape"], dtype=s["dtype"],
                                        update_ms={k: v["library"]["ms"] for k, v in s["update"].items()},
                                        torch_ms={k: v["torch"]["ms"] for k, v in s["update"].items() if "torch" in v})
                                   for s in report["shapes"]])))


if __name__ == "__main__":
    main()
