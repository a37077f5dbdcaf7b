#!/usr/bin/env python3
"""Times the grouped forward (cuembed_amd.embedding_forward_grouped: T tables of one width in ONE launch, result
[B, T, W]) against what a caller has without it, on one GPU:

    loop          T calls of embedding_forward (embedding_forward_quantized), one [B, W] result per table
    loop+stack    the same loop followed by torch.stack(per_table, dim=1) into the [B, T, W] the layer above wants

All contenders run in one process on the same tensors; they alternate, `--rounds` rounds of `--calls` calls each between
one pair of device events ("eager": what the stream sees when the host enqueues as fast as it can) and again as replays
of a captured HIP graph ("graph": no host in the loop).  Every figure is the median over the rounds with min and max next
to it; a side is called faster only when its slowest round beats the other side's fastest (max < min).

Shape families:
    launch-bound      T = 26, W = 128, fp16,  1 M rows per table, B = 2,048, CSR bags of U[0, 40] lookups
    ... quantized     the same on fused 8-bit tables (fp16 output)
    bandwidth-bound   T = 4,  W = 256, fp16, 10 M rows per table, B = 16,384, hotness 64, alpha = 1.15 and alpha = 0

    python benchmarks/grouped_forward_benchmark.py --out profiles/grouped_forward_timing.json [--commit ID]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
    {name: dict(ms=median, min=, max=, rounds=[...])}."""
    for fn in sides.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    samples = {name: [] for name in sides}
    for _ in range(rounds):
        for name, fn in sides.items():
            samples[name].append(time_calls(torch, fn, calls))
    return {name: dict(ms=statistics.median(v), min=min(v), max=max(v), rounds=v) for name, v in samples.items()}


def faster(a, b):
    """a beats b by more than the spread of either side's repeated runs."""
    return a["max"] < b["min"]


def captured(torch, fn):
    """fn captured into a HIP graph on a side stream (one linear stream); returns the replay."""
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        fn()
        torch.cuda.current_stream().synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            fn()
    torch.cuda.synchronize()
    return g.replay


def commit_id(given):
    if given:
        return given
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stdout=subprocess.PIPE,
                              stderr=subprocess.DEVNULL, text=True, check=True).stdout.strip()
    except Exception:  # noqa: BLE001 - a source tree without its history
        return "unknown"


def run_family(torch, a, name, tables, quantized, batch, idx, offsets, hot):
    """idx: the group's ids (CSR: [nnz]; fixed: [T, B, H]); offsets: [T * B + 1] or None."""
    import cuembed_amd as ce
    T = len(tables)
    width = tables[0].shape[1] - (8 if quantized else 0)
    group = ce.TableGroup(tables)
    out_grouped = torch.empty((batch, T, width), dtype=torch.float16, device="cuda")
    out_stacked = torch.empty((batch, T, width), dtype=torch.float16, device="cuda")
    per_table = [torch.empty((batch, width), dtype=torch.float16, device="cuda") for _ in range(T)]
    # the single-table problems, sliced once (views of the group's tensors; CSR offsets rebased per table)
    pieces = []
    for t in range(T):
        if offsets is None:
            pieces.append((idx[t].reshape(-1), None))
        else:
            off = offsets[t * batch:(t + 1) * batch + 1]
            lo, hi = int(off[0]), int(off[-1])
            pieces.append((idx[lo:hi], (off - off[0]).contiguous()))

    if quantized:
        def grouped():
            ce.embedding_forward_quantized_grouped(group, idx, offsets, num_hots=hot, out=out_grouped)

        def loop():
            for t in range(T):
                ce.embedding_forward_quantized(tables[t], pieces[t][0], pieces[t][1], num_hots=hot, batch_size=batch,
                                               out=per_table[t])
    else:
        def grouped():
            ce.embedding_forward_grouped(group, idx, offsets, num_hots=hot, out=out_grouped)

        def loop():
            for t in range(T):
                ce.embedding_forward(tables[t], pieces[t][0], pieces[t][1], num_hots=hot, batch_size=batch,
                                     out=per_table[t])

    def loop_stack():
        loop()
        torch.stack(per_table, dim=1, out=out_stacked)

    sides = {"grouped": grouped, "loop": loop, "loop+stack": loop_stack}
    for fn in sides.values():
        fn()
    torch.cuda.synchronize()
    same = bool(torch.equal(out_grouped, out_stacked))
    eager = alternate(torch, sides, a.calls, a.rounds, a.warmup)
    graph = alternate(torch, {k: captured(torch, fn) for k, fn in sides.items()}, a.calls, a.rounds, a.warmup)
    r = dict(family=name, tables=T, width=width, quantized=quantized, batch_per_table=batch, hotness=hot or None,
             lookups=int(idx.numel()), same_bits_as_loop_and_stack=same, eager=eager, graph=graph)
    for how, got in (("eager", eager), ("graph", graph)):
        r[how + "_verdict"] = {
            "grouped_beats_loop": faster(got["grouped"], got["loop"]),
            "grouped_beats_loop+stack": faster(got["grouped"], got["loop+stack"]),
            "loop_beats_grouped": faster(got["loop"], got["grouped"]),
            # "does not lose beyond the loop's own run-to-run spread": grouped median <= loop max
            "grouped_within_the_spread_of_the_loop": got["grouped"]["ms"] <= got["loop"]["max"]}
        print("%-34s %-5s grouped %.4f [%.4f, %.4f]  loop %.4f [%.4f, %.4f]  loop+stack %.4f [%.4f, %.4f] ms  %s" % (
            name, how, got["grouped"]["ms"], got["grouped"]["min"], got["grouped"]["max"], got["loop"]["ms"],
            got["loop"]["min"], got["loop"]["max"], got["loop+stack"]["ms"], got["loop+stack"]["min"],
            got["loop+stack"]["max"], r[how + "_verdict"]), flush=True)
    assert same, "the grouped result differs from the stacked single-table results"
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
    a = p.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("grouped_forward_benchmark: needs a GPU (there is nothing to time without one)")
    import cuembed_amd as ce
    from cuembed_amd import harness
    torch.manual_seed(1)
    report = dict(tool="benchmarks/grouped_forward_benchmark.py", commit=commit_id(a.commit),
                  device=torch.cuda.get_device_name(0),
                  arch=getattr(torch.cuda.get_device_properties(0), "gcnArchName", None), torch=torch.__version__, calls_per_round=a.calls, rounds=a.rounds,
                  families=[])

    # ---- launch-bound: 26 tables, 2,048 ragged bags each
    T, W, B = 26, 128, 2048
    rng = np.random.default_rng(2)
    lengths = rng.integers(0, 41, T * B)
    offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)).cuda()
    idx = torch.from_numpy(rng.integers(0, a.small_rows, int(lengths.sum())).astype(np.int32)).cuda()
    tables = [torch.empty((a.small_rows, W), dtype=torch.float16, device="cuda").uniform_(-1, 1) for _ in range(T)]
    report["families"].append(run_family(torch, a, "launch-bound fp16", tables, False, B, idx, offsets, 0))
    qtables = [ce.quantize_rows(t) for t in tables]
    del tables
    report["families"].append(run_family(torch, a, "launch-bound 8-bit", qtables, True, B, idx, offsets, 0))
    del qtables
    torch.cuda.empty_cache()

    # ---- bandwidth-bound: 4 tables of 10 M rows, 16,384 samples of 64 lookups each
    T, W, B, H = 4, 256, 16384, 64
    tables = [torch.empty((a.large_rows, W), dtype=torch.float16, device="cuda").uniform_(-1, 1) for _ in range(T)]
    for alpha in (1.15, 0.0):
        ids = harness.generate_indices(a.large_rows, T * B, H, alpha=alpha).reshape(T, B, H)   # other samples per table
        idx = torch.from_numpy(np.ascontiguousarray(ids)).cuda()
        report["families"].append(run_family(torch, a, "bandwidth-bound fp16 alpha=%g" % alpha, tables, False, B, idx,
                                             None, H))
    text = json.dumps(report, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(dict(summary=[dict(family=f["family"], eager={k: v["ms"] for k, v in f["eager"].items()},
                                        graph={k: v["ms"] for k, v in f["graph"].items()}) for f in report["families"]])))


if __name__ == "__main__":
    main()
