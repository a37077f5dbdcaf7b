#!/usr/bin/env python3
"""Times the mixed-width grouped forward (cuembed_amd.embedding_forward_mixed_group: T tables of different widths in
ONE launch, result [B, D]) against what a caller has without it, on one GPU:

    mixed          the mixed-width call
    per-class+cat  one embedding_forward_grouped per width class ([B, T_c, W]), then torch.cat of the classes' [B, T_c * W]
                   views into [B, D] (the tables are ordered by width, so this is the same layout)
    loop+cat       T calls of embedding_forward, then torch.cat of the [B, W_t] results into [B, D]
    same-width     (second family only) the existing embedding_forward_grouped on a same-width variant, next to the mixed
                   call on the same tables

The protocol is benchmarks/grouped_forward_benchmark.py's: one process, the same tensors, the contenders alternating,
`--rounds` rounds of `--calls` calls each between one pair of device events, eager and as replays of a captured HIP
graph; median with min and max; a side is called faster only when its slowest round beats the other's fastest.  The
contenders' results are compared with torch.equal BEFORE anything is timed.

Families:
    (a)           26 x (1 M rows, fp16), widths cycling 16 / 32 / 64 / 128 (ordered by width), B = 2,048, CSR U[0, 40]
    (a) all 128   the same with every width 128: the same-width kernel's home ground
    (b)           4 x 10 M rows of widths 64 / 128 / 256 / 256, fp16, B = 16,384, H = 64, alpha = 1.15 and alpha = 0

    python benchmarks/mixed_group_forward_benchmark.py --out profiles/mixed_group_forward_timing.json [--commit ID]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from grouped_forward_benchmark import alternate, captured, commit_id, faster  # noqa: E402


def run_family(torch, a, name, tables, batch, idx, offsets, hot):
    """tables ordered by width; idx: the group's ids (CSR: [nnz]; fixed: [T, B, H]); offsets: [T * B + 1] or None."""
    import cuembed_amd as ce
    T = len(tables)
    widths = [t.shape[1] for t in tables]
    assert widths == sorted(widths), "tables ordered by width: every contender then writes the same [B, D] layout"
    D = sum(widths)
    dtype = tables[0].dtype
    mixed_group = ce.MixedTableGroup(tables)
    out_mixed = torch.empty((batch, D), dtype=dtype, device="cuda")
    out_classes = torch.empty((batch, D), dtype=dtype, device="cuda")
    out_loop = torch.empty((batch, D), dtype=dtype, device="cuda")
    per_table = [torch.empty((batch, w), dtype=dtype, device="cuda") for w in widths]
    # the single-table problems and the width classes, sliced once (views; CSR offsets rebased)
    pieces, classes, first = [], [], 0
    for t in range(T):
        if offsets is None:
            pieces.append((idx[t].reshape(-1), None))
        else:
            off = offsets[t * batch:(t + 1) * batch + 1]
            pieces.append((idx[int(off[0]):int(off[-1])], (off - off[0]).contiguous()))
    while first < T:
        last = first
        while last < T and widths[last] == widths[first]:
            last += 1
        n = last - first
        if offsets is None:
            c_idx, c_off = idx[first:last].contiguous(), None
        else:
            off = offsets[first * batch:last * batch + 1]
            c_idx, c_off = idx[int(off[0]):int(off[-1])], (off - off[0]).contiguous()
        classes.append((ce.TableGroup(tables[first:last]), c_idx, c_off,
                        torch.empty((batch, n, widths[first]), dtype=dtype, device="cuda")))
        first = last

    def mixed():
        ce.embedding_forward_mixed_group(mixed_group, idx, offsets, num_hots=hot, out=out_mixed)

    def per_class_cat():
        for group, c_idx, c_off, c_out in classes:
            ce.embedding_forward_grouped(group, c_idx, c_off, num_hots=hot, out=c_out)
        torch.cat([c[3].view(batch, -1) for c in classes], dim=1, out=out_classes)

    def loop_cat():
        for t in range(T):
            ce.embedding_forward(tables[t], pieces[t][0], pieces[t][1], num_hots=hot, batch_size=batch, out=per_table[t])
        torch.cat(per_table, dim=1, out=out_loop)

    sides = {"mixed": mixed, "per-class+cat": per_class_cat, "loop+cat": loop_cat}
    if len(classes) == 1:      # one width: the existing grouped call alone writes the layout, no cat
        group, c_idx, c_off, c_out = classes[0]
        sides["same-width"] = lambda: ce.embedding_forward_grouped(group, c_idx, c_off, num_hots=hot, out=c_out)
    for fn in sides.values():
        fn()
    torch.cuda.synchronize()
    same = bool(torch.equal(out_mixed, out_classes)) and bool(torch.equal(out_mixed, out_loop))
    assert same, "the contenders' results differ"
    eager = alternate(torch, sides, a.calls, a.rounds, a.warmup)
    graph = alternate(torch, {k: captured(torch, fn) for k, fn in sides.items()}, a.calls, a.rounds, a.warmup)
    r = dict(family=name, tables=T, widths=widths, width_classes=len(classes), embedding_dim=D, batch_per_table=batch,
             hotness=hot or None, lookups=int(idx.numel()), same_bits=same, eager=eager, graph=graph)
    for how, got in (("eager", eager), ("graph", graph)):
        verdict = {}
        for other in sides:
            if other != "mixed":
                verdict["mixed_vs_" + other] = ("faster" if faster(got["mixed"], got[other]) else
                                                "slower" if faster(got[other], got["mixed"]) else "the same")
        r[how + "_verdict"] = verdict
        print("%-26s %-5s %s  %s" % (name, how, "  ".join("%s %.4f [%.4f, %.4f]" % (k, v["ms"], v["min"], v["max"])
                                                          for k, v in got.items()), verdict), flush=True)
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
        sys.exit("mixed_group_forward_benchmark: needs a GPU (there is nothing to time without one)")
    from cuembed_amd import harness
    torch.manual_seed(1)
    report = dict(tool="benchmarks/mixed_group_forward_benchmark.py", commit=commit_id(a.commit),
                  device=torch.cuda.get_device_name(0),
                  arch=getattr(torch.cuda.get_device_properties(0), "gcnArchName", None), torch=torch.__version__,
                  calls_per_round=a.calls, rounds=a.rounds, families=[])

    def table(rows, width):
        return torch.empty((rows, width), dtype=torch.float16, device="cuda").uniform_(-1, 1)

    # ---- (a): 26 tables, 2,048 ragged bags each; widths cycling 16 / 32 / 64 / 128, ordered by width
    T, B = 26, 2048
    rng = np.random.default_rng(2)
    lengths = rng.integers(0, 41, T * B)
    offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)).cuda()
    idx = torch.from_numpy(rng.integers(0, a.small_rows, int(lengths.sum())).astype(np.int32)).cuda()
    widths = sorted((16, 32, 64, 128)[t % 4] for t in range(T))
    tables = [table(a.small_rows, w) for w in widths]
    report["families"].append(run_family(torch, a, "(a) 26 tables, 16-128", tables, B, idx, offsets, 0))
    del tables
    tables = [table(a.small_rows, 128) for _ in range(T)]
    report["families"].append(run_family(torch, a, "(a) 26 tables, all 128", tables, B, idx, offsets, 0))
    del tables
    torch.cuda.empty_cache()

    # ---- (b): 4 tables of 10 M rows, widths 64 / 128 / 256 / 256; 16,384 samples of 64 lookups each
    B, H = 16384, 64
    tables = [table(a.large_rows, w) for w in (64, 128, 256, 256)]
    for alpha in (1.15, 0.0):
        ids = harness.generate_indices(a.large_rows, 4 * B, H, alpha=alpha).reshape(4, B, H)
        idx = torch.from_numpy(np.ascontiguousarray(ids)).cuda()
        report["families"].append(run_family(torch, a, "(b) 4 tables alpha=%g" % alpha, tables, B, idx, None, H))
    text = json.dumps(report, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(dict(summary=[dict(family=f["family"], eager={k: v["ms"] for k, v in f["eager"].items()},
                                        graph={k: v["ms"] for k, v in f["graph"].items()},
                                        graph_verdict=f["graph_verdict"]) for f in report["families"]])))


if __name__ == "__main__":
    main()
