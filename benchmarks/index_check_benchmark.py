#!/usr/bin/env python3
"""Times the device-side index check (cuembed_amd.check_indices) against its two yardsticks, on one GPU:

    report        check only: the four report words
    in_place      check + repair into the batch's own arrays (a clean batch: nothing is written)
    out_of_place  check + repair into separate arrays
    copy          device-to-device copy_ of the same index and offset tensors: the bytes of the out-of-place repair, the
                  yardstick for a streaming pass
    forward       the forward that the check protects, at the same shape

All contenders run in one process on the same tensors; they alternate, `--rounds` rounds of `--calls` calls each between
one pair of device events ("eager") and again as replays of a captured HIP graph ("graph").  Every figure is the median
over the rounds with min and max next to it; two sides are called separable only when the slower side's fastest round is
slower than the faster side's slowest (max < min).  The batches are clean (the expected case; a bad id costs one atomic
pair per wavefront that holds one).

Shapes:
    26 tables         26 x (1 M x 128) fp16, B = 2,048, ragged CSR bags of U[0, 40] lookups, int32 ids, int64 offsets
    4 tables          4 x (10 M x 256) fp16, B = 16,384, hotness 64
    headline          65,536 x 64 int32 ids, one table of 10 M x 256 fp16

    python benchmarks/index_check_benchmark.py --out profiles/index_check_timing.json [--commit ID]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from grouped_forward_benchmark import alternate, captured, commit_id, faster  # noqa: E402

CHECKS = ("report", "in_place", "out_of_place")


def run_shape(torch, a, name, source, forward, idx, offsets, batch, hot):
    """source: dict(num_rows=) or dict(group=); forward: the protected forward as a callable without arguments."""
    import cuembed_amd as ce
    tables = 1 if "num_rows" in source else source["group"].num_tables
    report = ce.new_index_report("cuda")
    need = ce.check_indices_workspace_bytes(tables, batch, hot, idx.numel())
    workspace = torch.empty((max(need, 8),), dtype=torch.uint8, device="cuda")
    idx_out = torch.empty_like(idx)
    off_out = None if offsets is None else torch.empty_like(offsets)
    common = dict(batch_size=batch, num_hots=hot, report=report, workspace=workspace)
    common.update(source)

    def report_only():
        ce.check_indices(idx, offsets, **common)

    def in_place():
        ce.check_indices(idx, offsets, repair=True, out_indices=idx, out_offsets=offsets, **common)

    def out_of_place():
        ce.check_indices(idx, offsets, repair=True, out_indices=idx_out, out_offsets=off_out, **common)

    def copy():
        idx_out.copy_(idx)
        if offsets is not None:
            off_out.copy_(offsets)

    sides = {"report": report_only, "in_place": in_place, "out_of_place": out_of_place, "copy": copy, "forward": forward}
    for fn in sides.values():
        fn()
    torch.cuda.synchronize()
    assert report.tolist() == [0, -1, 0, -1], "the benchmark's batch must be clean: %s" % report.tolist()
    assert torch.equal(idx_out, idx) and (offsets is None or torch.equal(off_out, offsets))
    eager = alternate(torch, sides, a.calls, a.rounds, a.warmup)
    graph = alternate(torch, {k: captured(torch, fn) for k, fn in sides.items()}, a.calls, a.rounds, a.warmup)
    moved = idx.numel() * idx.element_size() + (0 if offsets is None else offsets.numel() * offsets.element_size())
    r = dict(shape=name, tables=tables, batch_per_table=batch, hotness=hot or None, lookups=int(idx.numel()),
             index_bytes=int(idx.numel() * idx.element_size()), index_and_offset_bytes=int(moved), workspace_bytes=need,
             eager=eager, graph=graph)
    for how, got in (("eager", eager), ("graph", graph)):
        ratios = {}
        for c in CHECKS:
            for base in ("copy", "forward"):
                ratios["%s/%s" % (c, base)] = dict(
                    ratio=got[c]["ms"] / got[base]["ms"],
                    separable=faster(got[c], got[base]) or faster(got[base], got[c]),
                    faster_side=c if faster(got[c], got[base]) else (base if faster(got[base], got[c]) else None))
        r[how + "_ratios"] = ratios
        print("%-10s %-5s " % (name, how) + "  ".join("%s %.4f [%.4f, %.4f]" % (k, v["ms"], v["min"], v["max"])
                                                     for k, v in got.items()) + " ms", flush=True)
        print("%-10s %-5s " % (name, how) + "  ".join("%s %.2f%s" % (k, v["ratio"], "" if v["separable"] else " (~)")
                                                     for k, v in ratios.items()), flush=True)
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
        sys.exit("index_check_benchmark: needs a GPU (there is nothing to time without one)")
    import cuembed_amd as ce
    from cuembed_amd import harness
    torch.manual_seed(1)
    report = dict(tool="benchmarks/index_check_benchmark.py", commit=commit_id(a.commit),
                  device=torch.cuda.get_device_name(0),
                  arch=getattr(torch.cuda.get_device_properties(0), "gcnArchName", None), torch=torch.__version__,
                  calls_per_round=a.calls, rounds=a.rounds, shapes=[])

    # ---- 26 tables, 2,048 ragged bags each (the launch-bound shape of the grouped forward)
    T, W, B = 26, 128, 2048
    rng = np.random.default_rng(2)
    lengths = rng.integers(0, 41, T * B)
    offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)).cuda()
    idx = torch.from_numpy(rng.integers(0, a.small_rows, int(lengths.sum())).astype(np.int32)).cuda()
    group = ce.TableGroup([torch.empty((a.small_rows, W), dtype=torch.float16, device="cuda").uniform_(-1, 1)
                           for _ in range(T)])
    out = torch.empty((B, T, W), dtype=torch.float16, device="cuda")
    report["shapes"].append(run_shape(
        torch, a, "26 tables", dict(group=group),
        lambda: ce.embedding_forward_grouped(group, idx, offsets, out=out), idx, offsets, B, 0))
    del group, out
    torch.cuda.empty_cache()

    # ---- 4 tables of 10 M rows, 16,384 samples of 64 lookups each (the bandwidth-bound shape)
    T, W, B, H = 4, 256, 16384, 64
    group4 = ce.TableGroup([torch.empty((a.large_rows, W), dtype=torch.float16, device="cuda").uniform_(-1, 1)
                            for _ in range(T)])
    ids = harness.generate_indices(a.large_rows, T * B, H, alpha=1.15).reshape(T, B, H)
    idx4 = torch.from_numpy(np.ascontiguousarray(ids)).cuda()
    out4 = torch.empty((B, T, W), dtype=torch.float16, device="cuda")
    report["shapes"].append(run_shape(
        torch, a, "4 tables", dict(group=group4),
        lambda: ce.embedding_forward_grouped(group4, idx4, num_hots=H, out=out4), idx4, None, B, H))

    # ---- the headline index array: 65,536 x 64 int32, one table
    B1 = 65536
    table = group4.tables[0]
    idx1 = torch.from_numpy(np.ascontiguousarray(harness.generate_indices(a.large_rows, B1, H, alpha=1.15))
                            .astype(np.int32)).cuda().reshape(1, B1, H)
    out1 = torch.empty((B1, W), dtype=torch.float16, device="cuda")
    report["shapes"].append(run_shape(
        torch, a, "headline", dict(num_rows=a.large_rows),
        lambda: ce.embedding_forward(table, idx1.view(-1), num_hots=H, batch_size=B1, out=out1), idx1, None, B1, H))

    text = json.dumps(report, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(dict(summary=[dict(shape=s["shape"], eager={k: round(v["ms"], 5) for k, v in s["eager"].items()},
                                        graph={k: round(v["ms"], 5) for k, v in s["graph"].items()})
                                   for s in report["shapes"]])))


if __name__ == "__main__":
    main()
