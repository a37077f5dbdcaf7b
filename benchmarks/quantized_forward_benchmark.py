#!/usr/bin/env python3
"""Times the forward on an 8-bit row-wise quantized table (cuembed_amd.embedding_forward_quantized, fp16 output)
against the existing fp16 forward (cuembed_amd.embedding_forward) on one GPU.

Both sides run on the same index stream; the quantized table is made from the same fp16 table.  Shapes: config 2
(10 M x 256, batch 65,536, hotness 64) at alpha = 1.15 and at alpha = 0, and batch 1,024 (alpha = 1.15); the quantizer
is timed on the whole 10 M x 256 table.  For each shape the report holds both times, their ratio, the ratio of
algorithmic bytes (rows read + output written, from shapes: at config 2 (64 * 264 + 512) / (65 * 512) = 0.523, the
floor for the time ratio) and, per side, achieved bytes / s against the 6.29 TB/s a float4 copy reaches on the MI355X.

One process; device events around `--calls` calls after a warm-up; the two sides alternate, `--rounds` rounds each;
every figure is the median over the rounds with the spread (max - min) of the same side next to it.  A side is called
faster only when its slowest round beats the other side's fastest.

    python benchmarks/quantized_forward_benchmark.py --out profiles/quantized_forward_timing.json [--commit ID]
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


def forward_bytes(batch, hotness, width, row_bytes, out_elem_size=2):
    """Bytes one forward has to move: every looked-up row once, every output row once (indices not counted: they are
    the same on both sides)."""
    return batch * (hotness * row_bytes + width * out_elem_size)


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


def run_shape(torch, a, table, qtable, name, batch, alpha, row_loads):
    import cuembed_amd as ce
    from cuembed_amd import harness
    ncat, W, H = a.rows, a.width, a.hotness
    idx = torch.from_numpy(harness.generate_indices(ncat, batch, H, alpha=alpha)).to("cuda")
    out16 = torch.empty((batch, W), dtype=torch.float16, device="cuda")
    outq = torch.empty((batch, W), dtype=torch.float16, device="cuda")
    sides = {
        "quantized": lambda: ce.embedding_forward_quantized(qtable, idx, num_hots=H, out=outq, row_loads=row_loads),
        "fp16": lambda: ce.embedding_forward(table, idx, num_hots=H, out=out16, row_loads=row_loads),
    }
    got = alternate(torch, sides, a.calls, a.rounds, a.warmup)
    # the two sides look up the same rows: the quantized sums differ from the fp16 ones by the 8-bit step only
    step = float((out16.float() - outq.float()).abs().max())
    bytes_q = forward_bytes(batch, H, W, W + 8)
    bytes_h = forward_bytes(batch, H, W, 2 * W)
    for side, moved in (("quantized", bytes_q), ("fp16", bytes_h)):
        got[side]["algorithmic_bytes"] = moved
        got[side]["tb_per_s"] = moved / (got[side]["ms"] * 1e-3) / 1e12
        got[side]["share_of_float4_copy"] = got[side]["tb_per_s"] / FLOAT4_COPY_TBS
    return dict(shape=name, rows=ncat, width=W, batch=batch, hotness=H, alpha=alpha, row_loads=row_loads or "default",
                quantized=got["quantized"], fp16=got["fp16"], time_ratio=got["quantized"]["ms"] / got["fp16"]["ms"],
                byte_ratio=bytes_q / bytes_h, quantized_faster_beyond_the_spread=faster(got["quantized"], got["fp16"]),
                fp16_faster_beyond_the_spread=faster(got["fp16"], got["quantized"]), max_abs_difference_of_outputs=step)


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--rows", type=int, default=10_000_000)
    p.add_argument("--width", type=int, default=256)
    p.add_argument("--hotness", type=int, default=64)
    p.add_argument("--batch", type=int, default=65536)
    p.add_argument("--small_batch", type=int, default=1024)
    p.add_argument("--calls", type=int, default=200, help="timed calls per round")
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--out", default=None, help="write the JSON here as well")
    p.add_argument("--commit", default=None, help="commit the tree was built from (default: git rev-parse)")
    a = p.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("quantized_forward_benchmark: needs a GPU (there is nothing to time without one)")
    import cuembed_amd as ce
    torch.manual_seed(1)
    table = torch.empty((a.rows, a.width), dtype=torch.float16, device="cuda").uniform_(-1, 1)
    qtable = torch.empty((a.rows, a.width + 8), dtype=torch.uint8, device="cuda")
    report = dict(tool="benchmarks/quantized_forward_benchmark.py", commit=commit_id(a.commit),
                  device=torch.cuda.get_device_name(0), torch=torch.__version__, calls_per_round=a.calls, rounds=a.rounds,
                  float4_copy_tb_per_s=FLOAT4_COPY_TBS, table_bytes=dict(fp16=table.numel() * 2, quantized=qtable.numel()),
                  shapes=[])

    # ---- the quantizer on the whole table (offline work: fewer calls, it moves 7.8 GB each)
    q = alternate(torch, {"quantize_rows": lambda: ce.quantize_rows(table, out=qtable)}, max(1, a.calls // 20), a.rounds, 2)
    moved = a.rows * (a.width * 2 + a.width + 8)
    q = q["quantize_rows"]
    q.update(algorithmic_bytes=moved, tb_per_s=moved / (q["ms"] * 1e-3) / 1e12)
    q["share_of_float4_copy"] = q["tb_per_s"] / FLOAT4_COPY_TBS
    report["quantizer"] = dict(rows=a.rows, width=a.width, input="float16", **q)
    print("quantize_rows %d x %d fp16: %.3f ms (spread %.3f), %.2f TB/s = %.0f %% of the float4 copy" % (
        a.rows, a.width, q["ms"], q["spread"], q["tb_per_s"], 100 * q["share_of_float4_copy"]), flush=True)

    cases = [("C2 alpha=1.15", a.batch, 1.15, None), ("C2 alpha=0", a.batch, 0.0, None),
             ("C2 alpha=0 streaming", a.batch, 0.0, "streaming"), ("B=%d alpha=1.15" % a.small_batch, a.small_batch, 1.15, None)]
    for name, batch, alpha, row_loads in cases:
        r = run_shape(torch, a, table, qtable, name, batch, alpha, row_loads)
        report["shapes"].append(r)
        print("%-22s quantized %.4f ms (spread %.4f, %.2f TB/s = %.0f %% of the copy)  fp16 %.4f ms (spread %.4f, %.2f TB/s"
              " = %.0f %%)  time ratio %.3f, byte ratio %.3f, quantized faster beyond the spread: %s" % (
                  name, r["quantized"]["ms"], r["quantized"]["spread"], r["quantized"]["tb_per_s"],
                  100 * r["quantized"]["share_of_float4_copy"], r["fp16"]["ms"], r["fp16"]["spread"], r["fp16"]["tb_per_s"],
                  100 * r["fp16"]["share_of_float4_copy"], r["time_ratio"], r["byte_ratio"],
                  r["quantized_faster_beyond_the_spread"]), flush=True)
    text = json.dumps(report, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(dict(summary=[dict(shape=s["shape"], quantized_ms=s["quantized"]["ms"], fp16_ms=s["fp16"]["ms"],
                                        time_ratio=s["time_ratio"], byte_ratio=s["byte_ratio"]) for s in report["shapes"]])))


if __name__ == "__main__":
    main()
