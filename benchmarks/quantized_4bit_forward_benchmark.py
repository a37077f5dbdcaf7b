#!/usr/bin/env python3
"""Times the forward on a fused 4-bit row-wise table (cuembed_amd.embedding_forward_quantized(bits=4), fp16 output)
against the 8-bit forward and the fp16 forward (cuembed_amd.embedding_forward) on one GPU.

The protocol is benchmarks/quantized_forward_benchmark.py's (its helpers are imported): one process, device events
around `--calls` calls after a warm-up, the three sides alternate, `--rounds` rounds each, median and [min, max] per
side; the same index stream on every side; both quantized tables made from the same fp16 table.  Shapes: the four rows
of DESIGN.md 3.8 -- config 2 (10 M x 256, batch 65,536, hotness 64) at alpha = 1.15, at alpha = 0 with default and with
streaming row loads, and batch 1,024 -- and the 4-bit quantizer on the whole table in one launch.  A side is called
faster than another only when its slowest round beats the other's fastest.

    python benchmarks/quantized_4bit_forward_benchmark.py --out profiles/quantized_4bit_forward_timing.json [--commit ID]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from quantized_forward_benchmark import FLOAT4_COPY_TBS, alternate, commit_id, faster, forward_bytes  # noqa: E402


def outcome(a, b):
    """How side a stands against side b: faster beyond the spread, the same within it, or slower."""
    return "faster" if faster(a, b) else "slower" if faster(b, a) else "same within the spread"


def run_shape(torch, a, tables, name, batch, alpha, row_loads):
    import cuembed_amd as ce
    from cuembed_amd import harness
    ncat, W, H = a.rows, a.width, a.hotness
    idx = torch.from_numpy(harness.generate_indices(ncat, batch, H, alpha=alpha)).to("cuda")
    out = {side: torch.empty((batch, W), dtype=torch.float16, device="cuda") for side in ("4bit", "8bit", "fp16")}
    sides = {
        "4bit": lambda: ce.embedding_forward_quantized(tables["4bit"], idx, num_hots=H, out=out["4bit"], row_loads=row_loads,
                                                       bits=4),
        "8bit": lambda: ce.embedding_forward_quantized(tables["8bit"], idx, num_hots=H, out=out["8bit"], row_loads=row_loads),
        "fp16": lambda: ce.embedding_forward(tables["fp16"], idx, num_hots=H, out=out["fp16"], row_loads=row_loads),
    }
    got = alternate(torch, sides, a.calls, a.rounds, a.warmup)
    row_bytes = {"4bit": W // 2 + 4, "8bit": W + 8, "fp16": 2 * W}
    for side, r in got.items():
        r["algorithmic_bytes"] = forward_bytes(batch, H, W, row_bytes[side])
        r["tb_per_s"] = r["algorithmic_bytes"] / (r["ms"] * 1e-3) / 1e12
        r["share_of_float4_copy"] = r["tb_per_s"] / FLOAT4_COPY_TBS
    return dict(shape=name, rows=ncat, width=W, batch=batch, hotness=H, alpha=alpha, row_loads=row_loads or "default",
                sides=got, time_ratio_4bit_to_8bit=got["4bit"]["ms"] / got["8bit"]["ms"],
                time_ratio_4bit_to_fp16=got["4bit"]["ms"] / got["fp16"]["ms"],
                byte_ratio_4bit_to_8bit=got["4bit"]["algorithmic_bytes"] / got["8bit"]["algorithmic_bytes"],
                outcome_4bit_against_8bit=outcome(got["4bit"], got["8bit"]),
                outcome_4bit_against_fp16=outcome(got["4bit"], got["fp16"]),
                # the sides look up the same rows: the sums differ by the quantization steps only
                max_abs_difference_4bit_to_fp16=float((out["4bit"].float() - out["fp16"].float()).abs().max()))


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
        sys.exit("quantized_4bit_forward_benchmark: needs a GPU (there is nothing to time without one)")
    import cuembed_amd as ce
    torch.manual_seed(1)
    tables = {"fp16": torch.empty((a.rows, a.width), dtype=torch.float16, device="cuda").uniform_(-1, 1)}
    tables["8bit"] = ce.quantize_rows(tables["fp16"])
    tables["4bit"] = torch.empty((a.rows, a.width // 2 + 4), dtype=torch.uint8, device="cuda")
    report = dict(tool="benchmarks/quantized_4bit_forward_benchmark.py", commit=commit_id(a.commit),
                  device=torch.cuda.get_device_name(0), torch=torch.__version__, calls_per_round=a.calls, rounds=a.rounds,
                  float4_copy_tb_per_s=FLOAT4_COPY_TBS,
                  table_bytes={side: t.numel() * t.element_size() for side, t in tables.items()}, shapes=[])

    # ---- the 4-bit quantizer on the whole table, one launch (offline work: fewer calls)
    q = alternate(torch, {"q": lambda: ce.quantize_rows(tables["fp16"], out=tables["4bit"], bits=4)}, max(1, a.calls // 20),
                  a.rounds, 2)["q"]
    moved = a.rows * (a.width * 2 + a.width // 2 + 4)
    q.update(algorithmic_bytes=moved, tb_per_s=moved / (q["ms"] * 1e-3) / 1e12)
    q["share_of_float4_copy"] = q["tb_per_s"] / FLOAT4_COPY_TBS
    report["quantizer"] = dict(rows=a.rows, width=a.width, input="float16", bits=4, **q)
    print("quantize_rows(bits=4) %d x %d fp16: %.3f ms [%.3f, %.3f], %.2f TB/s = %.0f %% of the float4 copy" % (
        a.rows, a.width, q["ms"], q["min"], q["max"], q["tb_per_s"], 100 * q["share_of_float4_copy"]), flush=True)

    cases = [("C2 alpha=1.15", a.batch, 1.15, None), ("C2 alpha=0", a.batch, 0.0, None),
             ("C2 alpha=0 streaming", a.batch, 0.0, "streaming"), ("B=%d alpha=1.15" % a.small_batch, a.small_batch, 1.15, None)]
    for name, batch, alpha, row_loads in cases:
        r = run_shape(torch, a, tables, name, batch, alpha, row_loads)
        report["shapes"].append(r)
        print("%-22s %s  | 4-bit / 8-bit %.3f (bytes %.3f): %s; 4-bit / fp16 %.3f: %s" % (
            name, "  ".join("%s %.4f ms [%.4f, %.4f]" % (s, v["ms"], v["min"], v["max"]) for s, v in r["sides"].items()),
            r["time_ratio_4bit_to_8bit"], r["byte_ratio_4bit_to_8bit"], r["outcome_4bit_against_8bit"],
            r["time_ratio_4bit_to_fp16"], r["outcome_4bit_against_fp16"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(report, indent=1) + "\n")
    print(json.dumps(dict(summary=[dict(shape=s["shape"], **{k: v["ms"] for k, v in s["sides"].items()},
                                        outcome_4bit_against_8bit=s["outcome_4bit_against_8bit"]) for s in report["shapes"]])))


if __name__ == "__main__":
    main()
