#!/usr/bin/env python3
"""Times the grouped backward (cuembed_amd.embedding_backward_grouped: the gradient of T tables of one width through ONE
key launch, ONE sort and ONE scatter-add) against what a caller has without it, on one GPU:

    backward   grouped   embedding_backward_grouped to a compressed gradient (global ids, device-side count)
               loop      T single-table chains: row ids, transpose with the remap, embedding_backward into buffers
                         (fixed hotness: transpose_fixed_hotness, which never materialises the sample ids)
    step       grouped   forward + backward + SGD on a ONE-STORAGE group: embedding_forward_grouped,
                         embedding_backward_grouped, one sparse_row_update on group.flat
               loop      T times embedding_forward, the chain above and sparse_row_update on the table

All contenders run in one process on the same indices and gradients; they alternate, `--rounds` rounds of `--calls` calls
each between one pair of device events ("eager") and again as replays of a captured HIP graph ("graph": no host in the
loop; nothing here reads back).  Every figure is the median over the rounds with min and max next to it; a side is called
faster only when its slowest round beats the other side's fastest (max < min).

Shape families (the ones the grouped forward was timed on):
    launch-bound      T = 26, W = 128, fp16,  1 M rows per table, B = 2,048, CSR bags of U[0, 40] lookups
    bandwidth-bound   T = 4,  W = 256, fp16, 10 M rows per table, B = 16,384, hotness 64, alpha = 1.15

    python benchmarks/grouped_backward_benchmark.py --out profiles/grouped_backward_timing.json [--commit ID]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "benchmarks"))

from grouped_forward_benchmark import alternate, captured, commit_id, faster  # noqa: E402


def run_family(torch, a, name, row_counts, width, batch, idx, offsets, hot):
    """idx: the group's ids (CSR: [nnz]; fixed: [T, B, H]); offsets: [T * B + 1] or None."""
    import cuembed_amd as ce
    T = len(row_counts)
    dtype, lr = torch.float16, 2.0 ** -20
    group = ce.TableGroup.allocate(row_counts, width, dtype=dtype)
    group.flat.uniform_(-1, 1)
    tables = [t.clone() for t in group.tables]
    grad_y = torch.empty((batch, T, width), dtype=dtype, device="cuda").uniform_(-1, 1)
    grad_t = [grad_y[:, t].contiguous() for t in range(T)]     # a caller of T separate lookups has them like this
    out_grouped = torch.empty((batch, T, width), dtype=dtype, device="cuda")
    per_table = [torch.empty((batch, width), dtype=dtype, device="cuda") for _ in range(T)]
    pieces = []                                                # the single-table problems, sliced once
    for t in range(T):
        if offsets is None:
            pieces.append((idx[t].reshape(-1), None, batch * hot))
        else:
            off = offsets[t * batch:(t + 1) * batch + 1]
            lo, hi = int(off[0]), int(off[-1])
            pieces.append((idx[lo:hi], (off - off[0]).to(torch.int32).contiguous(), hi - lo))
    buffers = [(torch.empty((min(n, row_counts[t]), width), dtype=dtype, device="cuda"),
                torch.empty((min(n, row_counts[t]),), dtype=idx.dtype, device="cuda")) for t, (_, _, n) in enumerate(pieces)]

    def chain(t):
        ids, off, n = pieces[t]
        if off is None:
            t_idx, t_sid, _, remap = ce.transpose_fixed_hotness(ids, batch, hot, num_categories=row_counts[t], remapped=True)
        else:
            sample_ids = ce.extract_row_ids_from_csr(off, nnz=n, dtype=torch.int32, batch_size=batch)
            t_idx, t_sid, _, remap = ce.transpose(sample_ids, ids, num_categories=row_counts[t], remapped=True)
        ce.embedding_backward(grad_t[t], None, t_idx, t_sid, remap, grad_embedding=buffers[t][0],
                              inverse_mapping=buffers[t][1])
        return remap[-1:]

    def backward_grouped():
        return ce.embedding_backward_grouped(group, grad_y, idx, offsets, num_hots=hot)

    def backward_loop():
        for t in range(T):
            chain(t)

    def step_grouped():
        ce.embedding_forward_grouped(group, idx, offsets, num_hots=hot, out=out_grouped)
        g = backward_grouped()
        ce.sparse_row_update(group.flat, g.ids, g.rows, rule="sgd", lr=lr, last_id=g.last_id)

    def step_loop():
        for t in range(T):
            ce.embedding_forward(tables[t], pieces[t][0], pieces[t][1], num_hots=hot, batch_size=batch, out=per_table[t])
            last = chain(t)
            ce.sparse_row_update(tables[t], buffers[t][1], buffers[t][0], rule="sgd", lr=lr, last_id=last)

    # the two backwards give the same gradient rows (up to the association of the sums): checked once, outside the timing
    g = backward_grouped()
    backward_loop()
    torch.cuda.synchronize()
    got = g.per_table()
    worst = 0.0
    for t in range(T):
        n = got[t][0].numel()
        assert torch.equal(got[t][0].to(idx.dtype), buffers[t][1][:n]), "table %d: the ids differ" % t
        if n:
            worst = max(worst, float((got[t][1].float() - buffers[t][0][:n].float()).abs().max()))
    sides = {"backward grouped": backward_grouped, "backward loop": backward_loop,
             "step grouped": step_grouped, "step loop": step_loop}
    eager = alternate(torch, sides, a.calls, a.rounds, a.warmup)
    graph = alternate(torch, {k: captured(torch, fn) for k, fn in sides.items()}, a.calls, a.rounds, a.warmup)
    assert not ce.capacity_overflowed()
    r = dict(family=name, tables=T, width=width, batch_per_table=batch, hotness=hot or None, lookups=int(idx.numel()),
             total_rows=int(sum(row_counts)), same_ids_as_the_loop=True, max_abs_difference_of_rows=worst, eager=eager,
             graph=graph)
    for how, res in (("eager", eager), ("graph", graph)):
        r[how + "_verdict"] = {
            "backward_grouped_beats_loop": faster(res["backward grouped"], res["backward loop"]),
            "backward_loop_beats_grouped": faster(res["backward loop"], res["backward grouped"]),
            "step_grouped_beats_loop": faster(res["step grouped"], res["step loop"]),
            "step_loop_beats_grouped": faster(res["step loop"], res["step grouped"])}
        print("%-32s %-5s %s  %s" % (name, how, "  ".join("%s %.4f [%.4f, %.4f]" % (k, v["ms"], v["min"], v["max"])
                                                           for k, v in res.items()), r[how + "_verdict"]), flush=True)
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
        sys.exit("grouped_backward_benchmark: needs a GPU (there is nothing to time without one)")
    from cuembed_amd import harness
    torch.manual_seed(1)
    report = dict(tool="benchmarks/grouped_backward_benchmark.py", commit=commit_id(a.commit),
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
