#!/usr/bin/env python3
"""Times the mixed-width grouped backward (cuembed_amd.embedding_backward_mixed_group: one key launch, one sort and ONE
scatter-add for T tables of different widths) against what a caller has without it, on one GPU:

    mixed          the mixed-width call (the launch shape PlanScatter picks for W_max)
    mixed 1 slice  the same under set_backward_tuning(column_slices=1)
    loop           T single-table chains (row ids, transpose with the remap, embedding_backward with the device-side
                   count) on grad_y[:, c_t:c_t + W_t].contiguous() -- only code that exists without the mixed kernel
    pad+reuse      grad_y spread into [B * T, W_max] by ONE gather launch (index_select with a precomputed column map
                   onto a zero column), then the same-width embedding_backward_grouped at W_max.  The contender is given
                   its best case: grad_y already lies in a persistent [B, D + 1] buffer whose last column is zero, as
                   if the layer above had written it there (the copy into it is not timed)
and, as "fwd+bwd", each of mixed / loop / pad+reuse behind its forward (mixed and pad+reuse: the mixed-width forward;
loop: T embedding_forward calls and torch.cat).

The protocol is benchmarks/grouped_forward_benchmark.py's: one process, the same tensors, the contenders alternating,
`--rounds` rounds of `--calls` calls each between one pair of device events, eager and as replays of a captured HIP
graph; median with min and max; a side is called faster only when its slowest round beats the other's fastest.  The
contenders' gradients are compared bit for bit on exactly representable data (grad_y in {-1, 0, 1}) BEFORE anything is
timed.

Families (benchmarks/mixed_group_forward_benchmark.py's):
    (a)  26 x (1 M rows, fp16), widths cycling 16 / 32 / 64 / 128 (ordered by width), B = 2,048, CSR U[0, 40]
    (b)  4 x 10 M rows of widths 64 / 128 / 256 / 256, fp16, B = 16,384, H = 64, alpha = 1.15 and alpha = 0

    python benchmarks/mixed_group_backward_benchmark.py --out profiles/mixed_group_backward_timing.json [--commit ID]
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
    rows = [t.shape[0] for t in tables]
    D, w_max, dtype = sum(widths), max(widths), tables[0].dtype
    cols = [sum(widths[:t]) for t in range(T + 1)]
    group = ce.MixedTableGroup(tables)
    # (the same-width pipeline reads no table value: uninitialised tables of the padded width)
    padded_group = ce.TableGroup([torch.empty((r, w_max), dtype=dtype, device="cuda") for r in rows])
    column_map = torch.tensor([cols[t] + j if j < widths[t] else D for t in range(T) for j in range(w_max)],
                              dtype=torch.int64, device="cuda")
    grad_y = (torch.randint(-1, 2, (batch, D), device="cuda") * torch.randint(0, 2, (batch, D), device="cuda")).to(dtype)
    staged_grad_y = torch.zeros((batch, D + 1), dtype=dtype, device="cuda")      # pad+reuse: grad_y and a zero column
    staged_grad_y[:, :D] = grad_y
    flat_idx = idx.reshape(-1)
    pieces = []
    for t in range(T):
        if offsets is None:
            pieces.append((idx[t].reshape(-1).contiguous(), None))
        else:
            off = offsets[t * batch:(t + 1) * batch + 1]
            pieces.append((flat_idx[int(off[0]):int(off[-1])], (off - off[0]).contiguous()))
    results = {}

    def mixed():
        results["mixed"] = ce.embedding_backward_mixed_group(group, grad_y, flat_idx, offsets, num_hots=hot)

    def mixed_one_slice():
        try:
            ce.set_backward_tuning(segment_len=0, column_slices=1)
            results["mixed 1 slice"] = ce.embedding_backward_mixed_group(group, grad_y, flat_idx, offsets, num_hots=hot)
        finally:
            ce.set_backward_tuning(segment_len=0, column_slices=0)

    def loop():
        out = []
        for t in range(T):
            ids_t, off_t = pieces[t]
            nnz = ids_t.numel()
            grad_t = grad_y[:, cols[t]:cols[t + 1]].contiguous()
            if off_t is None:
                t_idx, t_sid, _, remap = ce.transpose_fixed_hotness(ids_t, batch, hot, num_categories=rows[t], remapped=True)
            else:
                sid = ce.extract_row_ids_from_csr(off_t, nnz=nnz, dtype=ids_t.dtype)
                t_idx, t_sid, _, remap = ce.transpose(sid, ids_t, None, num_categories=rows[t], remapped=True)
            capacity = min(nnz, rows[t])
            g = torch.empty((capacity, widths[t]), dtype=dtype, device="cuda")
            inv = torch.empty((capacity,), dtype=ids_t.dtype, device="cuda")
            ce.embedding_backward(grad_t, None, t_idx, t_sid, remap, None, grad_embedding=g, inverse_mapping=inv)
            out.append((inv, g, remap[-1:]))
        results["loop"] = out

    def pad_reuse():
        spread = staged_grad_y.index_select(1, column_map)
        results["pad+reuse"] = ce.embedding_backward_grouped(padded_group, spread.view(batch, T, w_max), flat_idx, offsets,
                                                             num_hots=hot, dense=False)

    out_mixed = torch.empty((batch, D), dtype=dtype, device="cuda")
    per_table = [torch.empty((batch, w), dtype=dtype, device="cuda") for w in widths]
    out_loop = torch.empty((batch, D), dtype=dtype, device="cuda")

    def forward_mixed():
        ce.embedding_forward_mixed_group(group, flat_idx if offsets is not None else idx, offsets, num_hots=hot, out=out_mixed)

    def forward_loop():
        for t in range(T):
            ce.embedding_forward(tables[t], pieces[t][0], pieces[t][1], num_hots=hot, batch_size=batch, out=per_table[t])
        torch.cat(per_table, dim=1, out=out_loop)

    def both(forward, backward):
        def step():
            forward()
            backward()
        return step

    sides = {"mixed": mixed, "mixed 1 slice": mixed_one_slice, "loop": loop, "pad+reuse": pad_reuse}
    for fn in sides.values():
        fn()
    torch.cuda.synchronize()
    # ---- the same gradient, bit for bit, from every contender
    m, one, padded = results["mixed"], results["mixed 1 slice"], results["pad+reuse"]
    count = int(m.last_id) + 1
    same = int(one.last_id) + 1 == count == int(padded.last_id) + 1 and bool(torch.equal(m.ids[:count], padded.ids[:count]))
    for (ids_m, rows_m), (ids_1, rows_1), (inv, g, last), t in zip(m.per_table(), one.per_table(), results["loop"], range(T)):
        n = int(last) + 1
        same = same and ids_m.numel() == n and bool(torch.equal(ids_m, inv[:n])) and bool(torch.equal(rows_m, g[:n]))
        same = same and bool(torch.equal(ids_1, ids_m)) and bool(torch.equal(rows_1, rows_m))
    cuts = m.table_cuts().tolist()
    for t in range(T):
        same = same and bool(torch.equal(padded.rows[cuts[t]:cuts[t + 1], :widths[t]], m.rows[cuts[t]:cuts[t + 1], :widths[t]]))
    print("%-26s the contenders' gradients are %s (%d entries)" % (name, "bit-identical" if same else "DIFFERENT", count),
          flush=True)
    assert same, "the contenders' gradients differ"
    shape = ce.mixed_group_backward_launch_shape(dtype, widths, flat_idx.numel(), pointer_bits=grad_y.data_ptr())
    both_sides = {"mixed": both(forward_mixed, mixed), "loop": both(forward_loop, loop),
                  "pad+reuse": both(forward_mixed, pad_reuse)}
    r = dict(family=name, tables=T, widths=widths, embedding_dim=D, batch_per_table=batch, hotness=hot or None,
             lookups=int(flat_idx.numel()), entries=count, same_bits=same, launch_shape=shape)
    for what, these in (("backward", sides), ("forward_backward", both_sides)):
        eager = alternate(torch, these, a.calls, a.rounds, a.warmup)
        graph = alternate(torch, {k: captured(torch, fn) for k, fn in these.items()}, a.calls, a.rounds, a.warmup)
        r[what] = dict(eager=eager, graph=graph)
        for how, got in (("eager", eager), ("graph", graph)):
            verdict = {}
            for other in these:
                if other != "mixed":
                    verdict["mixed_vs_" + other] = ("faster" if faster(got["mixed"], got[other]) else
                                                    "slower" if faster(got[other], got["mixed"]) else "the same")
            r[what][how + "_verdict"] = verdict
            print("%-26s %-16s %-5s %s  %s" % (name, what, how, "  ".join("%s %.4f [%.4f, %.4f]" % (k, v["ms"], v["min"], v["max"])
                                                                          for k, v in got.items()), verdict), flush=True)
    return r


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--calls", type=int, default=100, help="timed calls per round")
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--small_rows", type=int, default=1_000_000)
    p.add_argument("--large_rows", type=int, default=10_000_000)
    p.add_argument("--families", default="a,b", help="which families to run: a, b or a,b")
    p.add_argument("--out", default=None, help="write the JSON here as well")
    p.add_argument("--commit", default=None, help="commit the tree was built from (default: git rev-parse)")
    a = p.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("mixed_group_backward_benchmark: needs a GPU (there is nothing to time without one)")
    from cuembed_amd import harness
    torch.manual_seed(1)
    report = dict(tool="benchmarks/mixed_group_backward_benchmark.py", commit=commit_id(a.commit),
                  device=torch.cuda.get_device_name(0),
                  arch=getattr(torch.cuda.get_device_properties(0), "gcnArchName", None), torch=torch.__version__,
                  calls_per_round=a.calls, rounds=a.rounds, families=[])

    def table(rows, width):
        return torch.empty((rows, width), dtype=torch.float16, device="cuda").uniform_(-1, 1)

    def save():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(json.dumps(report, indent=1) + "\n")

    if "a" in a.families:
        # ---- (a): 26 tables, 2,048 ragged bags each; widths cycling 16 / 32 / 64 / 128, ordered by width
        T, B = 26, 2048
        rng = np.random.default_rng(2)
        lengths = rng.integers(0, 41, T * B)
        offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)).cuda()
        idx = torch.from_numpy(rng.integers(0, a.small_rows, int(lengths.sum())).astype(np.int32)).cuda()
        widths = sorted((16, 32, 64, 128)[t % 4] for t in range(T))
        tables = [table(a.small_rows, w) for w in widths]
        report["families"].append(run_family(torch, a, "(a) 26 tables, 16-128", tables, B, idx, offsets, 0))
        save()
        del tables
        torch.cuda.empty_cache()
    if "b" in a.families:
        # ---- (b): 4 tables of 10 M rows, widths 64 / 128 / 256 / 256; 16,384 samples of 64 lookups each
        B, H = 16384, 64
        tables = [table(a.large_rows, w) for w in (64, 128, 256, 256)]
        for alpha in (1.15, 0.0):
            ids = harness.generate_indices(a.large_rows, 4 * B, H, alpha=alpha).reshape(4, B, H)
            idx = torch.from_numpy(np.ascontiguousarray(ids)).cuda()
            report["families"].append(run_family(torch, a, "(b) 4 tables alpha=%g" % alpha, tables, B, idx, None, H))
            save()
    print(json.dumps(dict(summary=[dict(family=f["family"],
                                        backward_graph={k: v["ms"] for k, v in f["backward"]["graph"].items()},
                                        backward_graph_verdict=f["backward"]["graph_verdict"],
                                        forward_backward_graph={k: v["ms"] for k, v in f["forward_backward"]["graph"].items()})
                                   for f in report["families"]])))


if __name__ == "__main__":
    main()
