#!/usr/bin/env python3
"""Times the one-launch optimizer step of a mixed-width group (cuembed_amd.sparse_row_update_mixed_group /
sparse_row_adam_mixed_group) against what a caller has without it, on one GPU:

    mixed        the one-launch step on the MixedGroupedGrad of embedding_backward_mixed_group (eager and as graph replays)
    loop         MixedGroupedGrad.per_table() -- ONE read-back of the cuts -- and T single-table steps on its row views
                 made contiguous (eager only: a read-back cannot be captured); the same bits (checked on copies of the
                 tables and state before anything is timed, in every family)
    chain        forward + backward + step: the mixed-width forward, embedding_backward_mixed_group and the mixed step as
                 ONE graph replay, against the eager chain that ends in the loop

for SGD, row-wise Adagrad and row-wise Adam, and reports the step's achieved bytes per second from the bytes the rule
must move (per entry of width W in fp16: the gradient row, the weights read and written, 6 W; row-wise Adagrad + 8 for its
word; row-wise Adam + 8 W for the first moment read and written + 8 for its word; + the id), next to the 6.29 TB/s that a
float4 copy reaches on an MI355X.

The protocol is benchmarks/grouped_forward_benchmark.py's: one process, the same tensors, the arms alternating, `--rounds`
rounds of `--calls` calls each between one pair of device events; median with min and max; an arm is called faster only
when its slowest round beats the other's fastest.

Families (benchmarks/mixed_group_backward_benchmark.py's):
    (a)  26 x (1 M rows, fp16), widths cycling 16 / 32 / 64 / 128 (ordered by width), B = 2,048, CSR U[0, 40]
    (b)  4 x 10 M rows of widths 64 / 128 / 256 / 256, fp16, B = 16,384, H = 64, alpha = 1.15 and alpha = 0

    python benchmarks/mixed_group_optimizer_step_benchmark.py --out profiles/mixed_group_optimizer_step_timing.json
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from grouped_forward_benchmark import alternate, captured, commit_id, faster  # noqa: E402

RULES = ("sgd", "rowwise_adagrad", "rowwise_adam")
COPY_TBPS = 6.29
LR, EPS, BETAS = 1e-4, 1e-3, (0.9, 0.98)


def verdict(mine, other):
    return "faster" if faster(mine, other) else "slower" if faster(other, mine) else "the same"


def run_family(torch, a, name, tables, batch, idx, offsets, hot):
    import cuembed_amd as ce
    T = len(tables)
    widths = [t.shape[1] for t in tables]
    D, dtype = sum(widths), tables[0].dtype
    group = ce.MixedTableGroup(tables)
    flat_idx = idx.reshape(-1)
    grad_y = (torch.randint(-1, 2, (batch, D), device="cuda") * torch.randint(0, 2, (batch, D), device="cuda")).to(dtype)
    out_y = torch.empty((batch, D), dtype=dtype, device="cuda")
    grad = ce.embedding_backward_mixed_group(group, grad_y, flat_idx, offsets, num_hots=hot)
    cuts = grad.table_cuts().tolist()
    entries = [cuts[t + 1] - cuts[t] for t in range(T)]
    r = dict(family=name, tables=T, widths=widths, batch_per_table=batch, hotness=hot or None,
             lookups=int(flat_idx.numel()), entries=cuts[-1], rules={})
    for rule in RULES:
        adam = rule == "rowwise_adam"
        m = [torch.zeros(tuple(t.shape), dtype=torch.float32, device="cuda") for t in tables] if adam else None
        words = None if rule == "sgd" else [torch.full((t.shape[0],), 0.125, dtype=torch.float32, device="cuda") for t in tables]

        def mixed_step(g=None):
            g = g or grad
            if adam:
                ce.sparse_row_adam_mixed_group(group, g.ids, g.rows, exp_avg=m, exp_avg_sq=words, lr=LR, betas=BETAS, eps=EPS,
                                               rowwise=True, last_id=g.last_id)
            else:
                ce.sparse_row_update_mixed_group(group, g.ids, g.rows, rule=rule, lr=LR, eps=EPS, states=words,
                                                 last_id=g.last_id)

        def loop_step(g=None, into=None, m_into=None, words_into=None):
            into, m_into, words_into = into or tables, m_into or m, words_into or words
            for t, (local_ids, local_rows) in enumerate((g or grad).per_table()):
                local_rows = local_rows.contiguous()
                if adam:
                    ce.sparse_row_adam(into[t], local_ids, local_rows, exp_avg=m_into[t], exp_avg_sq=words_into[t], lr=LR,
                                       betas=BETAS, eps=EPS, rowwise=True)
                else:
                    ce.sparse_row_update(into[t], local_ids, local_rows, rule=rule, lr=LR, eps=EPS,
                                         state=None if words_into is None else words_into[t])

        def chain(step):
            def run():
                ce.embedding_forward_mixed_group(group, flat_idx if offsets is not None else idx, offsets, num_hots=hot, out=out_y)
                step(ce.embedding_backward_mixed_group(group, grad_y, flat_idx, offsets, num_hots=hot))
            return run

        # ---- the same bits from both arms, on copies, before anything is timed
        copies = [t.clone() for t in tables]
        m_copy = None if m is None else [s.clone() for s in m]
        words_copy = None if words is None else [s.clone() for s in words]
        mixed_step()
        loop_step(into=copies, m_into=m_copy, words_into=words_copy)
        torch.cuda.synchronize()
        same = all(torch.equal(x.view(torch.int16), y.view(torch.int16)) for x, y in zip(tables, copies))
        for mine, theirs in ((m, m_copy), (words, words_copy)):
            if mine is not None:
                same = same and all(torch.equal(x, y) for x, y in zip(mine, theirs))
        assert same, "the two arms' tables or state differ"
        del copies, m_copy, words_copy
        torch.cuda.empty_cache()
        per_elem = 6 + (8 if adam else 0)
        moved = sum(n * (w * per_elem + 4 + (0 if rule == "sgd" else 8)) for n, w in zip(entries, widths))
        steps = alternate(torch, {"mixed": mixed_step, "mixed, graph replay": captured(torch, mixed_step), "loop": loop_step},
                          a.calls, a.rounds, a.warmup)
        eager = {"mixed": steps["mixed"], "loop": steps["loop"]}
        graph = {"mixed": steps["mixed, graph replay"]}
        chains = alternate(torch, {"graph of the mixed chain": captured(torch, chain(mixed_step)),
                                   "eager mixed chain": chain(mixed_step), "eager loop chain": chain(loop_step)},
                           a.calls, a.rounds, a.warmup)
        r["rules"][rule] = dict(
            same_bits=same, bytes_moved=moved, step_eager=eager, step_graph=graph, chain=chains,
            step_tb_per_s=dict(eager=moved / eager["mixed"]["ms"] * 1e-9, graph=moved / graph["mixed"]["ms"] * 1e-9,
                               float4_copy=COPY_TBPS),
            verdicts=dict(mixed_graph_vs_mixed_eager=verdict(graph["mixed"], eager["mixed"]),
                          mixed_vs_loop_eager=verdict(eager["mixed"], eager["loop"]),
                          mixed_graph_vs_loop_eager=verdict(graph["mixed"], eager["loop"]),
                          chain_graph_vs_eager_loop_chain=verdict(chains["graph of the mixed chain"], chains["eager loop chain"])))
        line = lambda got: "  ".join("%s %.4f [%.4f, %.4f]" % (k, v["ms"], v["min"], v["max"]) for k, v in got.items())  # noqa: E731
        print("%-24s %-16s step eager: %s | graph: %s | %.2f TB/s" % (name, rule, line(eager), line(graph),
                                                                       r["rules"][rule]["step_tb_per_s"]["graph"]), flush=True)
        print("%-24s %-16s chain: %s  %s" % (name, rule, line(chains), r["rules"][rule]["verdicts"]), flush=True)
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
        sys.exit("mixed_group_optimizer_step_benchmark: needs a GPU (there is nothing to time without one)")
    from cuembed_amd import harness
    torch.manual_seed(1)
    report = dict(tool="benchmarks/mixed_group_optimizer_step_benchmark.py", commit=commit_id(a.commit),
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
        T, B = 26, 2048
        rng = np.random.default_rng(2)
        lengths = rng.integers(0, 41, T * B)
        offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)).cuda()
        idx = torch.from_numpy(rng.integers(0, a.small_rows, int(lengths.sum())).astype(np.int32)).cuda()
        tables = [table(a.small_rows, w) for w in sorted((16, 32, 64, 128)[t % 4] for t in range(T))]
        report["families"].append(run_family(torch, a, "(a) 26 tables, 16-128", tables, B, idx, offsets, 0))
        save()
        del tables
        torch.cuda.empty_cache()
    if "b" in a.families:
        B, H = 16384, 64
        tables = [table(a.large_rows, w) for w in (64, 128, 256, 256)]
        for alpha in (1.15, 0.0):
            ids = harness.generate_indices(a.large_rows, 4 * B, H, alpha=alpha).reshape(4, B, H)
            idx = torch.from_numpy(np.ascontiguousarray(ids)).cuda()
            report["families"].append(run_family(torch, a, "(b) 4 tables alpha=%g" % alpha, tables, B, idx, None, H))
            save()


if __name__ == "__main__":
    main()
