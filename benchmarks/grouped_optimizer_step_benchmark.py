#!/usr/bin/env python3
"""Times the optimizer step on a group of SEPARATE table tensors (cuembed_amd.sparse_row_update_grouped /
sparse_row_adam_grouped: one launch, the kernel finds each entry's table) against what a caller has without it, on one GPU:

    step alone   grouped   the grouped step on the compressed gradient of the group (global ids, device-side count)
                 loop      today's way on separate tensors: GroupedGrad.per_table() -- ONE read-back of the cuts -- and
                           T single-table steps; eager only, a read-back cannot be captured
                 flat      the existing single-table step on a ONE-STORAGE copy of the same group (group.flat and one state
                           tensor for all rows): the floor, for models that can hold their tables like that
                 for SGD, row-wise Adagrad and row-wise Adam
    whole step   grouped   forward + backward + step on separate tensors: embedding_forward_grouped and
                           GroupSparseUpdater.backward_and_apply (SGD)
                 flat      the one-storage chain: embedding_forward_grouped, embedding_backward_grouped, sparse_row_update
                           on group.flat

All contenders run in one process on the same indices and gradients; they alternate, `--rounds` rounds of `--calls` calls
each between one pair of device events ("eager") and again as replays of a captured HIP graph ("graph").  Every figure is
the median over the rounds with min and max next to it; a pair is called "faster beyond the spread" only when the slowest
round of one side beats the fastest of the other, "slower beyond the spread" likewise, else "the same within the spread".

Shape families (those of the grouped forward and backward):
    launch-bound      T = 26, W = 128, fp16,  1 M rows per table, B = 2,048, CSR bags of U[0, 40] lookups
    bandwidth-bound   T = 4,  W = 256, fp16, 10 M rows per table, B = 16,384, hotness 64, alpha = 1.15

    python benchmarks/grouped_optimizer_step_benchmark.py --out profiles/grouped_optimizer_step_timing.json

Stochastic rounding: `--stochastic-rounding` times the step alone with one seed per table instead (fp16 tables, the same
two shapes and three rules; `--out profiles/grouped_optimizer_step_stochastic_timing.json`):
    stochastic   the grouped step with stochastic_rounding=True, seeds=[one per table]
    nearest      the grouped step with round to nearest, on the same tree: the difference prices the rounding
    loop         GroupedGrad.per_table() -- the read-back -- and T single-table stochastic steps with seed = seeds[t]: the
                 same bits as `stochastic`, and the only way to them without it; eager only
    flat         the existing single-table stochastic step on a one-storage copy: other bits (named by the global row),
                 the same work
The step comes from one int64 device word in every stochastic arm.

No regression on the existing step: `--existing-only --tree DIR --out FILE` times the `flat` arms alone with the package of
another checkout (built there), e.g. the parent commit's; a full run with `--parent-existing FILE [FILE ...]` records them
next to its own `flat` arms with the verdict of each pair (one such run before and one after the full run show the
machine's drift between processes; `--this-existing FILE`, an --existing-only run of this tree between the two, is then
what they are compared with: the same process on both sides).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "benchmarks"))

RULES = ("sgd", "rowwise_adagrad", "rowwise_adam")
LR = 2.0 ** -20


def verdict(a, b):
    """a against b: beyond the spread only when one side's slowest round beats the other's fastest."""
    if a["max"] < b["min"]:
        return "faster beyond the spread"
    if b["max"] < a["min"]:
        return "slower beyond the spread"
    return "the same within the spread"


def line(name, how, res):
    print("%-32s %-5s %s" % (name, how, "  ".join("%s %.4f [%.4f, %.4f]" % (k, v["ms"], v["min"], v["max"])
                                                   for k, v in res.items())), flush=True)


def flat_state(torch, rule, total, width):
    """The one-storage step's state: (state) or (exp_avg, exp_avg_sq) over all rows of the group."""
    if rule == "rowwise_adagrad":
        return (torch.full((total,), 0.1, dtype=torch.float32, device="cuda"),)
    if rule == "rowwise_adam":
        return (torch.zeros((total, width), dtype=torch.float32, device="cuda"),
                torch.zeros((total,), dtype=torch.float32, device="cuda"))
    return ()


def run_family_stochastic(torch, ce, a, name, row_counts, width, batch, idx, offsets, hot, timers):
    """--stochastic-rounding: the step alone, grouped with seeds against grouped nearest, the per-table loop and the
    one-storage step, for the three rules."""
    alternate, captured = timers
    T, total, dtype = len(row_counts), sum(row_counts), torch.float16
    flat_group = ce.TableGroup.allocate(row_counts, width, dtype=dtype)
    flat_group.flat.uniform_(-1, 1)
    grad_y = torch.empty((batch, T, width), dtype=dtype, device="cuda").uniform_(-1, 1)
    grad = ce.embedding_backward_grouped(flat_group, grad_y, idx, offsets, num_hots=hot)
    bias = torch.full((1,), 0.8, dtype=torch.float32, device="cuda")
    step = torch.full((1,), 2 ** 32 + 5, dtype=torch.int64, device="cuda")
    seeds = [0x9E3779B97F4A7C15 * (t + 1) % 2 ** 64 for t in range(T)]
    r = dict(family=name, tables=T, width=width, batch_per_table=batch, hotness=hot or None, lookups=int(idx.numel()),
             total_rows=int(total), entries=int(grad.last_id.item()) + 1, step_alone={})
    group = ce.TableGroup([t.clone() for t in flat_group.tables])          # the same tables as separate tensors
    from cuembed_amd import optim
    for rule in RULES:
        state = flat_state(torch, rule, total, width)
        if rule == "rowwise_adam":
            updater = optim.GroupSparseAdamUpdater(group, LR, rowwise=True)
        else:
            updater = optim.GroupSparseUpdater(group, rule, LR, initial_accumulator_value=0.1)

        def grouped(rounding, updater=updater, rule=rule):
            if rule == "rowwise_adam":      # (the functions, not updater.apply: no clock or step-word launch in any arm)
                return lambda: ce.sparse_row_adam_grouped(group, grad.ids, grad.rows, exp_avg=updater.exp_avg,
                                                          exp_avg_sq=updater.exp_avg_sq, lr=LR, bias_factor=bias,
                                                          rowwise=True, last_id=grad.last_id, **rounding)
            return lambda: ce.sparse_row_update_grouped(group, grad.ids, grad.rows, rule=rule, lr=LR, states=updater.states,
                                                        last_id=grad.last_id, **rounding)

        def loop(updater=updater, rule=rule):
            for t, (ids, rows) in enumerate(grad.per_table()):           # (the read-back is inside per_table)
                kw = dict(stochastic_rounding=True, seed=seeds[t], step=step)
                if rule == "rowwise_adam":
                    ce.sparse_row_adam(group.tables[t], ids, rows, exp_avg=updater.exp_avg[t],
                                       exp_avg_sq=updater.exp_avg_sq[t], lr=LR, bias_factor=bias, rowwise=True, **kw)
                else:
                    ce.sparse_row_update(group.tables[t], ids, rows, rule=rule, lr=LR,
                                         state=updater.states[t] if updater.states else None, **kw)

        def flat(rule=rule, state=state):
            kw = dict(stochastic_rounding=True, seed=seeds[0], step=step, last_id=grad.last_id)
            if rule == "rowwise_adam":
                return ce.sparse_row_adam(flat_group.flat, grad.ids, grad.rows, exp_avg=state[0], exp_avg_sq=state[1],
                                          lr=LR, bias_factor=bias, rowwise=True, **kw)
            return ce.sparse_row_update(flat_group.flat, grad.ids, grad.rows, rule=rule, lr=LR,
                                        state=state[0] if state else None, **kw)

        sides = {"stochastic": grouped(dict(stochastic_rounding=True, seeds=seeds, step=step)), "nearest": grouped({}),
                 "loop": loop, "flat": flat}
        eager = alternate(torch, sides, a.calls, a.rounds, a.warmup)
        graph = alternate(torch, {k: captured(torch, f) for k, f in sides.items() if k != "loop"}, a.calls, a.rounds,
                          a.warmup)
        r["step_alone"][rule] = dict(
            eager=eager, graph=graph,
            verdicts={"eager stochastic against loop": verdict(eager["stochastic"], eager["loop"]),
                      "graph stochastic against eager loop": verdict(graph["stochastic"], eager["loop"]),
                      "eager stochastic against nearest": verdict(eager["stochastic"], eager["nearest"]),
                      "graph stochastic against nearest": verdict(graph["stochastic"], graph["nearest"]),
                      "eager stochastic against flat": verdict(eager["stochastic"], eager["flat"]),
                      "graph stochastic against flat": verdict(graph["stochastic"], graph["flat"])})
        line(name + " " + rule, "eager", eager)
        line(name + " " + rule, "graph", graph)
        print("    ", r["step_alone"][rule]["verdicts"], flush=True)
        del state, updater, sides, grouped, loop, flat
    return r


def run_family(torch, ce, a, name, row_counts, width, batch, idx, offsets, hot, timers):
    if a.stochastic_rounding:
        return run_family_stochastic(torch, ce, a, name, row_counts, width, batch, idx, offsets, hot, timers)
    """idx: the group's ids (CSR: [nnz]; fixed: [T, B, H]); offsets: [T * B + 1] or None."""
    alternate, captured = timers
    T, total, dtype = len(row_counts), sum(row_counts), torch.float16
    flat_group = ce.TableGroup.allocate(row_counts, width, dtype=dtype)
    flat_group.flat.uniform_(-1, 1)
    grad_y = torch.empty((batch, T, width), dtype=dtype, device="cuda").uniform_(-1, 1)
    out = torch.empty((batch, T, width), dtype=dtype, device="cuda")
    grad = ce.embedding_backward_grouped(flat_group, grad_y, idx, offsets, num_hots=hot)
    bias = torch.full((1,), 0.8, dtype=torch.float32, device="cuda")
    r = dict(family=name, tables=T, width=width, batch_per_table=batch, hotness=hot or None, lookups=int(idx.numel()),
             total_rows=int(total), entries=int(grad.last_id.item()) + 1, step_alone={}, whole_step={})

    def flat_step(rule, state):
        if rule == "rowwise_adam":
            return lambda: ce.sparse_row_adam(flat_group.flat, grad.ids, grad.rows, exp_avg=state[0], exp_avg_sq=state[1],
                                              lr=LR, bias_factor=bias, rowwise=True, last_id=grad.last_id)
        return lambda: ce.sparse_row_update(flat_group.flat, grad.ids, grad.rows, rule=rule, lr=LR,
                                            state=state[0] if state else None, last_id=grad.last_id)

    if a.existing_only:
        for rule in RULES:
            state = flat_state(torch, rule, total, width)
            sides = {"flat": flat_step(rule, state)}
            r["step_alone"][rule] = dict(eager=alternate(torch, sides, a.calls, a.rounds, a.warmup),
                                         graph=alternate(torch, {k: captured(torch, f) for k, f in sides.items()}, a.calls,
                                                         a.rounds, a.warmup))
            line(name + " " + rule, "eager", r["step_alone"][rule]["eager"])
            line(name + " " + rule, "graph", r["step_alone"][rule]["graph"])
            del state, sides
        return r

    group = ce.TableGroup([t.clone() for t in flat_group.tables])          # the same tables as separate tensors
    from cuembed_amd import optim
    for rule in RULES:
        state = flat_state(torch, rule, total, width)
        if rule == "sgd":
            updater = optim.GroupSparseUpdater(group, "sgd", LR)
        elif rule == "rowwise_adagrad":
            updater = optim.GroupSparseUpdater(group, rule, LR, initial_accumulator_value=0.1)
        else:
            updater = optim.GroupSparseAdamUpdater(group, LR, rowwise=True)

        def loop(updater=updater, rule=rule):
            for t, (ids, rows) in enumerate(grad.per_table()):           # (the read-back is inside per_table)
                if rule == "rowwise_adam":
                    ce.sparse_row_adam(group.tables[t], ids, rows, exp_avg=updater.exp_avg[t],
                                       exp_avg_sq=updater.exp_avg_sq[t], lr=LR, bias_factor=bias, rowwise=True)
                else:
                    ce.sparse_row_update(group.tables[t], ids, rows, rule=rule, lr=LR,
                                         state=updater.states[t] if updater.states else None)

        if rule == "rowwise_adam":      # (the functions, not updater.apply: no clock launch, as in the other arms)
            def grouped(updater=updater):
                ce.sparse_row_adam_grouped(group, grad.ids, grad.rows, exp_avg=updater.exp_avg,
                                           exp_avg_sq=updater.exp_avg_sq, lr=LR, bias_factor=bias, rowwise=True,
                                           last_id=grad.last_id)
        else:
            def grouped(updater=updater, rule=rule):
                ce.sparse_row_update_grouped(group, grad.ids, grad.rows, rule=rule, lr=LR, states=updater.states,
                                             last_id=grad.last_id)

        sides = {"grouped": grouped, "loop": loop, "flat": flat_step(rule, state)}
        eager = alternate(torch, sides, a.calls, a.rounds, a.warmup)
        graph = alternate(torch, {k: captured(torch, f) for k, f in sides.items() if k != "loop"}, a.calls, a.rounds,
                          a.warmup)
        r["step_alone"][rule] = dict(
            eager=eager, graph=graph,
            verdicts={"eager grouped against loop": verdict(eager["grouped"], eager["loop"]),
                      "eager grouped against flat": verdict(eager["grouped"], eager["flat"]),
                      "graph grouped against flat": verdict(graph["grouped"], graph["flat"]),
                      "graph grouped against eager loop": verdict(graph["grouped"], eager["loop"])})
        line(name + " " + rule, "eager", eager)
        line(name + " " + rule, "graph", graph)
        print("    ", r["step_alone"][rule]["verdicts"], flush=True)
        del state, updater, sides, grouped, loop

    updater = optim.GroupSparseUpdater(group, "sgd", LR)

    def whole_grouped():
        ce.embedding_forward_grouped(group, idx, offsets, num_hots=hot, out=out)
        updater.backward_and_apply(grad_y, idx, offsets)

    def whole_flat():
        ce.embedding_forward_grouped(flat_group, idx, offsets, num_hots=hot, out=out)
        g = ce.embedding_backward_grouped(flat_group, grad_y, idx, offsets, num_hots=hot)
        ce.sparse_row_update(flat_group.flat, g.ids, g.rows, rule="sgd", lr=LR, last_id=g.last_id)

    sides = {"grouped": whole_grouped, "flat": whole_flat}
    eager = alternate(torch, sides, a.calls, a.rounds, a.warmup)
    graph = alternate(torch, {k: captured(torch, f) for k, f in sides.items()}, a.calls, a.rounds, a.warmup)
    r["whole_step"] = dict(rule="sgd", eager=eager, graph=graph,
                           verdicts={"eager grouped against flat": verdict(eager["grouped"], eager["flat"]),
                                     "graph grouped against flat": verdict(graph["grouped"], graph["flat"])})
    line(name + " whole step", "eager", eager)
    line(name + " whole step", "graph", graph)
    print("    ", r["whole_step"]["verdicts"], flush=True)
    assert not ce.capacity_overflowed()
    return r


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--calls", type=int, default=100, help="timed calls per round")
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--small_rows", type=int, default=1_000_000)
    p.add_argument("--large_rows", type=int, default=10_000_000)
    p.add_argument("--families", default="launch,bandwidth", help="comma-separated: launch, bandwidth")
    p.add_argument("--out", default=None, help="write the JSON here as well")
    p.add_argument("--commit", default=None, help="commit the tree was built from (default: git rev-parse)")
    p.add_argument("--existing-only", action="store_true", help="time the one-storage (`flat`) step alone")
    p.add_argument("--stochastic-rounding", action="store_true",
                   help="time the step alone with stochastic rounding: grouped with one seed per table against grouped "
                        "nearest, the per-table loop and the one-storage step")
    p.add_argument("--tree", default=ROOT, help="import cuembed_amd from this checkout (with --existing-only: e.g. the parent's)")
    p.add_argument("--this-existing", default=None,
                   help="the JSON of an --existing-only run of THIS tree: what the parent's runs are compared with "
                        "(default: this run's own `flat` arms)")
    p.add_argument("--parent-existing", nargs="*", default=None,
                   help="the JSON files of --existing-only runs on the parent commit, to record next to this run")
    a = p.parse_args()
    if a.stochastic_rounding and (a.existing_only or a.parent_existing or a.this_existing):
        sys.exit("--stochastic-rounding is a run of its own: not with --existing-only / --parent-existing / --this-existing")
    if a.tree != ROOT and not a.existing_only:
        sys.exit("--tree goes with --existing-only: another checkout has no grouped step to time")
    sys.path.insert(0, os.path.abspath(a.tree))
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("grouped_optimizer_step_benchmark: needs a GPU (there is nothing to time without one)")
    import cuembed_amd as ce
    from cuembed_amd import harness
    from grouped_forward_benchmark import alternate, captured, commit_id
    assert os.path.abspath(ce.__file__).startswith(os.path.abspath(a.tree)), ce.__file__
    torch.manual_seed(1)
    report = dict(tool="benchmarks/grouped_optimizer_step_benchmark.py", commit=commit_id(a.commit),
                  package="this tree" if os.path.abspath(a.tree) == ROOT else "another checkout (--tree)",
                  device=torch.cuda.get_device_name(0),
                  arch=getattr(torch.cuda.get_device_properties(0), "gcnArchName", None), torch=torch.__version__,
                  calls_per_round=a.calls, rounds=a.rounds, existing_only=a.existing_only,
                  stochastic_rounding=a.stochastic_rounding, families=[])
    timers = (alternate, captured)
    families = a.families.split(",")

    if "launch" in families:      # ---- launch-bound: 26 tables, 2,048 ragged bags each
        T, W, B = 26, 128, 2048
        rng = np.random.default_rng(2)
        lengths = rng.integers(0, 41, T * B)
        offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)).cuda()
        idx = torch.from_numpy(rng.integers(0, a.small_rows, int(lengths.sum())).astype(np.int32)).cuda()
        report["families"].append(run_family(torch, ce, a, "launch-bound fp16", (a.small_rows,) * T, W, B, idx, offsets, 0,
                                             timers))
        torch.cuda.empty_cache()
    if "bandwidth" in families:   # ---- bandwidth-bound: 4 tables of 10 M rows, 16,384 samples of 64 lookups each
        T, W, B, H = 4, 256, 16384, 64
        ids = harness.generate_indices(a.large_rows, T * B, H, alpha=1.15).reshape(T, B, H)
        idx = torch.from_numpy(np.ascontiguousarray(ids)).cuda()
        report["families"].append(run_family(torch, ce, a, "bandwidth-bound fp16 alpha=1.15", (a.large_rows,) * T, W, B,
                                             idx, None, H, timers))
    own = report["families"]
    if a.this_existing:                         # like for like: an --existing-only run of this tree, a process like the parent's
        with open(a.this_existing) as f:
            report["existing_step_on_this_tree"] = json.load(f)
        own = report["existing_step_on_this_tree"]["families"]
    report["existing_step_on_the_parent"] = []
    for path in a.parent_existing or ():       # (runs before and after this tree's: the drift of the machine shows)
        with open(path) as f:
            parent = json.load(f)
        verdicts = {}
        for mine, theirs in zip(own, parent["families"]):
            assert mine["family"] == theirs["family"]
            for rule in RULES:
                for how in ("eager", "graph"):
                    verdicts["%s, %s, %s: this tree against the parent" % (mine["family"], rule, how)] = verdict(
                        mine["step_alone"][rule][how]["flat"], theirs["step_alone"][rule][how]["flat"])
        report["existing_step_on_the_parent"].append(dict(commit=parent["commit"], package=parent["package"],
                                                          families=parent["families"], verdicts=verdicts))
        print(json.dumps(verdicts, indent=1))
    text = json.dumps(report, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(dict(summary=[dict(family=f["family"],
                                        step_alone={rule: {how: {k: v["ms"] for k, v in res[how].items()}
                                                           for how in ("eager", "graph")}
                                                    for rule, res in f["step_alone"].items()})
                                   for f in report["families"]])))


if __name__ == "__main__":
    main()
