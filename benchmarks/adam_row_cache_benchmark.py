#!/usr/bin/env python3
"""Times a TRAINING step with the Adam family on a HOST-resident fp16 table (pinned memory, reached over PCIe) on one
GPU -- forward, compressed backward (count on the device) and the Adam step -- for lazy Adam and for row-wise Adam, in
three arrangements:

    cache       AdamRowCache: forward and apply_update through the cache, both moments on the cache slots
    host        table and moments addressed directly in pinned host memory: the forward and the sparse Adam step read
                and write every row over PCIe
    device      table and moments on the device, optim.SparseAdamUpdater (what the cache can at best approach)

The protocol is that of dynamic_row_cache_benchmark.py --leg train, whose table, index stream (power law, alpha = 1.15,
the hot set re-drawn every `--redraw` steps), cache size and helpers this tool takes over: a warm-up pass each, then
`--rounds` interleaved rounds of one pass over all `--steps` batches, ms per step as median [min, max].  For every pair
the verdict is "faster beyond the spread" (the slowest round of one beats the fastest of the other), "slower" (the
reverse) or "the same within the spread".  Before the timed passes the three arrangements run a few steps on SHARED
gradients (one backward per step); whether their forward outputs, tables and moments then hold the same bits (after the
cache's flush) is recorded.  A fill moves 2 * W + 8 * W bytes of a 16-bit row with lazy Adam and 2 * W + 4 * W + 4 with
row-wise Adam; the report states both next to the timings.

    python benchmarks/adam_row_cache_benchmark.py --out profiles/row_cache_adam_timing.json [--commit ID]

--stochastic-rounding times the step THROUGH THE CACHE with its two roundings instead (dynamic_row_cache_benchmark.py's
rounding_legs): `nearest`, AdamRowCache, against `stochastic`, AdamRowCache(stochastic_rounding=True); the bit check's
other side is optim.SparseAdamUpdater(stochastic_rounding=True) with the same seed on a device copy.
"""
import argparse
import ctypes
import gc
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import dynamic_row_cache_benchmark as D  # noqa: E402 - the protocol's helpers

LR, BETAS, EPS = 0.001, (0.9, 0.999), 1e-8


def pinned_copy(torch, t):
    out = torch.empty(t.shape, dtype=t.dtype).pin_memory()
    out.copy_(t)
    return out


def pinned_zeros(torch, shape):
    return torch.zeros(shape, dtype=torch.float32).pin_memory()


def one_rule(torch, ce, a, batches, source_table, rowwise):
    """The three arrangements of one rule: their timings, the cache's counters and the bit check."""
    from cuembed_amd import _lib, ops
    from cuembed_amd.optim import SparseAdamUpdater
    from cuembed_amd.row_cache import AdamRowCache, CachedHostTable
    rule = "rowwise_adam" if rowwise else "adam"
    cap = a.batch * a.hotness
    sq_shape = (a.rows,) if rowwise else (a.rows, a.width)
    cache = AdamRowCache(pinned_copy(torch, source_table), "cuda", num_sets=a.num_sets, rowwise=rowwise, betas=BETAS,
                         eps=EPS)
    direct = dict(table=pinned_copy(torch, source_table), exp_avg=pinned_zeros(torch, (a.rows, a.width)),
                  exp_avg_sq=pinned_zeros(torch, sq_shape))
    direct_powers, direct_bias = ops.new_adam_clock("cuda")
    reader = CachedHostTable(direct["table"], "cuda", capacity_rows=1)          # (its forward with use_cache=False)
    updater = SparseAdamUpdater(source_table.clone(), LR, betas=BETAS, eps=EPS, rowwise=rowwise)
    g = torch.Generator(device="cuda")
    g.manual_seed(a.seed + 1)
    grad_y = (torch.randn((a.batch, a.width), device="cuda", generator=g) * 0.1).to(torch.float16)
    out = torch.empty((a.batch, a.width), dtype=torch.float16, device="cuda")
    grad = torch.empty((cap, a.width), dtype=torch.float16, device="cuda")
    inv = torch.empty((cap,), dtype=torch.int32, device="cuda")

    def backward(idx):
        t_idx, t_sid, _, remap = ce.transpose_fixed_hotness(idx, a.batch, a.hotness, num_categories=a.rows, remapped=True)
        ce.embedding_backward(grad_y, None, t_idx, t_sid, remap, grad_embedding=grad, inverse_mapping=inv)
        return remap[-1:]

    def host_update(last):
        # ops.sparse_row_adam takes device tensors only: the same entry point on the pinned tensors' pointers
        ops.adam_clock_advance(direct_powers, direct_bias, BETAS)
        p = ctypes.c_void_p
        _lib.lib().cuembed_sparse_row_adam(
            p(direct["table"].data_ptr()), ops._ELEM[torch.float16], a.width, p(direct["exp_avg"].data_ptr()),
            p(direct["exp_avg_sq"].data_ptr()), ops.ADAM_RULES[rule], ops._ptr(inv), ops._INDEX[torch.int32],
            ops._ptr(grad), cap, 1, -1, None, 0, ops._ptr(last), LR, None, 1.0, ops._ptr(direct_bias), BETAS[0],
            1.0 - BETAS[0], BETAS[1], 1.0 - BETAS[1], EPS, 0.0, ops._stream(last))

    # every arrangement as (forward, update of the compressed gradient in grad / inv with its last id)
    parts = {
        "cache": (lambda idx: cache.forward(idx, num_hots=a.hotness, out=out),
                  lambda last: cache.apply_update(inv, grad, LR, last_id=last)),
        "host": (lambda idx: reader.forward(idx, num_hots=a.hotness, use_cache=False, out=out), host_update),
        "device": (lambda idx: ce.embedding_forward(updater.table, idx, num_hots=a.hotness, out=out),
                   lambda last: updater.apply(inv, grad, last_id=last)),
    }

    def step_of(name):
        forward, update = parts[name]

        def step(idx):
            forward(idx)
            update(backward(idx))
        return step

    sides = {name: step_of(name) for name in parts}
    # before anything is timed: the three arrangements on SHARED gradients (one backward per step: its sums of
    # duplicates go through atomics, so two calls need not give the same bits) pool and train the same bits.  The
    # steps cross a re-draw of the hot set, so the cache evicts dirty rows and writes them back on the way.
    checked = batches[:min(len(batches), a.redraw + 2)]
    same_forward = True
    for idx in checked:
        pooled = []
        for forward, _ in parts.values():
            forward(idx)
            pooled.append(out.clone())
        same_forward = same_forward and bool(torch.equal(pooled[0], pooled[1]) and torch.equal(pooled[0], pooled[2]))
        last = backward(idx)
        for _, update in parts.values():
            update(last)
    cache.flush()
    torch.cuda.synchronize()
    same_bits = same_forward
    for name, device_side in (("table", updater.table), ("exp_avg", updater.exp_avg), ("exp_avg_sq", updater.exp_avg_sq)):
        through_cache = cache.table if name == "table" else getattr(cache, name)
        same_bits = bool(same_bits and torch.equal(through_cache, direct[name]) and
                         torch.equal(through_cache, device_side.cpu()))
    for fn in sides.values():          # warm-up; the cache reaches its steady state
        D.time_pass(torch, fn, batches)
    before = cache.stats()
    samples = {name: [] for name in sides}
    for _ in range(a.rounds):
        for name, fn in sides.items():
            samples[name].append(D.time_pass(torch, fn, batches))
    after = cache.stats()
    got = {name: D.summarise(v) for name, v in samples.items()}
    steps = a.rounds * a.steps
    per_step = {k: (after[k] - before[k]) / steps for k in ("hits", "misses", "evictions", "write_backs", "unplaced")}
    distinct = per_step["hits"] + per_step["misses"]
    moment_bytes_per_row = 4 * a.width + (4 if rowwise else 4 * a.width)
    for name in sides:
        print("%-13s %-8s %.4f ms / step [%.4f, %.4f]" % (rule, name, got[name]["ms"], got[name]["min"], got[name]["max"]),
              flush=True)
    return dict(step="forward + compressed backward (count on the device) + %s" % ("row-wise Adam" if rowwise else "lazy Adam"),
                bytes_per_fill=dict(row=2 * a.width, moments=moment_bytes_per_row,
                                    times_the_row=(2 * a.width + moment_bytes_per_row) / (2 * a.width)),
                moment_bytes=a.rows * moment_bytes_per_row, cache_bytes=64 * a.num_sets * (2 * a.width + moment_bytes_per_row),
                ms_per_step=got,
                cache_per_step=dict(per_step, hit_rate_of_distinct_rows=per_step["hits"] / max(distinct, 1e-9)),
                cache_against_host=D.verdict(got["cache"], got["host"]),
                cache_against_device=D.verdict(got["cache"], got["device"]),
                host_against_device=D.verdict(got["host"], got["device"]),
                same_bits_on_shared_gradients=dict(steps=len(checked), forward_outputs_tables_and_moments_equal=same_bits))


def one_rule_roundings(torch, ce, a, batches, source_table, rowwise):
    """--stochastic-rounding: one rule through the cache, to nearest and stochastically."""
    from cuembed_amd.optim import SparseAdamUpdater
    from cuembed_amd.row_cache import AdamRowCache

    def make_cache(stochastic):
        kw = dict(stochastic_rounding=True, seed=a.seed) if stochastic else {}
        return AdamRowCache(pinned_copy(torch, source_table), "cuda", num_sets=a.num_sets, rowwise=rowwise, betas=BETAS,
                            eps=EPS, **kw)

    got = D.rounding_legs(torch, ce, a, batches, make_cache,
                          lambda: SparseAdamUpdater(source_table.clone(), LR, betas=BETAS, eps=EPS, rowwise=rowwise,
                                                    stochastic_rounding=True, seed=a.seed), LR)
    return dict(step="forward + compressed backward (count on the device) + %s, through the cache"
                     % ("row-wise Adam" if rowwise else "lazy Adam"), **got)


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--rows", type=int, default=1 << 22, help="table rows (a power of two)")
    p.add_argument("--width", type=int, default=128)
    p.add_argument("--batch", type=int, default=16384)
    p.add_argument("--hotness", type=int, default=32)
    p.add_argument("--num_sets", type=int, default=4096, help="sets of 64 ways: the cache holds 64 * num_sets rows")
    p.add_argument("--alpha", type=float, default=1.15)
    p.add_argument("--steps", type=int, default=40, help="batches per pass")
    p.add_argument("--redraw", type=int, default=10, help="the hot set is re-drawn every this many steps")
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--seed", type=int, default=1)
    p.add_argument("--rule", choices=("both", "adam", "rowwise_adam"), default="both")
    p.add_argument("--stochastic-rounding", action="store_true",
                   help="the step through the cache with round to nearest against stochastic rounding")
    p.add_argument("--out", default=None, help="write the JSON here as well")
    p.add_argument("--commit", default=None, help="commit the tree was built from (default: git rev-parse)")
    a = p.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("adam_row_cache_benchmark: needs a GPU (there is nothing to time without one)")
    if a.rows & (a.rows - 1):
        sys.exit("--rows must be a power of two (the rank -> row map is an affine permutation mod rows)")
    import cuembed_amd as ce

    torch.manual_seed(a.seed)
    source_table = torch.empty((a.rows, a.width), dtype=torch.float16, device="cuda").uniform_(-1, 1)
    batches = D.make_batches(torch, a)
    rules = {}
    for rule in (("adam", "rowwise_adam") if a.rule == "both" else (a.rule,)):
        rules[rule] = (one_rule_roundings if a.stochastic_rounding else one_rule)(torch, ce, a, batches, source_table,
                                                                                   rowwise=rule == "rowwise_adam")
        gc.collect()                       # the pinned tables and moments of one rule go before the next one's come
        torch.cuda.empty_cache()
    capacity = 64 * a.num_sets
    tool = "benchmarks/adam_row_cache_benchmark.py" + (" --stochastic-rounding" if a.stochastic_rounding else "")
    report = dict(tool=tool, commit=D.commit_id(a.commit),
                  device=torch.cuda.get_device_name(0), torch=torch.__version__,
                  shape=dict(rows=a.rows, width=a.width, dtype="float16", batch=a.batch, hotness=a.hotness, alpha=a.alpha,
                             steps_per_pass=a.steps, hot_set_redrawn_every=a.redraw, cache_rows=capacity,
                             num_sets=a.num_sets, table_bytes=a.rows * a.width * 2),
                  hyper_parameters=dict(lr=LR, betas=BETAS, eps=EPS, weight_decay=0.0), rounds=a.rounds, rules=rules)
    text = json.dumps(report, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    if a.stochastic_rounding:
        print(json.dumps({rule: dict(summary={k: v["ms"] for k, v in r["ms_per_step"].items()},
                                     stochastic_against_nearest=r["stochastic_against_nearest"],
                                     same_bits=r["same_bits_as_the_stochastic_updater"]["forward_outputs_and_tables_equal"])
                          for rule, r in rules.items()}))
        return
    print(json.dumps({rule: dict(summary={k: r["ms_per_step"][k]["ms"] for k in r["ms_per_step"]},
                                 cache_against_host=r["cache_against_host"],
                                 cache_against_device=r["cache_against_device"],
                                 same_bits=r["same_bits_on_shared_gradients"]["forward_outputs_tables_and_moments_equal"])
                      for rule, r in rules.items()}))


if __name__ == "__main__":
    main()
