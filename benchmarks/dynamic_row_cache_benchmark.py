#!/usr/bin/env python3
"""Times the forward on a HOST-resident fp16 table (pinned memory, read over PCIe) four ways on one GPU:

    (a) host        CachedHostTable.forward(use_cache=False): every row over PCIe
    (b) static      CachedHostTable with cache_most_frequent() computed ONCE, on the first epoch's indices
    (c) dynamic     DynamicRowCache.forward in steady state: prefetch (sort, probe, place, row exchange) + translate +
                    forward, every step
    (d) device      embedding_forward on a device-resident copy of the table (what the cache can at best approach)

The index stream is a power law (alpha = 1.15, the reference generator's inverse-CDF recipe, drawn on the device) over
ranks; rank -> row is an affine permutation whose shift is RE-DRAWN every `--redraw` steps, so the hot set moves: (b)'s
rows go cold after the first epoch, (c) follows.  Every side walks the same pre-generated batches in the same order.

Per side: `--rounds` rounds of one pass over all `--steps` batches, one pair of device events around the pass; the
figure is ms per step, median and min over the rounds with the spread (max - min) next to it.  A side is called faster
only when its slowest round beats the other's fastest.  Hit rates: (c) from the cache's device counters over the timed
passes (distinct rows), (b) from slot_of_row per epoch (lookups).

    python benchmarks/dynamic_row_cache_benchmark.py --out profiles/dynamic_row_cache_timing.json [--commit ID]

--leg train times a TRAINING step instead -- forward, compressed backward (count on the device) and row-wise Adagrad --
on the same stream, in three arrangements:

    cache       DynamicRowCache(rule="rowwise_adagrad"): forward and apply_update through the cache, the state on the
                cache slots
    host        table and state addressed directly in pinned host memory: the forward and the sparse step read and
                write every row over PCIe
    device      table and state on the device (what the cache can at best approach)

Same protocol: a warm-up pass each, then `--rounds` interleaved rounds of one pass, ms per step as median [min, max].  For
every pair the verdict is "faster beyond the spread" (the slowest round of one beats the fastest of the other), "slower"
(the reverse) or "the same within the spread".  Before the timed passes the three arrangements run a few steps on SHARED
gradients (one backward per step); whether their forward outputs, tables and states then hold the same bits (after the
cache's flush) is recorded.

    python benchmarks/dynamic_row_cache_benchmark.py --leg train --out profiles/row_cache_state_timing.json [--commit ID]

--leg train --stochastic-rounding times the same training step THROUGH THE CACHE with its two roundings instead: `nearest`,
DynamicRowCache(rule="rowwise_adagrad"), against `stochastic`, the same cache with stochastic_rounding=True (the named
step: one more id array, and one widening launch for the int32 ids).  Same table, stream, cache size, warm-up and
interleaved rounds; the verdict is worded the same way.  Before the timed passes the stochastic cache and
optim.SparseUpdater(stochastic_rounding=True) with the same seed on a device copy run a few steps on shared gradients;
whether they then hold the same bits is recorded.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def power_law_ranks(torch, rows, count, alpha, generator):
    """Ranks in [0, rows) with P(rank) ~ (rank + 1) ** -alpha: x = (u * (rows ** (1 - alpha) - 1) + 1) ** (1 / (1 -
    alpha)), rank = floor(x) - 1 (the reference generator's recipe, in float64 on the device)."""
    u = torch.rand((count,), dtype=torch.float64, device="cuda", generator=generator)
    x = (u * (float(rows) ** (1.0 - alpha) - 1.0) + 1.0) ** (1.0 / (1.0 - alpha))
    return (x.floor().long() - 1).clamp_(0, rows - 1)


def make_batches(torch, a):
    """`steps` batches [batch, hotness] int32; the rank -> row shift changes every `redraw` steps."""
    g = torch.Generator(device="cuda")
    g.manual_seed(a.seed)
    stride = 2_654_435_761 % a.rows | 1          # odd; rows is checked to be a power of two, so this is a permutation
    batches, shifts = [], []
    for step in range(a.steps):
        if step % a.redraw == 0:
            shifts.append(int(torch.randint(0, a.rows, (1,), generator=g, device="cuda").item()))
        ranks = power_law_ranks(torch, a.rows, a.batch * a.hotness, a.alpha, g)
        batches.append(((ranks * stride + shifts[-1]) % a.rows).to(torch.int32).reshape(a.batch, a.hotness))
    return batches


def time_pass(torch, fn, batches):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for idx in batches:
        fn(idx)
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / len(batches)


def summarise(v):
    return dict(ms=statistics.median(v), min=min(v), max=max(v), spread=max(v) - min(v), rounds=v)


def commit_id(given):
    if given:
        return given
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stdout=subprocess.PIPE,
                              stderr=subprocess.DEVNULL, text=True, check=True).stdout.strip()
    except Exception:  # noqa: BLE001 - a source tree without its history
        return "unknown"


def verdict(x, y):
    """How side x did against side y, from their rounds."""
    if x["max"] < y["min"]:
        return "faster beyond the spread"
    if y["max"] < x["min"]:
        return "slower"
    return "the same within the spread"


def rounding_legs(torch, ce, a, batches, make_cache, make_updater, lr):
    """--stochastic-rounding: the training step through the cache with round to nearest and with stochastic rounding.
    make_cache(stochastic) -> a cache on a pinned table of its own; make_updater() -> the stochastic updater on a device
    copy, the bit check's other side.  Returns the report of one rule."""
    cap = a.batch * a.hotness
    caches = {"nearest": make_cache(False), "stochastic": make_cache(True)}
    updater = make_updater()
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

    def step_of(cache):
        def step(idx):
            cache.forward(idx, num_hots=a.hotness, out=out)
            cache.apply_update(inv, grad, lr, last_id=backward(idx))
        return step

    # before anything is timed: the stochastic cache and the stochastic updater on SHARED gradients, across a re-draw
    checked = batches[:min(len(batches), a.redraw + 2)]
    same_bits = True
    for idx in checked:
        caches["stochastic"].forward(idx, num_hots=a.hotness, out=out)
        same_bits = same_bits and bool(torch.equal(out, ce.embedding_forward(updater.table, idx, num_hots=a.hotness)))
        last = backward(idx)
        caches["stochastic"].apply_update(inv, grad, lr, last_id=last)
        updater.apply(inv, grad, last_id=last)
    caches["stochastic"].flush()
    torch.cuda.synchronize()
    same_bits = bool(same_bits and torch.equal(caches["stochastic"].table, updater.table.cpu()) and
                     int(caches["stochastic"].rounding_step) == int(updater.rounding_step) == len(checked))
    del updater
    sides = {name: step_of(cache) for name, cache in caches.items()}
    for fn in sides.values():          # warm-up; the caches reach their steady state
        time_pass(torch, fn, batches)
    samples = {name: [] for name in sides}
    for _ in range(a.rounds):
        for name, fn in sides.items():
            samples[name].append(time_pass(torch, fn, batches))
    got = {name: summarise(v) for name, v in samples.items()}
    for name in sides:
        print("%-10s %.4f ms / step [%.4f, %.4f]" % (name, got[name]["ms"], got[name]["min"], got[name]["max"]), flush=True)
    return dict(ms_per_step=got, stochastic_against_nearest=verdict(got["stochastic"], got["nearest"]),
                same_bits_as_the_stochastic_updater=dict(steps=len(checked), forward_outputs_and_tables_equal=same_bits))


def stochastic_training_leg(torch, ce, a, batches, host_table, device_table):
    """--leg train --stochastic-rounding: row-wise Adagrad through the cache, to nearest and stochastically."""
    from cuembed_amd.optim import SparseUpdater
    from cuembed_amd.row_cache import DynamicRowCache
    rule, lr, eps = "rowwise_adagrad", 0.01, 1e-8

    def make_cache(stochastic):
        table = torch.empty_like(host_table).pin_memory()
        table.copy_(host_table)
        kw = dict(stochastic_rounding=True, seed=a.seed) if stochastic else {}
        return DynamicRowCache(table, "cuda", num_sets=a.num_sets, rule=rule, eps=eps, **kw)

    got = rounding_legs(torch, ce, a, batches, make_cache,
                        lambda: SparseUpdater(device_table, rule, lr, eps=eps, stochastic_rounding=True, seed=a.seed), lr)
    capacity = 64 * a.num_sets
    report = dict(tool="benchmarks/dynamic_row_cache_benchmark.py --leg train --stochastic-rounding",
                  commit=commit_id(a.commit), device=torch.cuda.get_device_name(0), torch=torch.__version__,
                  step="forward + compressed backward (count on the device) + row-wise Adagrad, through the cache",
                  shape=dict(rows=a.rows, width=a.width, dtype="float16", batch=a.batch, hotness=a.hotness, alpha=a.alpha,
                             steps_per_pass=a.steps, hot_set_redrawn_every=a.redraw, cache_rows=capacity,
                             num_sets=a.num_sets, table_bytes=a.rows * a.width * 2), rounds=a.rounds, **got)
    text = json.dumps(report, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(dict(summary={k: v["ms"] for k, v in got["ms_per_step"].items()},
                          stochastic_against_nearest=got["stochastic_against_nearest"],
                          same_bits=got["same_bits_as_the_stochastic_updater"]["forward_outputs_and_tables_equal"])))


def training_leg(torch, ce, a, batches, host_table, device_table):
    """Forward + backward + row-wise Adagrad per step, through the cache, directly in host memory and on the device."""
    import ctypes
    from cuembed_amd import _lib, ops
    from cuembed_amd.row_cache import CachedHostTable, DynamicRowCache
    rule, lr, eps = "rowwise_adagrad", 0.01, 1e-8
    cap = a.batch * a.hotness
    direct_table = torch.empty_like(host_table).pin_memory()
    direct_table.copy_(host_table)
    direct_state = torch.zeros((a.rows,), dtype=torch.float32).pin_memory()
    device_state = torch.zeros((a.rows,), dtype=torch.float32, device="cuda")
    cache = DynamicRowCache(host_table, "cuda", num_sets=a.num_sets, rule=rule, eps=eps)
    reader = CachedHostTable(direct_table, "cuda", capacity_rows=1)          # (its forward with use_cache=False)
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

    # every arrangement as (forward, update of the compressed gradient in grad / inv with its last id)
    def host_update(last):
        # ops.sparse_row_update takes device tensors only: the same entry point on the pinned tensors' pointers
        _lib.lib().cuembed_sparse_row_update(
            ctypes.c_void_p(direct_table.data_ptr()), ops._ELEM[torch.float16], a.width,
            ctypes.c_void_p(direct_state.data_ptr()), ops.UPDATE_RULES[rule], ops._ptr(inv), ops._INDEX[torch.int32],
            ops._ptr(grad), cap, 1, -1, None, 0, ops._ptr(last), lr, None, eps, ops._stream(last))

    parts = {
        "cache": (lambda idx: cache.forward(idx, num_hots=a.hotness, out=out),
                  lambda last: cache.apply_update(inv, grad, lr, last_id=last)),
        "host": (lambda idx: reader.forward(idx, num_hots=a.hotness, use_cache=False, out=out), host_update),
        "device": (lambda idx: ce.embedding_forward(device_table, idx, num_hots=a.hotness, out=out),
                   lambda last: ce.sparse_row_update(device_table, inv, grad, rule=rule, state=device_state, lr=lr, eps=eps,
                                                     last_id=last)),
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
    same_bits = bool(same_forward and torch.equal(host_table, direct_table) and
                     torch.equal(host_table, device_table.cpu()) and torch.equal(cache.state, direct_state) and
                     torch.equal(cache.state, device_state.cpu()))
    for fn in sides.values():          # warm-up; the cache reaches its steady state
        time_pass(torch, fn, batches)
    before = cache.stats()
    samples = {name: [] for name in sides}
    for _ in range(a.rounds):
        for name, fn in sides.items():
            samples[name].append(time_pass(torch, fn, batches))
    after = cache.stats()
    got = {name: summarise(v) for name, v in samples.items()}
    steps = a.rounds * a.steps
    per_step = {k: (after[k] - before[k]) / steps for k in ("hits", "misses", "evictions", "write_backs", "unplaced")}
    distinct = per_step["hits"] + per_step["misses"]
    capacity = 64 * a.num_sets
    report = dict(tool="benchmarks/dynamic_row_cache_benchmark.py --leg train", commit=commit_id(a.commit),
                  device=torch.cuda.get_device_name(0), torch=torch.__version__,
                  step="forward + compressed backward (count on the device) + row-wise Adagrad",
                  shape=dict(rows=a.rows, width=a.width, dtype="float16", batch=a.batch, hotness=a.hotness, alpha=a.alpha,
                             steps_per_pass=a.steps, hot_set_redrawn_every=a.redraw, cache_rows=capacity,
                             num_sets=a.num_sets, table_bytes=a.rows * a.width * 2, state_bytes=a.rows * 4,
                             cache_bytes=capacity * (a.width * 2 + 4)),
                  rounds=a.rounds, ms_per_step=got,
                  cache_per_step=dict(per_step, hit_rate_of_distinct_rows=per_step["hits"] / max(distinct, 1e-9)),
                  cache_against_host=verdict(got["cache"], got["host"]),
                  cache_against_device=verdict(got["cache"], got["device"]),
                  host_against_device=verdict(got["host"], got["device"]),
                  same_bits_on_shared_gradients=dict(steps=len(checked), forward_outputs_tables_and_states_equal=same_bits))
    for name in sides:
        print("%-8s %.4f ms / step [%.4f, %.4f]" % (name, got[name]["ms"], got[name]["min"], got[name]["max"]), flush=True)
    text = json.dumps(report, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(dict(summary={k: got[k]["ms"] for k in got}, cache_against_host=report["cache_against_host"],
                          cache_against_device=report["cache_against_device"], same_bits=same_bits)))


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
    p.add_argument("--leg", choices=("forward", "train"), default="forward",
                   help="forward: the four forwards (default); train: forward + backward + row-wise Adagrad, three ways")
    p.add_argument("--stochastic-rounding", action="store_true",
                   help="with --leg train: the step through the cache with round to nearest against stochastic rounding")
    p.add_argument("--out", default=None, help="write the JSON here as well")
    p.add_argument("--commit", default=None, help="commit the tree was built from (default: git rev-parse)")
    a = p.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("dynamic_row_cache_benchmark: needs a GPU (there is nothing to time without one)")
    if a.rows & (a.rows - 1):
        sys.exit("--rows must be a power of two (the rank -> row map is an affine permutation mod rows)")
    import cuembed_amd as ce
    from cuembed_amd.row_cache import CachedHostTable, DynamicRowCache

    torch.manual_seed(a.seed)
    device_table = torch.empty((a.rows, a.width), dtype=torch.float16, device="cuda").uniform_(-1, 1)
    host_table = torch.empty((a.rows, a.width), dtype=torch.float16).pin_memory()
    host_table.copy_(device_table)
    batches = make_batches(torch, a)
    if a.stochastic_rounding and a.leg != "train":
        sys.exit("--stochastic-rounding goes with --leg train")
    if a.leg == "train" and a.stochastic_rounding:
        return stochastic_training_leg(torch, ce, a, batches, host_table, device_table)
    if a.leg == "train":
        return training_leg(torch, ce, a, batches, host_table, device_table)
    capacity = 64 * a.num_sets
    static = CachedHostTable(host_table, "cuda", capacity_rows=capacity)
    static.cache_most_frequent(torch.cat([b.reshape(-1) for b in batches[:a.redraw]]))
    dynamic = DynamicRowCache(host_table, "cuda", num_sets=a.num_sets)
    out = torch.empty((a.batch, a.width), dtype=torch.float16, device="cuda")
    sides = {
        "host": lambda idx: static.forward(idx, num_hots=a.hotness, use_cache=False, out=out),
        "static": lambda idx: static.forward(idx, num_hots=a.hotness, out=out),
        "dynamic": lambda idx: dynamic.forward(idx, num_hots=a.hotness, out=out),
        "device": lambda idx: ce.embedding_forward(device_table, idx, num_hots=a.hotness, out=out),
    }
    # every side gives the device table's bits
    want = ce.embedding_forward(device_table, batches[0], num_hots=a.hotness)
    for name, fn in sides.items():
        assert torch.equal(fn(batches[0]), want), name
    # warm-up: one pass each (the dynamic cache reaches its steady state: the pass ends where the next one begins)
    for fn in sides.values():
        time_pass(torch, fn, batches)
    before = dynamic.stats()
    samples = {name: [] for name in sides}
    for _ in range(a.rounds):
        for name, fn in sides.items():
            samples[name].append(time_pass(torch, fn, batches))
    after = dynamic.stats()
    got = {name: summarise(v) for name, v in samples.items()}

    distinct = (after["hits"] - before["hits"]) + (after["misses"] - before["misses"])
    dynamic_rates = dict(distinct_rows_per_step=distinct / (a.rounds * a.steps),
                         hit_rate_of_distinct_rows=(after["hits"] - before["hits"]) / max(distinct, 1),
                         evictions_per_step=(after["evictions"] - before["evictions"]) / (a.rounds * a.steps),
                         unplaced_per_step=(after["unplaced"] - before["unplaced"]) / (a.rounds * a.steps))
    lookup_hits = {"static": [], "dynamic_after_prefetch": []}
    for epoch in range(0, a.steps, a.redraw):
        idx = batches[epoch + a.redraw // 2].reshape(-1).long()
        lookup_hits["static"].append(float((static.slot_of_row[idx] >= 0).float().mean()))
        dynamic.prefetch(batches[epoch + a.redraw // 2])
        lookup_hits["dynamic_after_prefetch"].append(float((dynamic.slot_of_row[idx] >= 0).float().mean()))

    def faster(x, y):
        return got[x]["max"] < got[y]["min"]

    report = dict(tool="benchmarks/dynamic_row_cache_benchmark.py", commit=commit_id(a.commit),
                  device=torch.cuda.get_device_name(0), torch=torch.__version__,
                  shape=dict(rows=a.rows, width=a.width, dtype="float16", batch=a.batch, hotness=a.hotness, alpha=a.alpha,
                             steps_per_pass=a.steps, hot_set_redrawn_every=a.redraw, cache_rows=capacity,
                             num_sets=a.num_sets, table_bytes=a.rows * a.width * 2, cache_bytes=capacity * a.width * 2),
                  rounds=a.rounds, ms_per_step=got, dynamic_cache=dynamic_rates, share_of_lookups_served_from_hbm=lookup_hits,
                  dynamic_over_host=got["dynamic"]["ms"] / got["host"]["ms"],
                  dynamic_over_device=got["dynamic"]["ms"] / got["device"]["ms"],
                  dynamic_over_static=got["dynamic"]["ms"] / got["static"]["ms"],
                  dynamic_faster_than_host_beyond_the_spread=faster("dynamic", "host"),
                  host_faster_than_dynamic_beyond_the_spread=faster("host", "dynamic"),
                  dynamic_faster_than_static_beyond_the_spread=faster("dynamic", "static"),
                  static_faster_than_dynamic_beyond_the_spread=faster("static", "dynamic"))
    for name in sides:
        print("%-8s %.4f ms / step (min %.4f, spread %.4f)" % (name, got[name]["ms"], got[name]["min"], got[name]["spread"]),
              flush=True)
    text = json.dumps(report, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(dict(summary={k: got[k]["ms"] for k in got}, dynamic=dynamic_rates,
                          dynamic_over_host=report["dynamic_over_host"], dynamic_over_device=report["dynamic_over_device"])))


if __name__ == "__main__":
    main()
