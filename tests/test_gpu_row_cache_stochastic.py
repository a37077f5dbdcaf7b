"""Stochastic rounding through the row cache on the GPU: DynamicRowCache / AdamRowCache(stochastic_rounding=True,
seed=...) -- the named sparse step, which carries the batch's own ids next to the translated ones to name the rounding
bits -- against optim.SparseUpdater / SparseAdamUpdater(stochastic_rounding=True) with the same seed on device copies,
and against the host reference tests/stochastic_rounding_reference.py, BIT FOR BIT: the bits are a function of (seed,
step, table row, column) only, both sides run one walk with one launch shape on the same gradient tensor, and a cached
plane is a whole number of rows from its home tensor.  Placement is compared with
tests/dynamic_row_cache_reference.CacheModel.  Tiny shapes: 300 or 5,000 rows, 1 or 4 sets of 64 ways."""
import contextlib

import numpy as np
import pytest
import torch

import dynamic_row_cache_reference as M
import row_cache_state_reference as RS
import row_cache_stochastic_reference as N
import stochastic_rounding_reference as S

pytestmark = pytest.mark.gpu

DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16}
KIND = {"f16": "fp16", "bf16": "bf16"}          # (the names of stochastic_rounding_reference)
INDEX = {"i32": torch.int32, "i64": torch.int64}
RULES = ("sgd", "adagrad", "rowwise_adagrad", "adam", "rowwise_adam")
ADAMS = ("adam", "rowwise_adam")
LR, INIT, SEED = 0.0371, 0.5, 0xC0FFEE1234567
# 50: 4-byte lanes; 100: 8-byte lanes; 256: one slice per lane, two entries in flight; 1000: four slices per lane;
# 2056: the run-time loop (257 lanes of 16 bytes) -- the WIDTHS of test_gpu_stochastic_rounding.py
BODIES = [("f16", w) for w in (50, 100, 256, 1000, 2056)] + [("bf16", 256), ("bf16", 2056)]


@contextlib.contextmanager
def no_read_back():
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        yield
    finally:
        torch.cuda.set_sync_debug_mode("default")


def normal_table(kind, width, rows, seed=7):
    """Standard normal values rounded to the type: no update is representable."""
    rng = np.random.default_rng(seed)
    return torch.from_numpy(rng.standard_normal((rows, width)).astype(np.float32)).to(DTYPES[kind]).pin_memory()


def make_cache(rule, table, num_sets, **kw):
    from cuembed_amd.row_cache import AdamRowCache, DynamicRowCache
    if rule in ADAMS:
        return AdamRowCache(table, "cuda", num_sets=num_sets, rowwise=rule == "rowwise_adam", **kw)
    return DynamicRowCache(table, "cuda", num_sets=num_sets, rule=rule, initial_accumulator_value=INIT, **kw)


def make(rule, table, num_sets, lr=LR, seed=SEED):
    """(cache, updater): the stochastic cache on `table` and its oracle, the stochastic updater with the same seed on a
    device copy."""
    from cuembed_amd.optim import SparseAdamUpdater, SparseUpdater
    kw = dict(stochastic_rounding=True, seed=seed)
    d_table = table.cuda()
    cache = make_cache(rule, table, num_sets, **kw)
    if rule in ADAMS:
        updater = SparseAdamUpdater(d_table, lr, rowwise=rule == "rowwise_adam", **kw)
    else:
        updater = SparseUpdater(d_table, rule, lr, initial_accumulator_value=INIT, **kw)
    return cache, updater


def planes(owner, rule):
    """The table and the rule's state tensors of a cache (host side) or an updater (device side), by name."""
    out = dict(table=owner.table)
    if rule in ADAMS:
        out.update(exp_avg=owner.exp_avg, exp_avg_sq=owner.exp_avg_sq)
    elif rule != "sgd":
        out.update(state=owner.state)
    return out


def assert_planes_equal(cache, updater, rule):
    want = planes(updater, rule)
    for name, got in planes(cache, rule).items():
        assert torch.equal(got, want[name].cpu()), name


def randn(shape, dtype, generator):
    return torch.randn(shape, device="cuda", generator=generator).to(dtype)


def seeded(seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return g


def counters(cache):
    stats = cache.stats()
    return {k: stats[k] for k in M.COUNTERS}


def dev(bits, kind):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).view(DTYPES[kind]).cuda()


def pinned(bits, kind):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16).copy()).view(DTYPES[kind]).pin_memory()


def pat(t):
    return t.detach().contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def clean_exit():
    import cuembed_amd as ce
    torch.cuda.synchronize()
    assert ce._lib.lib().cuembed_peek_last_error() == 0


# ---- 1. training parity -----------------------------------------------------------------------------------------
TRAINING_CASES = [dict(width=24, num_sets=1, index="i32"), dict(width=8, num_sets=4, index="i64")]


@pytest.mark.parametrize("kind", ["f16", "bf16"])
@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("case", TRAINING_CASES, ids=lambda c: "w%d-s%d-%s" % (c["width"], c["num_sets"], c["index"]))
def test_training_through_the_cache_equals_training_on_the_device(case, rule, kind):
    """Five steps of forward, compressed backward (count on the device) and the rule, with stochastic rounding on both
    sides.  One set: some rows find no way and are updated over PCIe, where name and placed id are one number; int32
    ids: the names are widened."""
    import cuembed_amd as ce
    table = normal_table(kind, case["width"], M.ROWS)
    nearest = make_cache(rule, table.clone().pin_memory(), case["num_sets"])
    cache, updater = make(rule, table, case["num_sets"])
    assert cache.rounding_step.dtype == torch.int64 and cache.rounding_step.is_cuda and cache.rounding_step.item() == 0
    assert nearest.rounding_step is None
    cap, gen = M.BATCH * M.HOTS, seeded(3)
    index = INDEX[case["index"]]
    for idx in RS.training_batches():
        d_idx = torch.from_numpy(idx).to(index).cuda()
        grad_y = randn((M.BATCH, case["width"]), table.dtype, gen)
        t_idx, t_sid, _, remap = ce.transpose_fixed_hotness(d_idx, M.BATCH, M.HOTS, num_categories=M.ROWS, remapped=True)
        grad = torch.empty((cap, case["width"]), dtype=table.dtype, device="cuda")
        inv = torch.empty((cap,), dtype=index, device="cuda")
        ce.embedding_backward(grad_y, None, t_idx, t_sid, remap, grad_embedding=grad, inverse_mapping=inv)
        want = ce.embedding_forward(updater.table, d_idx, num_hots=M.HOTS)
        updater.apply(inv, grad, last_id=remap[-1:])
        with no_read_back():
            got = cache.forward(d_idx, num_hots=M.HOTS)
            cache.apply_update(inv, grad, LR, last_id=remap[-1:])
            nearest.forward(d_idx, num_hots=M.HOTS)
            nearest.apply_update(inv, grad, LR, last_id=remap[-1:])
        assert torch.equal(got, want)
    # rounding does not change placement
    model = RS.training_placement(case["num_sets"])
    for c in (cache, nearest):
        assert counters(c) == model.counters and c.stats()["overflow"] == 0
        assert np.array_equal(c.dirty.cpu().numpy(), model.dirty) and model.dirty.sum() > 0
        assert np.array_equal(c.slot_of_row.cpu().numpy(), model.slot_of_row)
    assert (model.counters["unplaced"] > 0) == (case["num_sets"] == 1) and model.counters["write_backs"] > 0
    assert cache.rounding_step.item() == updater.rounding_step.item() == RS.TRAINING_STEPS
    with no_read_back():
        cache.flush()
        nearest.flush()
    torch.cuda.synchronize()
    assert_planes_equal(cache, updater, rule)
    assert not torch.equal(cache.table, nearest.table)         # the option did something
    clean_exit()


# ---- 2. every body of the walk ----------------------------------------------------------------------------------
BODY_ROWS = 300
BODY_OTHERS = (np.arange(200, 232), np.arange(232, 264))


def body_ids():
    """101 distinct ids outside the rows the forwards read, in no order: the 64 smallest find a way, 37 do not."""
    rng = np.random.default_rng(101)
    free = np.setdiff1d(np.arange(BODY_ROWS), np.concatenate(BODY_OTHERS))
    return rng.permutation(free)[:101].astype(np.int64)


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("kind, width", BODIES, ids=lambda v: str(v))
def test_every_body_of_the_walk(kind, width, rule):
    """Two steps on 101 ids (an odd count: one group's second in-flight entry is dead) behind one set: 64 are cached, 37
    stay in host memory.  Between the steps the cache reads 64 other rows -- 32, the other 32, then the first 32 again,
    so that the ways' stamps are out of order -- which evicts every updated row dirty: in step two it is in another slot
    than in step one, or in host memory."""
    table = normal_table(kind, width, BODY_ROWS, seed=width)
    cache, updater = make(rule, table, 1)
    ids = body_ids()
    d_ids = torch.from_numpy(ids).cuda()
    gen = seeded(width)
    model = M.CacheModel(BODY_ROWS, 1)
    others = [torch.from_numpy(rows).cuda().reshape(-1, 1) for rows in BODY_OTHERS]
    seen = []
    for step in range(2):
        grad = randn((ids.size, width), table.dtype, gen)
        updater.apply(d_ids, grad)
        with no_read_back():
            cache.apply_update(d_ids, grad, LR)
        model.prefetch(ids, for_update=True)
        seen.append(cache.slot_of_row.cpu().numpy()[ids])
        assert np.array_equal(seen[-1], model.slot_of_row[ids])
        if step == 0:
            for k in (0, 1, 0):
                with no_read_back():
                    cache.forward(others[k], num_hots=1)
                model.prefetch(BODY_OTHERS[k])
            assert int((cache.slot_of_row[d_ids] >= 0).sum()) == 0 and cache.stats()["write_backs"] == 64
    first, second = seen
    assert int((first >= 0).sum()) == 64 and int((second >= 0).sum()) == 64
    assert np.array_equal(first >= 0, second >= 0) and not (first[first >= 0] == second[first >= 0]).any()
    assert counters(cache) == model.counters
    with no_read_back():
        cache.flush()
    torch.cuda.synchronize()
    assert_planes_equal(cache, updater, rule)
    assert cache.rounding_step.item() == updater.rounding_step.item() == 2
    clean_exit()


# ---- 3. the names are the table rows ----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["f16", "bf16"])
def test_the_names_are_the_table_rows(kind):
    """SGD against the host reference alone (no updater): ten rows read first hold ways 0 to 9, so no updated row sits in
    the slot of its own number; tests/test_row_cache_stochastic_host.py shows that bits drawn for the slot give another
    table."""
    from cuembed_amd.row_cache import DynamicRowCache
    table_bits, ids, grads = N.problem(KIND[kind])
    table = pinned(table_bits, kind)
    cache = DynamicRowCache(table, "cuda", num_sets=1, stochastic_rounding=True, seed=N.SEED)
    d_ids, read = torch.from_numpy(ids).cuda(), torch.from_numpy(N.READ).cuda().reshape(-1, 1)
    d_grads = [dev(grads[step], kind) for step in range(N.STEPS)]
    with no_read_back():
        cache.forward(read, num_hots=1)
        for step in range(N.STEPS):
            cache.apply_sgd(d_ids, d_grads[step], N.LR)
    slots = cache.slot_of_row.cpu().numpy()
    assert np.array_equal(slots[N.READ], np.arange(10)) and np.array_equal(slots[ids], N.slots(ids))
    assert not (slots[ids] == ids).any()
    with no_read_back():
        cache.flush()
    torch.cuda.synchronize()
    assert np.array_equal(pat(table), N.trained(KIND[kind]))      # the whole table: unnamed rows are untouched
    assert cache.rounding_step.item() == N.STEPS
    clean_exit()


# ---- 4. placement does not show ---------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", ["rowwise_adagrad", "adam"])
def test_placement_does_not_show(rule):
    """The same five gradient steps through one set (rows without a way, evictions) and through four: the same bits."""
    results = []
    for num_sets in (1, 4):
        table = normal_table("bf16", 24, M.ROWS)
        cache = make_cache(rule, table, num_sets, stochastic_rounding=True, seed=SEED)
        gen = seeded(11)
        for idx in RS.training_batches():
            ids = torch.from_numpy(np.unique(idx)).cuda()
            grad = randn((ids.numel(), 24), table.dtype, gen)
            with no_read_back():
                cache.apply_update(ids, grad, LR)
        with no_read_back():
            cache.flush()
        torch.cuda.synchronize()
        results.append(cache)
    one, four = results
    assert one.stats()["unplaced"] > 0 and four.stats()["unplaced"] == 0
    for name, got in planes(one, rule).items():
        assert torch.equal(got, planes(four, rule)[name]), name
    assert not torch.equal(one.table, normal_table("bf16", 24, M.ROWS))
    assert one.rounding_step.item() == four.rounding_step.item() == RS.TRAINING_STEPS
    clean_exit()


# ---- 5. the symptom and the cure, through the cache -------------------------------------------------------------
@pytest.mark.parametrize("kind", ["f16", "bf16"])
def test_the_512_step_walk_through_the_cache(kind):
    """512 SGD steps of 1/64 of a spacing on rows 0 to 63 of a table of ones: to nearest the table never moves, with
    stochastic rounding it is the reference's walk.  Ten other rows are read first, so that no row of the walk sits in
    the slot of its own number."""
    from cuembed_amd.row_cache import DynamicRowCache
    k = KIND[kind]
    tables = [torch.ones((256, S.WALK_WIDTH), dtype=DTYPES[kind]).pin_memory() for _ in range(2)]
    caches = [DynamicRowCache(tables[0], "cuda", num_sets=1, stochastic_rounding=True, seed=S.WALK_SEED),
              DynamicRowCache(tables[1], "cuda", num_sets=1)]
    ids = torch.arange(S.WALK_ROWS, device="cuda")
    read = torch.arange(246, 256, device="cuda").reshape(-1, 1)
    grad = torch.ones((S.WALK_ROWS, S.WALK_WIDTH), dtype=DTYPES[kind], device="cuda")
    with no_read_back():
        for cache in caches:
            cache.forward(read, num_hots=1)
            for _ in range(S.WALK_STEPS):
                cache.apply_sgd(ids, grad, S.WALK_LR[k])
    slots = caches[0].slot_of_row[:S.WALK_ROWS].cpu().numpy()
    assert (slots >= 0).all() and not (slots == np.arange(S.WALK_ROWS)).any()
    with no_read_back():
        for cache in caches:
            cache.flush()
    torch.cuda.synchronize()
    want = S.walk(k)[0]
    assert np.array_equal(pat(tables[0])[:S.WALK_ROWS], want) and not np.array_equal(want, pat(tables[1])[:S.WALK_ROWS])
    assert torch.equal(tables[0][S.WALK_ROWS:], torch.ones_like(tables[0][S.WALK_ROWS:]))
    assert torch.equal(tables[1], torch.ones_like(tables[1]))
    assert caches[0].rounding_step.item() == S.WALK_STEPS and caches[1].rounding_step is None
    clean_exit()


# ---- 6. count sources and edges ---------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", ["sgd", "rowwise_adam"])
def test_count_sources_name_the_same_entries(rule):
    ids = torch.from_numpy(np.random.default_rng(8).permutation(M.ROWS)[:100]).to(torch.int32).cuda()
    grad = randn((100, 24), torch.float16, seeded(7))
    sources = (dict(count=60), dict(count=torch.tensor([60], dtype=torch.int32, device="cuda")),
               dict(last_id=torch.tensor([59], dtype=torch.int32, device="cuda")))
    results = []
    for source in sources:
        cache, updater = make(rule, normal_table("f16", 24, M.ROWS), 4)
        with no_read_back():
            cache.apply_update(ids, grad, LR, **source)
            cache.flush()
        torch.cuda.synchronize()
        assert cache.stats()["batch_count"] == 60 and cache.stats()["misses"] == 60
        results.append(cache)
    updater.apply(ids, grad, count=60)
    before = normal_table("f16", 24, M.ROWS)
    untouched = np.setdiff1d(np.arange(M.ROWS), ids[:60].cpu().numpy())
    for cache in results:
        assert_planes_equal(cache, updater, rule)
        assert torch.equal(cache.table[untouched], before[untouched])
        assert cache.rounding_step.item() == updater.rounding_step.item() == 1
    assert not torch.equal(results[0].table, before)
    clean_exit()


@pytest.mark.parametrize("rule", ["sgd", "adagrad", "adam"])
def test_steps_without_entries_advance_the_rounding_step(rule):
    """Zero entries and count=0 advance rounding_step like the updater's, and touch no plane."""
    table = normal_table("f16", 24, M.ROWS)
    cache, updater = make(rule, table, 1)
    before = {name: t.clone() for name, t in planes(cache, rule).items()}
    ids = torch.arange(8, device="cuda")
    grad = torch.ones((8, 24), dtype=torch.float16, device="cuda")
    none = torch.empty((0,), dtype=torch.int64, device="cuda")
    no_rows = torch.empty((0, 24), dtype=torch.float16, device="cuda")
    updater.apply(none, no_rows)
    updater.apply(ids, grad, count=0)
    with no_read_back():
        cache.apply_update(none, no_rows, LR)
        cache.apply_update(ids, grad, LR, count=0)
        cache.flush()
    torch.cuda.synchronize()
    assert cache.rounding_step.item() == updater.rounding_step.item() == 2
    assert cache.stats()["misses"] == 0 and int((cache.tags >= 0).sum()) == 0
    for name, t in planes(cache, rule).items():
        assert torch.equal(t, before[name]), name
    assert_planes_equal(cache, updater, rule)
    # a run is resumed by filling the word: step 2 after a resume is step 2 of an uninterrupted run
    resumed, _ = make(rule, table.clone().pin_memory(), 1)
    resumed.rounding_step.fill_(2)
    updater.apply(ids, grad)
    with no_read_back():
        for c in (cache, resumed):
            c.apply_update(ids, grad, LR)
            c.flush()
    torch.cuda.synchronize()
    assert torch.equal(cache.table, updater.table.cpu()) and not torch.equal(cache.table, before["table"])
    if rule == "sgd":        # (the other rules' clocks and states are not resumed by the word alone)
        assert torch.equal(resumed.table, cache.table)
    assert resumed.rounding_step.item() == cache.rounding_step.item() == 3
    clean_exit()


def test_edges():
    from cuembed_amd.row_cache import AdamRowCache, DynamicRowCache
    half = normal_table("f16", 24, 300)
    single = torch.zeros((300, 24), dtype=torch.float32).pin_memory()
    for build in (lambda t, **kw: DynamicRowCache(t, "cuda", num_sets=1, **kw),
                  lambda t, **kw: DynamicRowCache(t, "cuda", num_sets=1, rule="rowwise_adagrad", **kw),
                  lambda t, **kw: AdamRowCache(t, "cuda", num_sets=1, **kw)):
        with pytest.raises(TypeError, match="float32 table"):
            build(single, stochastic_rounding=True)
        for seed in (-1, 2 ** 64, True):
            with pytest.raises(ValueError, match="seed must be an int"):
                build(half, stochastic_rounding=True, seed=seed)
        assert build(half).rounding_step is None and build(single).rounding_step is None
        assert build(half, seed=-1).rounding_step is None           # (the seed is looked at with the option only)
        cache = build(half, stochastic_rounding=True, seed=2 ** 64 - 1)
        assert cache.rounding_step.tolist() == [0] and cache.rounding_step.dtype == torch.int64
        assert cache.rounding_step.device == cache.device
    clean_exit()
