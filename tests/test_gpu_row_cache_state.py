"""DynamicRowCache with a state plane on the GPU: Adagrad and row-wise Adagrad on a host-resident table through the
cache (cuembed::RowCachePrefetch / RowCacheFlush with RowCache::state, cuembed::SparseRowUpdate with state_ids,
cache.apply_update) against the same steps on device copies, BIT FOR BIT -- both sides run one walk with one launch
shape on the same gradient tensor, and the planes are aligned like the tensors they mirror, so no tolerance is needed.
Gradients are torch.randn rounded to the table's type: sqrt and the division see inexact data.  Placement (counters,
dirty bytes) is compared with tests/dynamic_row_cache_reference.CacheModel; what the sequences contain is shown on the
CPU in tests/test_row_cache_state_host.py.  Tiny shapes: 5,000 rows, 1 or 4 sets of 64 ways."""
import contextlib

import numpy as np
import pytest
import torch

import dynamic_row_cache_reference as M
import row_cache_state_reference as S

pytestmark = pytest.mark.gpu

DTYPES = {"f32": torch.float32, "f16": torch.float16}
INDEX = {"i32": torch.int32, "i64": torch.int64}
LR, INIT = S.LR, 0.5


@contextlib.contextmanager
def no_read_back():
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        yield
    finally:
        torch.cuda.set_sync_debug_mode("default")


def host_table(kind, width, rows=M.ROWS, seed=7):
    rng = np.random.default_rng(seed)
    return torch.from_numpy(rng.integers(-8, 9, (rows, width)).astype(np.float32)).to(DTYPES[kind]).pin_memory()


def make(case, rule, rows=M.ROWS, **kw):
    """(host table, cache, device copy of the table, device copy of the state): the cache and its oracle."""
    from cuembed_amd.row_cache import DynamicRowCache
    table = host_table(case["kind"], case["width"], rows)
    kw.setdefault("initial_accumulator_value", INIT)
    cache = DynamicRowCache(table, "cuda", num_sets=case["num_sets"], rule=rule, **kw)
    return table, cache, table.cuda(), cache.state.cuda()


def randn(shape, dtype, generator):
    return torch.randn(shape, device="cuda", generator=generator).to(dtype)


def seeded(seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return g


def counters(cache):
    stats = cache.stats()
    return {k: stats[k] for k in M.COUNTERS}


def assert_planes_equal(table, cache, d_table, d_state, rows=slice(None)):
    assert torch.equal(table[rows], d_table.cpu()[rows])
    assert torch.equal(cache.state[rows], d_state.cpu()[rows])


def clean_exit():
    import cuembed_amd as ce
    torch.cuda.synchronize()
    assert ce._lib.lib().cuembed_peek_last_error() == 0


# ---- 1. training parity -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", S.RULES)
@pytest.mark.parametrize("case", S.TRAINING_CASES, ids=M.case_id)
def test_training_through_the_cache_equals_training_on_the_device(case, rule):
    """Five steps of forward, compressed backward (count on the device) and the rule.  The cache holds 64 / 256 rows,
    a step touches about 170: dirty rows are evicted and written back with their state, rows without a way are
    updated over PCIe, weights and state."""
    import cuembed_amd as ce
    table, cache, d_table, d_state = make(case, rule)
    cap, gen = M.BATCH * M.HOTS, seeded(3)
    index = INDEX[case["index"]]
    for idx in S.training_batches():
        d_idx = torch.from_numpy(idx).to(index).cuda()
        grad_y = randn((M.BATCH, case["width"]), table.dtype, gen)
        t_idx, t_sid, _, remap = ce.transpose_fixed_hotness(d_idx, M.BATCH, M.HOTS, num_categories=M.ROWS, remapped=True)
        grad = torch.empty((cap, case["width"]), dtype=table.dtype, device="cuda")
        inv = torch.empty((cap,), dtype=index, device="cuda")
        ce.embedding_backward(grad_y, None, t_idx, t_sid, remap, grad_embedding=grad, inverse_mapping=inv)
        want = ce.embedding_forward(d_table, d_idx, num_hots=M.HOTS)
        ce.sparse_row_update(d_table, inv, grad, rule=rule, state=d_state, lr=LR, last_id=remap[-1:])
        with no_read_back():
            got = cache.forward(d_idx, num_hots=M.HOTS)
            cache.apply_update(inv, grad, LR, last_id=remap[-1:])
        assert torch.equal(got, want)
    model = S.training_placement(case["num_sets"])
    assert counters(cache) == model.counters and cache.stats()["overflow"] == 0
    assert model.counters["write_backs"] > 0 and (model.counters["unplaced"] > 0) == (case["num_sets"] == 1)
    assert np.array_equal(cache.dirty.cpu().numpy(), model.dirty) and model.dirty.sum() > 0
    torch.cuda.synchronize()
    assert not torch.equal(table, d_table.cpu())               # the newest rows and their state are in the cache only
    assert not torch.equal(cache.state, d_state.cpu())
    with no_read_back():
        cache.flush()
    torch.cuda.synchronize()
    assert_planes_equal(table, cache, d_table, d_state)        # ... and write-back is what carries both planes
    assert cache.stats()["write_backs"] == model.counters["write_backs"] + int(model.dirty.sum())    # rows, not planes
    assert int(cache.dirty.sum()) == 0
    clean_exit()


# ---- 2. an evicted accumulator comes back ---------------------------------------------------------------------------
@pytest.mark.parametrize("rule", S.RULES)
def test_an_evicted_accumulator_comes_back(rule):
    """Rows 0..39 are updated, evicted dirty by a read of 64 other rows of the one set, and updated again.  The state
    starts at 0.5, not 0: an accumulator that was re-initialised on the second fill instead of written back and
    re-read gives other bits in the second step."""
    import cuembed_amd as ce
    case = dict(kind="f16", width=8, num_sets=1, index="i64")
    table, cache, d_table, d_state = make(case, rule)
    gen = seeded(4)
    ids = torch.from_numpy(S.EVICT_UPDATED).cuda()
    read = torch.from_numpy(S.EVICT_READ).cuda().reshape(-1, 1)
    first, second = randn((40, 8), table.dtype, gen), randn((40, 8), table.dtype, gen)
    ce.sparse_row_update(d_table, ids, first, rule=rule, state=d_state, lr=LR)
    with no_read_back():
        cache.apply_update(ids, first, LR)
        got = cache.forward(read, num_hots=1)
    assert torch.equal(got, ce.embedding_forward(d_table, read, num_hots=1))
    torch.cuda.synchronize()
    stats = cache.stats()
    assert stats["write_backs"] == 40 and stats["evictions"] == 40 and int((cache.slot_of_row[:40] >= 0).sum()) == 0
    # the write-back, not a flush, carried weights and state
    assert_planes_equal(table, cache, d_table, d_state, slice(0, 40))
    assert not torch.equal(cache.state[:40], torch.full_like(cache.state[:40], INIT))
    ce.sparse_row_update(d_table, ids, second, rule=rule, state=d_state, lr=LR)
    with no_read_back():
        cache.apply_update(ids, second, LR)
    torch.cuda.synchronize()
    assert not torch.equal(cache.state[:40], d_state.cpu()[:40])
    with no_read_back():
        cache.flush()
    torch.cuda.synchronize()
    assert_planes_equal(table, cache, d_table, d_state)
    clean_exit()


# ---- 3. a set that overflows ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", S.RULES)
def test_a_set_that_overflows_trains_correctly(rule):
    """70 rows of one set: six find no way and are updated in the host table and the host state over PCIe."""
    import cuembed_amd as ce
    case = dict(kind="f16", width=24, num_sets=S.OVERFLOW_SETS, index="i32")
    table, cache, d_table, d_state = make(case, rule)
    gen = seeded(5)
    rows = M.conflict_rows(S.OVERFLOW_SETS, S.OVERFLOW_SET, S.OVERFLOW_ROWS)
    model = M.CacheModel(M.ROWS, S.OVERFLOW_SETS)
    lr = torch.tensor([LR], dtype=torch.float32, device="cuda")           # (the learning rate as a device word)
    for batch in (rows[:5], rows):
        ids = torch.from_numpy(batch).to(torch.int32).cuda()
        grad = randn((batch.size, 24), table.dtype, gen)
        ce.sparse_row_update(d_table, ids, grad, rule=rule, state=d_state, lr=lr)
        with no_read_back():
            cache.apply_update(ids, grad, lr)
        model.prefetch(batch, for_update=True)
    torch.cuda.synchronize()
    assert model.counters["hits"] == 5 and model.counters["unplaced"] == 6 and counters(cache) == model.counters
    slot_of_row = cache.slot_of_row.cpu().numpy()
    assert np.array_equal(slot_of_row, model.slot_of_row)
    left_out, resident = rows[slot_of_row[rows] < 0], rows[slot_of_row[rows] >= 0]
    assert left_out.size == 6 and resident.size == 64
    assert_planes_equal(table, cache, d_table, d_state, torch.from_numpy(left_out))        # without a flush
    assert not torch.equal(cache.state[resident], d_state.cpu()[resident])
    with no_read_back():
        cache.flush()
    torch.cuda.synchronize()
    assert_planes_equal(table, cache, d_table, d_state)
    clean_exit()


# ---- 4. reads carry state -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule, given", [("rowwise_adagrad", True), ("adagrad", True), ("adagrad", False)])
def test_reads_carry_state(rule, given):
    """Rows filled by a forward bring their state along: an update that hits them later finds it in the cache."""
    import cuembed_amd as ce
    case = dict(kind="f32", width=16, num_sets=4, index="i64")
    kw = {}
    if given:    # a state of the caller's that differs row by row (initial_accumulator_value is then not used)
        shape = (M.ROWS, 16) if rule == "adagrad" else (M.ROWS,)
        kw["state"] = torch.rand(shape, generator=torch.Generator().manual_seed(9)).add_(0.25).pin_memory()
    table, cache, d_table, d_state = make(case, rule, **kw)
    initial = cache.state.clone()
    if given:
        assert cache.state is kw["state"]
    else:
        assert torch.equal(initial, torch.full((M.ROWS, 16), INIT)) and cache.state.is_pinned()
    read = torch.arange(100, 160, device="cuda")
    subset = read[::3].contiguous()
    grad = randn((subset.numel(), 16), table.dtype, seeded(6))
    ce.sparse_row_update(d_table, subset, grad, rule=rule, state=d_state, lr=LR)
    with no_read_back():
        cache.forward(read.reshape(12, 5), num_hots=5)
        cache.apply_update(subset, grad, LR)
        cache.flush()
    torch.cuda.synchronize()
    stats = cache.stats()
    assert stats["misses"] == 60 and stats["hits"] == 20 and stats["unplaced"] == 0 and stats["write_backs"] == 20
    assert_planes_equal(table, cache, d_table, d_state)
    touched = torch.zeros(M.ROWS, dtype=torch.bool)
    touched[subset.cpu()] = True
    assert torch.equal(cache.state[~touched], initial[~touched])
    assert not (cache.state[touched] == initial[touched]).reshape(20, -1).all(dim=1).any()
    clean_exit()


# ---- 5. the count sources ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", S.RULES)
def test_count_sources_name_the_same_entries(rule):
    import cuembed_amd as ce
    case = dict(kind="f16", width=24, num_sets=4, index="i32")
    ids = torch.from_numpy(np.random.default_rng(8).permutation(M.ROWS)[:100]).to(torch.int32).cuda()
    grad = randn((100, 24), torch.float16, seeded(7))
    sources = (dict(count=60), dict(count=torch.tensor([60], dtype=torch.int32, device="cuda")),
               dict(last_id=torch.tensor([59], dtype=torch.int32, device="cuda")))
    results = []
    for source in sources:
        table, cache, d_table, d_state = make(case, rule)
        with no_read_back():
            cache.apply_update(ids, grad, LR, **source)
            cache.flush()
        torch.cuda.synchronize()
        assert cache.stats()["batch_count"] == 60 and cache.stats()["misses"] == 60
        results.append((table, cache.state))
    ce.sparse_row_update(d_table, ids, grad, rule=rule, state=d_state, lr=LR, count=60)
    for table, state in results:
        assert torch.equal(table, d_table.cpu()) and torch.equal(state, d_state.cpu())
    untouched = np.setdiff1d(np.arange(M.ROWS), ids[:60].cpu().numpy())
    assert torch.equal(results[0][1][untouched], torch.full_like(results[0][1][untouched], INIT))
    clean_exit()


# ---- 6. edges -------------------------------------------------------------------------------------------------------
def test_edges():
    import cuembed_amd as ce
    case = dict(kind="f16", width=24, num_sets=1, index="i64")
    table, cache, d_table, d_state = make(case, "adagrad")
    before_table, before_state = table.clone(), cache.state.clone()
    # a zero-entry update is a no-op that still advances the clock
    none = torch.empty((0,), dtype=torch.int64, device="cuda")
    with no_read_back():
        cache.apply_update(none, torch.empty((0, 24), dtype=torch.float16, device="cuda"), LR)
        cache.apply_update(torch.arange(8, device="cuda"), torch.ones((8, 24), dtype=torch.float16, device="cuda"), LR,
                           count=0)
    stats = cache.stats()
    assert stats["clock"] == 3 and stats["misses"] == 0 and int((cache.tags >= 0).sum()) == 0
    # apply_sgd on a cache with another rule
    ids = torch.arange(8, device="cuda")
    grad = torch.ones((8, 24), dtype=torch.float16, device="cuda")
    with pytest.raises(RuntimeError, match="apply_update"):
        cache.apply_sgd(ids, grad, LR)
    assert cache.stats()["clock"] == 3
    with pytest.raises(TypeError):
        cache.apply_update(ids, grad.float(), LR)
    # invalidate() drops cached state as well, without write-back: the next forward re-reads the host state
    with no_read_back():
        cache.apply_update(ids, grad, LR)
    slots = cache.slot_of_row[:8].long()
    assert not torch.equal(cache.state_cache[slots].cpu(), before_state[:8])
    with no_read_back():
        cache.invalidate()
        cache.forward(ids.reshape(8, 1), num_hots=1)
    slots = cache.slot_of_row[:8].long()
    assert int((slots >= 0).sum()) == 8 and torch.equal(cache.state_cache[slots].cpu(), before_state[:8])
    cache.flush()
    torch.cuda.synchronize()
    assert torch.equal(table, before_table) and torch.equal(cache.state, before_state)
    assert cache.stats()["write_backs"] == 0
    # on a rule="sgd" cache apply_update is apply_sgd, and there is no state plane
    from cuembed_amd.row_cache import DynamicRowCache
    plain = DynamicRowCache(table, "cuda", num_sets=1)
    assert plain.rule == "sgd" and plain.state is None and plain.state_cache is None
    ce.sparse_row_update(d_table, ids, grad, rule="sgd", lr=LR)
    with no_read_back():
        plain.apply_update(ids, grad, LR)
        plain.flush()
    torch.cuda.synchronize()
    assert torch.equal(table, d_table.cpu())
    clean_exit()


# ---- 7. the state plane changes nothing about placement -------------------------------------------------------------
@pytest.mark.parametrize("case", [dict(kind="f16", width=24, num_sets=1, index="i32"),
                                  dict(kind="f32", width=16, num_sets=4, index="i64")], ids=M.case_id)
def test_rule_free_behaviour_is_untouched(case):
    from cuembed_amd.row_cache import DynamicRowCache
    table = host_table(case["kind"], case["width"])
    before = table.clone()
    plain = DynamicRowCache(table, "cuda", num_sets=case["num_sets"])
    with_state = DynamicRowCache(table, "cuda", num_sets=case["num_sets"], rule="rowwise_adagrad")
    _, snapshots = M.model_trace(case)
    for idx, for_update, snapshot in zip(M.batches(), M.FOR_UPDATE, snapshots):
        d_idx = torch.from_numpy(idx).to(INDEX[case["index"]]).cuda()
        with no_read_back():
            plain.prefetch(d_idx, for_update=for_update)
            with_state.prefetch(d_idx, for_update=for_update)
        for name in ("tags", "stamps", "dirty", "slot_of_row"):
            assert np.array_equal(getattr(plain, name).cpu().numpy(), getattr(with_state, name).cpu().numpy()), name
        assert plain.stats() == with_state.stats()
        tags, stamps, dirty, slot_of_row, counts, clock = snapshot
        assert counters(with_state) == counts and with_state.stats()["clock"] == clock
        assert np.array_equal(with_state.tags.cpu().numpy(), tags) and np.array_equal(with_state.dirty.cpu().numpy(), dirty)
    with_state.flush()
    plain.flush()
    torch.cuda.synchronize()
    assert plain.stats() == with_state.stats()
    assert torch.equal(table, before) and torch.equal(with_state.state, torch.zeros(M.ROWS))
    clean_exit()
