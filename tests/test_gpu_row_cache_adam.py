"""AdamRowCache on the GPU: lazy Adam and row-wise Adam on a host-resident table through the cache
(cuembed::RowCachePrefetch / RowCacheFlush with two state planes, cuembed::TranslateIndicesForRowCachePlanes,
cuembed::SparseRowAdam with placed moments, cache.apply_update) against optim.SparseAdamUpdater on device copies of the
table and the moments, BIT FOR BIT -- both sides run one walk with one launch shape on the same gradient tensor, and a
cached plane is a whole number of rows from its home tensor, hence aligned alike, so no tolerance is needed.  Gradients
are torch.randn rounded to the table's type: sqrt and the division see inexact data.  Placement (counters, dirty bytes,
slot_of_row) is compared with tests/dynamic_row_cache_reference.CacheModel; what the sequences contain is shown on the
CPU in tests/test_adam_row_cache_host.py.  Tiny shapes: 5,000 rows, 1 or 4 sets of 64 ways."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

import adam_row_cache_reference as AR
import dynamic_row_cache_reference as M
import row_cache_state_reference as S

pytestmark = pytest.mark.gpu

DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
INDEX = {"i32": torch.int32, "i64": torch.int64}
LR = AR.LR
RULES = AR.RULES
PLANES = ("table", "exp_avg", "exp_avg_sq")


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


def given_moments(width, rule):
    """Pinned moments that differ row by row and from each other (adam_row_cache_reference.initial_moments)."""
    m, v = AR.initial_moments(M.ROWS, width, rule)
    return (torch.from_numpy(m.astype(np.float32)).pin_memory(), torch.from_numpy(v.astype(np.float32)).pin_memory())


def make(case, rule, lr=LR, given=False, **kw):
    """(host table, cache, updater): the cache and its oracle, optim.SparseAdamUpdater on device copies of the table
    and the moments."""
    from cuembed_amd.optim import SparseAdamUpdater
    from cuembed_amd.row_cache import AdamRowCache
    table = host_table(case["kind"], case["width"])
    moments = {}
    if given:
        moments["exp_avg"], moments["exp_avg_sq"] = given_moments(case["width"], rule)
    cache = AdamRowCache(table, "cuda", num_sets=case["num_sets"], rowwise=rule == "rowwise_adam", **moments, **kw)
    updater = SparseAdamUpdater(table.cuda(), lr, rowwise=rule == "rowwise_adam", **kw)
    updater.exp_avg.copy_(cache.exp_avg)
    updater.exp_avg_sq.copy_(cache.exp_avg_sq)
    return table, cache, updater


def randn(shape, dtype, generator):
    return torch.randn(shape, device="cuda", generator=generator).to(dtype)


def seeded(seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return g


def counters(cache):
    stats = cache.stats()
    return {k: stats[k] for k in M.COUNTERS}


def host_planes(cache):
    return dict(table=cache.table, exp_avg=cache.exp_avg, exp_avg_sq=cache.exp_avg_sq)


def device_planes(updater):
    return dict(table=updater.table.cpu(), exp_avg=updater.exp_avg.cpu(), exp_avg_sq=updater.exp_avg_sq.cpu())


def assert_planes_equal(cache, updater, rows=slice(None)):
    got, want = host_planes(cache), device_planes(updater)
    for name in PLANES:
        assert torch.equal(got[name][rows], want[name][rows]), name


def assert_no_plane_equal(cache, updater, rows=slice(None)):
    got, want = host_planes(cache), device_planes(updater)
    for name in PLANES:
        assert not torch.equal(got[name][rows], want[name][rows]), name


def assert_clocks_equal(cache, updater):
    assert torch.equal(cache.powers, updater.powers) and torch.equal(cache.bias_factor, updater.bias_factor)


def clean_exit():
    import cuembed_amd as ce
    torch.cuda.synchronize()
    assert ce._lib.lib().cuembed_peek_last_error() == 0


# ---- 1. training parity -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("weight_decay", AR.WEIGHT_DECAYS)
@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("case", AR.TRAINING_CASES, ids=M.case_id)
def test_training_through_the_cache_equals_training_on_the_device(case, rule, weight_decay):
    """Five steps of forward, compressed backward (count on the device) and the rule.  The cache holds 64 / 256 rows,
    a step touches about 170: dirty rows are evicted and written back with both moments, rows without a way are
    updated over PCIe in all three planes."""
    import cuembed_amd as ce
    table, cache, updater = make(case, rule, weight_decay=weight_decay)
    assert cache.exp_avg.is_pinned() and cache.exp_avg_sq.is_pinned() and not cache.exp_avg.any()
    assert tuple(cache.exp_avg_sq.shape) == ((M.ROWS,) if rule == "rowwise_adam" else (M.ROWS, case["width"]))
    assert cache.powers.tolist() == [0.0, 1.0, 1.0] and cache.powers.is_cuda and cache.bias_factor.dtype == torch.float32
    cap, gen = M.BATCH * M.HOTS, seeded(3)
    index = INDEX[case["index"]]
    for idx in S.training_batches():
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
        assert torch.equal(got, want)
    model = S.training_placement(case["num_sets"])
    assert counters(cache) == model.counters and cache.stats()["overflow"] == 0
    assert model.counters["write_backs"] > 0 and (model.counters["unplaced"] > 0) == (case["num_sets"] == 1)
    assert np.array_equal(cache.dirty.cpu().numpy(), model.dirty) and model.dirty.sum() > 0
    assert np.array_equal(cache.slot_of_row.cpu().numpy(), model.slot_of_row)
    assert_clocks_equal(cache, updater)
    assert cache.powers[0].item() == S.TRAINING_STEPS
    torch.cuda.synchronize()
    assert_no_plane_equal(cache, updater)              # the newest rows and their moments are in the cache only
    with no_read_back():
        cache.flush()
    torch.cuda.synchronize()
    assert_planes_equal(cache, updater)                # ... and write-back is what carries all three planes
    assert cache.stats()["write_backs"] == model.counters["write_backs"] + int(model.dirty.sum())    # rows, not planes
    assert int(cache.dirty.sum()) == 0
    clean_exit()


# ---- 2. evicted moments come back -----------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", RULES)
def test_evicted_moments_come_back(rule):
    """Rows 0..39 are updated, evicted dirty by a read of 64 other rows of the one set, and updated again.  The caller's
    moments differ from each other and row by row: swapped planes, a wrong row size or a moment that was
    re-initialised on the second fill instead of written back and re-read gives other bits in the second step."""
    import cuembed_amd as ce
    case = dict(kind="f16", width=8, num_sets=1, index="i64")
    table, cache, updater = make(case, rule, given=True)
    first_moment, second_moment = given_moments(8, rule)
    assert torch.equal(cache.exp_avg, first_moment) and torch.equal(cache.exp_avg_sq, second_moment)
    gen = seeded(4)
    ids = torch.from_numpy(S.EVICT_UPDATED).cuda()
    read = torch.from_numpy(S.EVICT_READ).cuda().reshape(-1, 1)
    first, second = randn((40, 8), table.dtype, gen), randn((40, 8), table.dtype, gen)
    updater.apply(ids, first)
    with no_read_back():
        cache.apply_update(ids, first, LR)
        got = cache.forward(read, num_hots=1)
    assert torch.equal(got, ce.embedding_forward(updater.table, read, num_hots=1))
    torch.cuda.synchronize()
    stats = cache.stats()
    assert stats["write_backs"] == 40 and stats["evictions"] == 40 and int((cache.slot_of_row[:40] >= 0).sum()) == 0
    # the write-back, not a flush, carried the weights and both moments
    assert_planes_equal(cache, updater, slice(0, 40))
    assert not torch.equal(cache.exp_avg[:40], first_moment[:40])
    assert not torch.equal(cache.exp_avg_sq[:40], second_moment[:40])
    updater.apply(ids, second)
    with no_read_back():
        cache.apply_update(ids, second, LR)
    torch.cuda.synchronize()
    assert_no_plane_equal(cache, updater, slice(0, 40))
    with no_read_back():
        cache.flush()
    torch.cuda.synchronize()
    assert_planes_equal(cache, updater)
    assert torch.equal(cache.exp_avg[40:], first_moment[40:]) and torch.equal(cache.exp_avg_sq[40:], second_moment[40:])
    assert_clocks_equal(cache, updater)
    clean_exit()


# ---- 3. a set that overflows ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", RULES)
def test_a_set_that_overflows_trains_correctly(rule):
    """70 rows of one set of 64 ways: 70 - 64 = 6 find no way and are updated in the host table and both host moments
    over PCIe.  The learning rate is a device word."""
    case = dict(kind="f16", width=24, num_sets=S.OVERFLOW_SETS, index="i32")
    lr = torch.tensor([LR], dtype=torch.float32, device="cuda")
    table, cache, updater = make(case, rule, lr=lr, given=True)
    gen = seeded(5)
    rows = M.conflict_rows(S.OVERFLOW_SETS, S.OVERFLOW_SET, S.OVERFLOW_ROWS)
    model = M.CacheModel(M.ROWS, S.OVERFLOW_SETS)
    for batch in (rows[:5], rows):
        ids = torch.from_numpy(batch).to(torch.int32).cuda()
        grad = randn((batch.size, 24), table.dtype, gen)
        updater.apply(ids, grad)
        with no_read_back():
            cache.apply_update(ids, grad, lr)
        model.prefetch(batch, for_update=True)
    torch.cuda.synchronize()
    assert model.counters["hits"] == 5 and model.counters["unplaced"] == 6 and counters(cache) == model.counters
    slot_of_row = cache.slot_of_row.cpu().numpy()
    assert np.array_equal(slot_of_row, model.slot_of_row)
    left_out, resident = rows[slot_of_row[rows] < 0], rows[slot_of_row[rows] >= 0]
    assert left_out.size == 6 and resident.size == 64
    assert_planes_equal(cache, updater, torch.from_numpy(left_out))        # without a flush
    assert_no_plane_equal(cache, updater, torch.from_numpy(resident))
    with no_read_back():
        cache.flush()
    torch.cuda.synchronize()
    assert_planes_equal(cache, updater)
    clean_exit()


# ---- 4. reads carry both moments ------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", RULES)
def test_reads_carry_both_moments(rule):
    """Rows filled by a forward bring both moment rows along: an update that hits them later finds them in the cache."""
    case = dict(kind="f32", width=16, num_sets=4, index="i64")
    table, cache, updater = make(case, rule, given=True)
    initial = dict(exp_avg=cache.exp_avg.clone(), exp_avg_sq=cache.exp_avg_sq.clone())
    read = torch.arange(100, 160, device="cuda")
    subset = read[::3].contiguous()
    grad = randn((subset.numel(), 16), table.dtype, seeded(6))
    updater.apply(subset, grad)
    with no_read_back():
        cache.forward(read.reshape(12, 5), num_hots=5)
    slots = cache.slot_of_row[100:160].long()
    cached = (cache.exp_avg_cache[slots].clone(), cache.exp_avg_sq_cache[slots].clone())
    with no_read_back():
        cache.apply_update(subset, grad, LR)
        cache.flush()
    torch.cuda.synchronize()
    assert torch.equal(cached[0].cpu(), initial["exp_avg"][100:160])
    assert torch.equal(cached[1].cpu(), initial["exp_avg_sq"][100:160])
    stats = cache.stats()
    assert stats["misses"] == 60 and stats["hits"] == 20 and stats["unplaced"] == 0 and stats["write_backs"] == 20
    assert_planes_equal(cache, updater)
    touched = torch.zeros(M.ROWS, dtype=torch.bool)
    touched[subset.cpu()] = True
    for name, before in initial.items():
        after = getattr(cache, name)
        assert torch.equal(after[~touched], before[~touched]), name
        assert not (after[touched] == before[touched]).reshape(20, -1).all(dim=1).any(), name
    clean_exit()


# ---- 5. the count sources ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", RULES)
def test_count_sources_name_the_same_entries(rule):
    case = dict(kind="f16", width=24, num_sets=4, index="i32")
    ids = torch.from_numpy(np.random.default_rng(8).permutation(M.ROWS)[:100]).to(torch.int32).cuda()
    grad = randn((100, 24), torch.float16, seeded(7))
    sources = (dict(count=60), dict(count=torch.tensor([60], dtype=torch.int32, device="cuda")),
               dict(last_id=torch.tensor([59], dtype=torch.int32, device="cuda")))
    results = []
    for source in sources:
        table, cache, updater = make(case, rule)
        with no_read_back():
            cache.apply_update(ids, grad, LR, **source)
            cache.flush()
        torch.cuda.synchronize()
        assert cache.stats()["batch_count"] == 60 and cache.stats()["misses"] == 60
        results.append(cache)
    updater.apply(ids, grad, count=60)
    for cache in results:
        assert_planes_equal(cache, updater)
        assert_clocks_equal(cache, updater)
    untouched = np.setdiff1d(np.arange(M.ROWS), ids[:60].cpu().numpy())
    assert not results[0].exp_avg[untouched].any() and not results[0].exp_avg_sq[untouched].any()
    clean_exit()


# ---- 6. edges -------------------------------------------------------------------------------------------------------
def test_edges():
    case = dict(kind="f16", width=24, num_sets=1, index="i64")
    table, cache, updater = make(case, "adam", given=True)
    before = {name: t.clone() for name, t in host_planes(cache).items()}
    ids = torch.arange(8, device="cuda")
    grad = torch.ones((8, 24), dtype=torch.float16, device="cuda")
    none = torch.empty((0,), dtype=torch.int64, device="cuda")
    no_rows = torch.empty((0, 24), dtype=torch.float16, device="cuda")
    # zero entries and count=0 advance both clocks -- the cache's and Adam's, like the updater's -- and touch nothing
    updater.apply(none, no_rows)
    updater.apply(ids, grad, count=0)
    with no_read_back():
        cache.apply_update(none, no_rows, LR)
        cache.apply_update(ids, grad, LR, count=0)
    stats = cache.stats()
    assert stats["clock"] == 3 and stats["misses"] == 0 and int((cache.tags >= 0).sum()) == 0
    assert cache.powers[0].item() == 2
    assert_clocks_equal(cache, updater)
    assert_planes_equal(cache, updater)
    # apply_sgd points to apply_update; neither clock moves
    with pytest.raises(RuntimeError, match="apply_update"):
        cache.apply_sgd(ids, grad, LR)
    # dtype and shape errors are raised before anything runs
    with pytest.raises(TypeError, match="dtype"):
        cache.apply_update(ids, grad.float(), LR)
    with pytest.raises(TypeError, match="int32 or int64"):
        cache.apply_update(ids.float(), grad, LR)
    with pytest.raises(ValueError, match="entries"):
        cache.apply_update(ids, grad[:, :12].contiguous(), LR)
    with pytest.raises(ValueError, match="entries"):
        cache.apply_update(ids[:4], grad, LR)
    with pytest.raises(TypeError, match="one-element float32"):
        cache.apply_update(ids, grad, torch.ones(2, device="cuda"))
    assert cache.stats()["clock"] == 3 and cache.powers[0].item() == 2
    # invalidate() drops the cached moments as well, without write-back: the next forward re-reads the host's
    with no_read_back():
        cache.apply_update(ids, grad, LR)
    slots = cache.slot_of_row[:8].long()
    assert not torch.equal(cache.exp_avg_cache[slots].cpu(), before["exp_avg"][:8])
    assert not torch.equal(cache.exp_avg_sq_cache[slots].cpu(), before["exp_avg_sq"][:8])
    with no_read_back():
        cache.invalidate()
        cache.forward(ids.reshape(8, 1), num_hots=1)
    slots = cache.slot_of_row[:8].long()
    assert int((slots >= 0).sum()) == 8
    assert torch.equal(cache.exp_avg_cache[slots].cpu(), before["exp_avg"][:8])
    assert torch.equal(cache.exp_avg_sq_cache[slots].cpu(), before["exp_avg_sq"][:8])
    cache.flush()
    torch.cuda.synchronize()
    for name, t in host_planes(cache).items():
        assert torch.equal(t, before[name]), name
    assert cache.stats()["write_backs"] == 0
    clean_exit()


@pytest.mark.parametrize("rule", RULES)
def test_without_bias_correction_the_factor_is_one_and_the_clock_still_counts(rule):
    case = dict(kind="f32", width=16, num_sets=4, index="i64")
    table, cache, updater = make(case, rule, bias_correction=False, weight_decay=0.01)
    with_correction = make(case, rule, weight_decay=0.01)[2]
    gen = seeded(9)
    ids = torch.arange(50, 90, device="cuda")
    for _ in range(2):
        grad = randn((40, 16), table.dtype, gen)
        updater.apply(ids, grad)
        with_correction.apply(ids, grad)
        with no_read_back():
            cache.apply_update(ids, grad, LR)
    with no_read_back():
        cache.flush()
    torch.cuda.synchronize()
    assert_planes_equal(cache, updater)
    assert_clocks_equal(cache, updater)
    assert cache.powers[0].item() == 2 and cache.bias_factor.item() != 1.0
    assert not torch.equal(table, with_correction.table.cpu())
    clean_exit()


# ---- 7. the moment planes change nothing about placement ------------------------------------------------------------
@pytest.mark.parametrize("case", [dict(kind="f16", width=24, num_sets=1, index="i32"),
                                  dict(kind="f32", width=16, num_sets=4, index="i64")], ids=M.case_id)
def test_placement_is_untouched(case):
    from cuembed_amd.row_cache import AdamRowCache, DynamicRowCache
    table = host_table(case["kind"], case["width"])
    before = table.clone()
    plain = DynamicRowCache(table, "cuda", num_sets=case["num_sets"])
    adam = AdamRowCache(table, "cuda", num_sets=case["num_sets"], rowwise=True)
    _, snapshots = M.model_trace(case)
    for idx, for_update, snapshot in zip(M.batches(), M.FOR_UPDATE, snapshots):
        d_idx = torch.from_numpy(idx).to(INDEX[case["index"]]).cuda()
        with no_read_back():
            plain.prefetch(d_idx, for_update=for_update)
            adam.prefetch(d_idx, for_update=for_update)
        for name in ("tags", "stamps", "dirty", "slot_of_row"):
            assert np.array_equal(getattr(plain, name).cpu().numpy(), getattr(adam, name).cpu().numpy()), name
        assert plain.stats() == adam.stats()
        tags, stamps, dirty, slot_of_row, counts, clock = snapshot
        assert counters(adam) == counts and adam.stats()["clock"] == clock
        assert np.array_equal(adam.tags.cpu().numpy(), tags) and np.array_equal(adam.dirty.cpu().numpy(), dirty)
        assert np.array_equal(adam.slot_of_row.cpu().numpy(), slot_of_row)
    adam.flush()
    plain.flush()
    torch.cuda.synchronize()
    assert plain.stats() == adam.stats()
    assert torch.equal(table, before) and not adam.exp_avg.any() and not adam.exp_avg_sq.any()
    assert adam.powers.tolist() == [0.0, 1.0, 1.0]           # prefetches and flushes are not steps
    clean_exit()


# ---- 8. the fused translate -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", ["i32", "i64"])
def test_the_fused_translate_equals_three_single_translates(index):
    """One launch, three offsets: each output is what cuembed_translate_indices_for_row_cache gives with that offset, for
    resident rows, rows that are not cached and ids outside the table; a null output is skipped."""
    import cuembed_amd as ce
    from cuembed_amd.row_cache import DynamicRowCache
    cache = DynamicRowCache(host_table("f16", 8), "cuda", num_sets=1)
    cache.prefetch(torch.arange(0, 120, 3, device="cuda"))
    rng = np.random.default_rng(12)
    idx = rng.integers(0, 200, 3000)                          # (more than one workgroup's items)
    idx[[5, 77, 2999]] = [-1, M.ROWS, M.ROWS + 123]
    d_idx = torch.from_numpy(idx).to(INDEX[index]).cuda()
    assert int((cache.slot_of_row[d_idx[(d_idx >= 0) & (d_idx < M.ROWS)].long()] >= 0).sum()) > 100
    offsets = (cache.cache_row_offset, -77, 2 ** 40 + 3)
    L = ce._lib.lib()
    p = ctypes.c_void_p
    stream = p(torch.cuda.current_stream().cuda_stream)
    code = ce.ops._INDEX[d_idx.dtype]
    want = []
    for offset in offsets:
        out = torch.empty((idx.size,), dtype=torch.int64, device="cuda")
        L.cuembed_translate_indices_for_row_cache(p(d_idx.data_ptr()), code, idx.size, p(cache.slot_of_row.data_ptr()),
                                                  M.ROWS, offset, p(out.data_ptr()), stream)
        want.append(out)
    got = torch.full((3, idx.size), -5, dtype=torch.int64, device="cuda")
    with no_read_back():
        L.cuembed_translate_indices_for_row_cache_planes(
            p(d_idx.data_ptr()), code, idx.size, p(cache.slot_of_row.data_ptr()), M.ROWS, offsets[0], p(got[0].data_ptr()),
            offsets[1], p(got[1].data_ptr()), offsets[2], p(got[2].data_ptr()), stream)
    for k in range(3):
        assert torch.equal(got[k], want[k]), k
    assert got[0][5].item() == -1 and got[2][77].item() == M.ROWS and got[1][2999].item() == M.ROWS + 123
    # a null output is skipped: the others are written, nothing else is
    got.fill_(-5)
    with no_read_back():
        L.cuembed_translate_indices_for_row_cache_planes(
            p(d_idx.data_ptr()), code, idx.size, p(cache.slot_of_row.data_ptr()), M.ROWS, offsets[0], None, offsets[1],
            p(got[1].data_ptr()), offsets[2], None, stream)
    assert torch.equal(got[1], want[1]) and bool((got[0] == -5).all()) and bool((got[2] == -5).all())
    clean_exit()
