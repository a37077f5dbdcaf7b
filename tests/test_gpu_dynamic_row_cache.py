"""DynamicRowCache on the GPU (cuembed::RowCachePrefetch / RowCacheFlush + cuembed_amd/row_cache.py): the cache's whole
state against the host model after every prefetch, bit-identical forwards, a set that overflows, training through the
write-back path, the edges, and no host read-back anywhere but stats().  Tiny shapes: 5,000 rows, 1 or 4 sets of 64
ways, batches of 64 x 5 lookups; rows of 64 and 48, of 40 and of 12 bytes take the mover's 16-, 8- and
4-byte lanes."""
import contextlib

import numpy as np
import pytest
import torch

import dynamic_row_cache_reference as M

pytestmark = pytest.mark.gpu

DTYPES = {"f32": torch.float32, "f16": torch.float16}
INDEX = {"i32": torch.int32, "i64": torch.int64}


@contextlib.contextmanager
def no_read_back():
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        yield
    finally:
        torch.cuda.set_sync_debug_mode("default")


def host_table(kind, width, rows=M.ROWS, seed=7):
    """Small integers: exactly representable in fp16, so sums of five rows are exact whatever the order."""
    rng = np.random.default_rng(seed)
    return torch.from_numpy(rng.integers(-8, 9, (rows, width)).astype(np.float32)).to(DTYPES[kind]).pin_memory()


def make(case, rows=M.ROWS):
    from cuembed_amd.row_cache import DynamicRowCache
    table = host_table(case["kind"], case["width"], rows)
    return table, DynamicRowCache(table, "cuda", num_sets=case["num_sets"])


def dev(idx, case):
    return torch.from_numpy(idx).to(INDEX[case["index"]]).cuda()


def assert_state(cache, snapshot, table):
    tags, stamps, dirty, slot_of_row, counters, clock = snapshot
    stats = cache.stats()
    assert {k: stats[k] for k in M.COUNTERS} == counters
    assert stats["clock"] == clock and stats["overflow"] == 0
    assert np.array_equal(cache.tags.cpu().numpy(), tags)
    assert np.array_equal(cache.stamps.cpu().numpy(), stamps)
    assert np.array_equal(cache.dirty.cpu().numpy(), dirty)
    assert np.array_equal(cache.slot_of_row.cpu().numpy(), slot_of_row)
    slots = np.nonzero(tags.reshape(-1) >= 0)[0]
    assert torch.equal(cache.cache.cpu()[slots], table[tags.reshape(-1)[slots]])      # every tagged slot holds its row


def clean_exit():
    import cuembed_amd as ce
    torch.cuda.synchronize()
    assert ce._lib.lib().cuembed_peek_last_error() == 0


@pytest.mark.parametrize("case", M.CASES, ids=M.case_id)
def test_state_equals_the_model_after_every_prefetch(case):
    table, cache = make(case)
    before = table.clone()
    _, snapshots = M.model_trace(case)
    for idx, for_update, snapshot in zip(M.batches(), M.FOR_UPDATE, snapshots):
        d_idx = dev(idx, case)
        with no_read_back():
            cache.prefetch(d_idx, for_update=for_update)
        assert_state(cache, snapshot, table)
    # write-backs of rows that nothing updated store what the table already held
    cache.flush()
    torch.cuda.synchronize()
    assert torch.equal(table, before) and int(cache.dirty.sum()) == 0
    clean_exit()


@pytest.mark.parametrize("case", [c for c in M.CASES if (c["index"] == "i32") == (c["num_sets"] == 1)], ids=M.case_id)
def test_forward_is_bit_identical_to_the_device_table(case):
    import cuembed_amd as ce
    table, cache = make(case)
    d_table = table.cuda()
    model = M.CacheModel(M.ROWS, case["num_sets"])
    weights = torch.randint(-2, 3, (M.BATCH, M.HOTS), device="cuda").to(table.dtype)
    lengths = 1 + np.random.default_rng(3).multinomial(M.BATCH * (M.HOTS - 1), np.ones(M.BATCH) / M.BATCH)   # ragged, none empty
    offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(lengths)])).to(torch.int32).cuda()
    for step, idx in enumerate(M.batches(seed=1, foreign=False)):
        d_idx = dev(idx, case)
        layouts = [dict(num_hots=M.HOTS), dict(weights=weights, num_hots=M.HOTS, mode="mean"),
                   dict(offsets=offsets, num_hots=0), dict(offsets=offsets, weights=weights.reshape(-1), mode="mean")]
        kw = layouts[step % len(layouts)]
        want = ce.embedding_forward(d_table, d_idx, **kw)
        with no_read_back():
            got = cache.forward(d_idx, **kw)
        assert torch.equal(got, want), (step, kw.keys())
        model.prefetch(idx)
        assert cache.stats()["hits"] == model.counters["hits"] and cache.stats()["unplaced"] == model.counters["unplaced"]
    assert model.counters["hits"] > 0 and model.counters["evictions"] > 0
    # the cached copies are what is read: zero them and a batch of resident rows pools zeros
    want = ce.embedding_forward(d_table, d_idx, num_hots=M.HOTS)
    assert torch.equal(cache.forward(d_idx, num_hots=M.HOTS), want)
    cache.cache.zero_()
    assert not torch.equal(cache.forward(d_idx, num_hots=M.HOTS), want)
    cache.invalidate()
    assert torch.equal(cache.forward(d_idx, num_hots=M.HOTS), want)
    clean_exit()


@pytest.mark.parametrize("case", [c for c in M.CASES if c["num_sets"] == 4 and c["width"] != 6 and
                                  (c["index"] == "i64") == (c["kind"] == "f32")], ids=M.case_id)
def test_a_set_that_overflows_keeps_its_resident_rows(case):
    import cuembed_amd as ce
    table, cache = make(case)
    d_table = table.cuda()
    model = M.CacheModel(M.ROWS, 4)
    rows = M.conflict_rows(4, 2, 70)                                      # 70 rows of set 2: six more than its ways
    early = rows[[1, 17, 40, 69]]
    other = np.setdiff1d(np.arange(300), rows)[:20]                       # and some rows of any set
    for batch in (np.concatenate([early, other]), np.concatenate([rows, other[:6]])):
        idx = np.resize(batch, (16, 5))                                   # (repeats the batch's first rows)
        d_idx = dev(idx, case)
        with no_read_back():
            got = cache.forward(d_idx, num_hots=5)
        model.prefetch(idx)
        assert torch.equal(got, ce.embedding_forward(d_table, d_idx, num_hots=5))
    stats = cache.stats()
    assert model.counters["unplaced"] == 70 - 64 and {"unplaced", "protected_hit"} <= model.events
    assert {k: stats[k] for k in M.COUNTERS} == model.counters
    slot_of_row = cache.slot_of_row.cpu().numpy()
    assert (slot_of_row[early] >= 0).all() and np.array_equal(slot_of_row, model.slot_of_row)
    assert np.array_equal(cache.tags.cpu().numpy(), model.tags) and np.array_equal(cache.stamps.cpu().numpy(), model.stamps)
    # the rows left out are the largest ids that were not resident: misses are placed in ascending row id
    assert np.array_equal(rows[slot_of_row[rows] < 0], np.setdiff1d(rows, early)[-6:])
    clean_exit()


@pytest.mark.parametrize("case", [dict(kind="f16", width=24, num_sets=1, index="i32"),
                                  dict(kind="f32", width=16, num_sets=4, index="i64")], ids=M.case_id)
def test_training_through_the_cache_equals_training_on_the_device(case):
    """Five steps of forward, compressed backward (count on the device) and SGD.  The cache holds 64 / 256 rows, a step
    touches about 170: dirty rows are evicted and written back, rows without a way are updated over PCIe."""
    import cuembed_amd as ce
    table, cache = make(case)
    d_table = table.cuda()
    lr, cap = 0.25, M.BATCH * M.HOTS
    model = M.CacheModel(M.ROWS, case["num_sets"])
    for idx in M.batches(seed=2, foreign=False)[:5]:
        d_idx = dev(idx, case)
        grad_y = torch.randint(-3, 4, (M.BATCH, case["width"]), device="cuda").to(table.dtype)
        t_idx, t_sid, _, remap = ce.transpose_fixed_hotness(d_idx, M.BATCH, M.HOTS, num_categories=M.ROWS, remapped=True)
        grad = torch.empty((cap, case["width"]), dtype=table.dtype, device="cuda")
        inv = torch.empty((cap,), dtype=d_idx.dtype, device="cuda")
        ce.embedding_backward(grad_y, None, t_idx, t_sid, remap, grad_embedding=grad, inverse_mapping=inv)
        want = ce.embedding_forward(d_table, d_idx, num_hots=M.HOTS)
        ce.sparse_row_update(d_table, inv, grad, rule="sgd", lr=lr, last_id=remap[-1:])
        with no_read_back():
            got = cache.forward(d_idx, num_hots=M.HOTS)
            cache.apply_sgd(inv, grad, lr, last_id=remap[-1:])
        assert torch.equal(got, want)
        model.prefetch(idx)
        model.prefetch(np.unique(idx), for_update=True)
    stats = cache.stats()
    assert {k: stats[k] for k in M.COUNTERS} == model.counters
    assert model.counters["write_backs"] > 0 and "dirty_eviction" in model.events
    assert np.array_equal(cache.dirty.cpu().numpy(), model.dirty) and model.dirty.sum() > 0
    torch.cuda.synchronize()
    assert not torch.equal(table, d_table.cpu())               # the newest rows are still in the cache only
    with no_read_back():
        cache.flush()
    torch.cuda.synchronize()
    assert torch.equal(table, d_table.cpu())                   # ... and write-back is what carries them
    assert cache.stats()["write_backs"] == model.counters["write_backs"] + int(model.dirty.sum())
    assert int(cache.dirty.sum()) == 0
    clean_exit()


def test_count_on_the_device_and_host_counts_name_the_same_lookups():
    case = dict(kind="f32", width=16, num_sets=4, index="i64")
    idx = M.batches(seed=3, foreign=True)[1].reshape(-1)
    want = M.CacheModel(M.ROWS, 4)
    want.prefetch(idx[:100])
    d_idx = dev(idx, case)
    for source in (dict(count=100), dict(count=torch.tensor([100], dtype=torch.int32, device="cuda")),
                   dict(count=torch.tensor([100], dtype=torch.int64, device="cuda")),
                   dict(last_id=torch.tensor([99], dtype=torch.int64, device="cuda"))):
        table, cache = make(case)
        with no_read_back():
            cache.prefetch(d_idx, **source)
        assert np.array_equal(cache.tags.cpu().numpy(), want.tags), source
        assert cache.stats()["batch_count"] == 100 and cache.stats()["misses"] == want.counters["misses"]
    # a count past the capacity counts as nothing, like the sparse step's
    past = torch.tensor([idx.size + 1], dtype=torch.int64, device="cuda")
    with no_read_back():
        cache.prefetch(d_idx, count=past)
    assert cache.stats()["batch_count"] == 0 and np.array_equal(cache.tags.cpu().numpy(), want.tags)
    clean_exit()


def test_edges():
    import cuembed_amd as ce
    case = dict(kind="f16", width=24, num_sets=1, index="i64")
    table, cache = make(case)
    model = M.CacheModel(M.ROWS, 1)
    # an empty batch: the clock moves, nothing else
    with no_read_back():
        cache.prefetch(torch.empty((0,), dtype=torch.int64, device="cuda"))
        out = cache.forward(torch.empty((0, 5), dtype=torch.int64, device="cuda"), num_hots=5)
    model.prefetch([])
    model.prefetch([])
    assert out.shape == (0, 24) and cache.stats()["clock"] == 3 and int((cache.tags >= 0).sum()) == 0
    # a batch entirely outside the table
    foreign = np.array([-1, -7, M.ROWS, M.ROWS + 9, 1 << 40])
    d_foreign = torch.from_numpy(foreign).cuda()
    with no_read_back():
        cache.prefetch(d_foreign)
        translated = cache.translate(d_foreign)
    model.prefetch(foreign)
    assert translated.tolist() == foreign.tolist() and int((cache.tags >= 0).sum()) == 0
    stats = cache.stats()
    assert {k: stats[k] for k in M.COUNTERS} == model.counters == dict.fromkeys(M.COUNTERS, 0) and stats["clock"] == 4
    # a table smaller than the cache: everything fits, every later batch hits
    small, tiny = make(dict(kind="f32", width=16, num_sets=4, index="i32"), rows=40)
    idx = torch.randint(0, 40, (64, 5), dtype=torch.int32, device="cuda")
    want = ce.embedding_forward(small.cuda(), idx, num_hots=5)
    for _ in range(2):
        with no_read_back():
            got = tiny.forward(idx, num_hots=5)
        assert torch.equal(got, want)
    distinct = int(idx.unique().numel())
    stats = tiny.stats()
    assert (stats["hits"], stats["misses"], stats["evictions"], stats["unplaced"]) == (distinct, distinct, 0, 0)
    # invalidate() drops everything, write-backs included; the next forward fills the cache again
    with no_read_back():
        tiny.prefetch(idx, for_update=True)
        tiny.invalidate()
        got = tiny.forward(idx, num_hots=5)
    assert torch.equal(got, want)
    stats = tiny.stats()
    assert stats["misses"] == 2 * distinct and stats["write_backs"] == 0 and int(tiny.dirty.sum()) == 0
    assert int((tiny.tags >= 0).sum()) == distinct
    with pytest.raises(RuntimeError, match="fills itself"):
        tiny.cache_most_frequent(idx)
    with pytest.raises(TypeError):
        tiny.apply_sgd(idx.reshape(-1)[:4].long(), torch.zeros((4, 16), dtype=torch.float16, device="cuda"), 0.1)
    clean_exit()
