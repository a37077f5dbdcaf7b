"""The row cache's PLANES on the GPU, every plane count in one matrix: the table's rows alone (rule="sgd"), with one state
plane (Adagrad, row-wise Adagrad) and with two (lazy Adam, row-wise Adam), with round to nearest and, for float16 tables,
stochastic rounding -- at the smallest shapes at which the plane plumbing can go wrong.  200 table rows behind 1 or 3 sets
of 64 ways (3 is no power of two); the widths make the mover take each of its lane sizes: float16 x 2 is a 4-byte row,
one uint32_t lane (the row-wise state is 4 bytes too), float32 x 6 a 24-byte row of 8-byte lanes, float16 x 8 one 16-byte
lane.

Every case runs the same traffic through the cache and through its oracle -- optim.SparseUpdater / SparseAdamUpdater with
the same rule, hyper-parameters and seed on device copies of the table and the state: step A, a step with no entries, a
step with count=0, step B, a forward on a third batch that mixes resident, evicted and never-seen rows, a flush.  The host
table and every host state tensor must then equal the oracle's BIT FOR BIT (integer views, no tolerance).

One set: every row maps to set 0, so the counters follow by construction.  A names 64 distinct rows (all 64 ways filled
and dirty), B 80 distinct rows, 32 of them A's: 32 hits, 48 misses for 64 - 32 = 32 free ways, hence 32 evictions, 32
write-backs and 48 - 32 = 16 rows without a way, which are updated in place in the host table and in every host state
plane.  Three sets: the expected words come from tests/dynamic_row_cache_reference.CacheModel, evaluated on the CPU, on
ids picked with conflict_rows so that the model shows evictions, write-backs and rows without a way."""
import functools

import numpy as np
import pytest
import torch

import dynamic_row_cache_reference as M

pytestmark = pytest.mark.gpu

ROWS = 200
DTYPES = {"f16": torch.float16, "f32": torch.float32}
INDEX = {"i32": torch.int32, "i64": torch.int64}
#: (element type, width): 4-byte rows (one uint32_t lane), 24-byte rows (8-byte lanes), 16-byte rows (one 16-byte lane)
GEOMETRY = [("f16", 2), ("f32", 6), ("f16", 8)]
KINDS = ("sgd", "adagrad", "rowwise_adagrad", "adam", "rowwise_adam")
ADAMS = ("adam", "rowwise_adam")
LR, INIT, EPS, SEED = 0.0371, 0.5, 1e-4, 0xC0FFEE1234567
#: counters that the two steps without entries must leave alone (they move the clock and clear the two per-batch words)
QUIET_WORDS = ("hits", "misses", "evictions", "write_backs", "unplaced", "overflow")


@functools.lru_cache(maxsize=None)
def traffic(num_sets):
    """(A, B, C, model after A and the two steps without entries, model after B): the row ids of the two steps and of
    the forward, and the CPU model's expectation.  Computed once per geometry and never changed."""
    if num_sets == 1:
        order = np.random.default_rng(11).permutation(ROWS)
        a, b = order[:64], np.concatenate([order[32:64], order[64:112]])
        c = np.concatenate([order[40:60], order[:20], order[120:140]])       # resident, evicted by B, never seen
    else:
        sets = [M.conflict_rows(num_sets, s, int((M.cache_set_of(np.arange(ROWS), num_sets) == s).sum()), rows=ROWS)
                for s in range(num_sets)]
        full = max(sets, key=len)                                             # the one set with more than 64 rows
        others = [s for s in sets if s is not full]
        assert len(full) >= 68
        # A fills the full set's ways; B hits 60 of them and misses with every other row of that set: 4 free ways
        a = np.concatenate([full[:64], others[0][:10], others[1][:10]])
        b = np.concatenate([full[4:], others[0][5:20], others[1][:3]])
        c = np.concatenate([full[:24], others[0][:8], others[1][30:58]])
    for batch in (a, b):
        assert np.unique(batch).size == batch.size
    model = M.CacheModel(ROWS, num_sets)
    model.prefetch(a, for_update=True)
    model.prefetch(np.empty(0, np.int64), for_update=True)
    model.prefetch(np.empty(0, np.int64), for_update=True)
    after_a = dict(model.counters)
    model.prefetch(b, for_update=True)
    after_b = dict(model.counters)
    unplaced = b[model.slot_of_row[b] < 0]
    evicted = np.setdiff1d(a, b)[model.slot_of_row[np.setdiff1d(a, b)] < 0]
    assert after_b["evictions"] > 0 and after_b["write_backs"] > 0 and after_b["unplaced"] > 0
    assert unplaced.size == after_b["unplaced"] and evicted.size == after_b["evictions"]
    # the forward's batch mixes rows that are resident, rows that B evicted and rows that no step has named
    assert np.intersect1d(c, evicted).size and np.setdiff1d(c, np.concatenate([a, b])).size
    assert (model.slot_of_row[c] >= 0).any()
    return a, b, c.reshape(-1, 4), after_a, after_b, unplaced


def test_the_traffic_is_what_the_docstring_says():
    a, b, c, after_a, after_b, unplaced = traffic(1)
    assert a.size == 64 and b.size == 80 and np.intersect1d(a, b).size == 32
    assert after_a == dict(hits=0, misses=64, evictions=0, write_backs=0, unplaced=0)
    assert after_b == dict(hits=32, misses=64 + 48, evictions=32, write_backs=32, unplaced=16)
    assert unplaced.size == 16


def host_table(kind, width):
    rng = np.random.default_rng(7)
    return torch.from_numpy(rng.standard_normal((ROWS, width)).astype(np.float32)).to(DTYPES[kind]).pin_memory()


def make(kind, table, num_sets, stochastic):
    """(cache, updater): the cache on the pinned `table` and its oracle on a device copy."""
    from cuembed_amd.optim import SparseAdamUpdater, SparseUpdater
    from cuembed_amd.row_cache import AdamRowCache, DynamicRowCache
    kw = dict(stochastic_rounding=True, seed=SEED) if stochastic else {}
    if kind in ADAMS:
        adam = dict(rowwise=kind == "rowwise_adam", betas=(0.75, 0.9), eps=EPS, weight_decay=0.01, **kw)
        return AdamRowCache(table, "cuda", num_sets=num_sets, **adam), SparseAdamUpdater(table.cuda(), LR, **adam)
    cache = DynamicRowCache(table, "cuda", num_sets=num_sets, rule=kind, initial_accumulator_value=INIT, eps=EPS, **kw)
    return cache, SparseUpdater(table.cuda(), kind, LR, eps=EPS, initial_accumulator_value=INIT, **kw)


def planes(owner, kind):
    """The table and the rule's state tensors of a cache (host side) or an updater (device side), by name."""
    if kind in ADAMS:
        return dict(table=owner.table, exp_avg=owner.exp_avg, exp_avg_sq=owner.exp_avg_sq)
    return dict(table=owner.table) if kind == "sgd" else dict(table=owner.table, state=owner.state)


def cached_planes(cache, kind):
    if kind in ADAMS:
        return dict(table=cache.cache, exp_avg=cache.exp_avg_cache, exp_avg_sq=cache.exp_avg_sq_cache)
    return dict(table=cache.cache) if kind == "sgd" else dict(table=cache.cache, state=cache.state_cache)


def bits(t):
    """`t` on the host as integers of its element size: comparing them compares bits (-0.0 and NaN included)."""
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def assert_planes_equal(cache, updater, kind, rows=None):
    want = planes(updater, kind)
    for name, got in planes(cache, kind).items():
        g, w = bits(got), bits(want[name])
        assert torch.equal(g if rows is None else g[rows], w if rows is None else w[rows]), name


def snapshot(cache, kind):
    """Everything a step without entries must leave alone, on the host."""
    torch.cuda.synchronize()
    out = {name: bits(t).clone() for name, t in planes(cache, kind).items()}
    out.update({"cached " + name: bits(t) for name, t in cached_planes(cache, kind).items()})
    out.update({name: getattr(cache, name).cpu().view(torch.uint8) for name in ("tags", "stamps", "dirty", "slot_of_row")})
    stats = cache.stats()
    out["words"] = torch.tensor([stats[k] for k in QUIET_WORDS])
    return out


def step_args(ids_np, capacity, index, source):
    """(ids, keyword arguments of the count): `ids_np` padded to `capacity` entries with rows it does not name, and the count as `source` gives it."""
    n = ids_np.size
    padded = np.concatenate([ids_np, np.setdiff1d(np.arange(ROWS), ids_np)[:capacity - n]])
    ids = torch.from_numpy(padded).to(INDEX[index]).cuda()
    if source == "last_id":
        return ids, dict(last_id=torch.tensor([n - 1], dtype=INDEX[index], device="cuda"))
    if source == "count_word":
        return ids, dict(count=torch.tensor([n], dtype=torch.int32, device="cuda"))
    return ids, (dict(count=n) if capacity > n else {})


def counters(cache):
    stats = cache.stats()
    return {k: stats[k] for k in M.COUNTERS}


def run_case(kind, geometry, num_sets, index, stochastic, source):
    import cuembed_amd as ce
    elem, width = geometry
    a, b, c, after_a, after_b, unplaced = traffic(num_sets)
    table = host_table(elem, width)
    cache, updater = make(kind, table, num_sets, stochastic)
    apply = cache.apply_sgd if kind == "sgd" else cache.apply_update
    gen = torch.Generator(device="cuda")
    gen.manual_seed(3)
    # a count that is not on the host comes with ids beyond it: rows that no step may touch
    capacity = {"host": 0, "last_id": 16, "count_word": 16}[source]

    def step(ids_np):
        ids, count = step_args(ids_np, ids_np.size + capacity, index, source)
        grad = torch.randn((ids.numel(), width), device="cuda", generator=gen).to(table.dtype)
        updater.apply(ids, grad, **count)
        apply(ids, grad, LR, **count)
        return ids, grad

    ids, grad = step(a)
    assert counters(cache) == after_a
    # a step with no entries and one with count=0: the Adam clock and rounding_step move by one each, nothing else does
    before = snapshot(cache, kind)
    none = torch.empty((0,), dtype=INDEX[index], device="cuda")
    no_rows = torch.empty((0, width), dtype=table.dtype, device="cuda")
    for empty in ((none, no_rows, {}), (ids, grad, dict(count=0))):
        clock = cache.powers[0].item() if kind in ADAMS else None
        rounding_step = cache.rounding_step.item() if stochastic else None
        updater.apply(empty[0], empty[1], **empty[2])
        assert apply(empty[0], empty[1], LR, **empty[2]) is None
        if kind in ADAMS:
            assert cache.powers[0].item() == clock + 1
        assert (cache.rounding_step.item() == rounding_step + 1) if stochastic else cache.rounding_step is None
    after = snapshot(cache, kind)
    for name in before:
        assert torch.equal(before[name], after[name]), name
    assert cache.stats()["clock"] == 4 and cache.stats()["batch_count"] == 0

    step(b)
    stats = cache.stats()
    assert {k: stats[k] for k in M.COUNTERS} == after_b and stats["overflow"] == 0
    assert stats["batch_count"] == b.size
    if num_sets == 1:
        assert after_b == dict(hits=32, misses=112, evictions=32, write_backs=32, unplaced=16)
    if kind in ADAMS:
        assert torch.equal(cache.powers, updater.powers) and torch.equal(cache.bias_factor, updater.bias_factor)
        assert cache.powers[0].item() == 4
    if stochastic:
        assert cache.rounding_step.item() == 4 and updater.rounding_step.item() == 4
    # rows without a way were updated in place in host memory, in the table and in every state plane -- no flush yet
    torch.cuda.synchronize()
    assert np.array_equal(np.sort(b[cache.slot_of_row.cpu().numpy()[b] < 0]), np.sort(unplaced))
    assert_planes_equal(cache, updater, kind, rows=torch.from_numpy(unplaced))

    d_c = torch.from_numpy(c).to(INDEX[index]).cuda()
    got = cache.forward(d_c, num_hots=c.shape[1])
    want = ce.ops.embedding_forward(updater.table, d_c, num_hots=c.shape[1])
    assert torch.equal(bits(got), bits(want))
    cache.flush()
    torch.cuda.synchronize()
    assert_planes_equal(cache, updater, kind)
    assert int(cache.dirty.sum()) == 0
    assert ce._lib.lib().cuembed_peek_last_error() == 0


def case_id(value):
    return "%s-w%d" % value if isinstance(value, tuple) else str(value)


@pytest.mark.parametrize("index", ["i32", "i64"])
@pytest.mark.parametrize("num_sets", [1, 3], ids=["s1", "s3"])
@pytest.mark.parametrize("geometry", GEOMETRY, ids=case_id)
@pytest.mark.parametrize("kind", KINDS)
def test_nearest(kind, geometry, num_sets, index):
    run_case(kind, geometry, num_sets, index, stochastic=False, source="host")


@pytest.mark.parametrize("index", ["i32", "i64"])
@pytest.mark.parametrize("num_sets", [1, 3], ids=["s1", "s3"])
@pytest.mark.parametrize("geometry", [g for g in GEOMETRY if g[0] == "f16"], ids=case_id)
@pytest.mark.parametrize("kind", KINDS)
def test_stochastic(kind, geometry, num_sets, index):
    run_case(kind, geometry, num_sets, index, stochastic=True, source="host")


@pytest.mark.parametrize("source,index,num_sets", [("last_id", "i32", 1), ("count_word", "i64", 3)])
@pytest.mark.parametrize("stochastic", [False, True], ids=["nearest", "stochastic"])
@pytest.mark.parametrize("kind", KINDS)
def test_count_on_the_device(kind, stochastic, source, index, num_sets):
    """The count as last_id= and as a device count= word, with 16 entries beyond it that name other rows: the counters
    and the bits are those of the host-side count."""
    run_case(kind, ("f16", 8), num_sets, index, stochastic, source)
