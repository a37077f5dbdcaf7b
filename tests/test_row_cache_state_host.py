"""DynamicRowCache's state plane without a GPU: the argument checks of `rule` and `state` (raised before any device is
asked for), the three new entry points, and the host model of tests/row_cache_state_reference.py -- its invariants on
the sequences the GPU tests run, and what those sequences contain."""
import os
import re

import numpy as np
import pytest
import torch

import dynamic_row_cache_reference as M
import row_cache_state_reference as S
from cuembed_amd.row_cache import WAYS, DynamicRowCache

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("cuembed_row_cache_prefetch_with_state", "cuembed_row_cache_flush_with_state",
               "cuembed_sparse_row_update_placed")


def test_rule_and_state_errors_come_before_any_device_check():
    """The table is an unpinned CPU tensor: whatever is wrong with rule / state is reported before the table's memory
    (ValueError "PINNED") or a device is looked at."""
    table = torch.zeros((8, 4), dtype=torch.float16)
    for bad in ("adam", "Adagrad", None, 3):
        with pytest.raises(ValueError, match="rule must be one of"):
            DynamicRowCache(table, num_sets=1, rule=bad)
    with pytest.raises(ValueError, match="takes no state"):
        DynamicRowCache(table, num_sets=1, state=torch.zeros(8))
    with pytest.raises(ValueError, match="takes no state"):
        DynamicRowCache(table, num_sets=1, rule="sgd", state=torch.zeros((8, 4)))
    with pytest.raises(TypeError, match="Tensor"):
        DynamicRowCache(table, num_sets=1, rule="adagrad", state=np.zeros((8, 4), np.float32))
    for rule, good in (("adagrad", (8, 4)), ("rowwise_adagrad", (8,))):
        with pytest.raises(TypeError, match="float32"):
            DynamicRowCache(table, num_sets=1, rule=rule, state=torch.zeros(good, dtype=torch.float16))
        with pytest.raises(TypeError, match="float32"):
            DynamicRowCache(table, num_sets=1, rule=rule, state=torch.zeros(good, dtype=torch.float64))
        for shape in ((8, 4) if rule == "rowwise_adagrad" else (8,), (7,) + good[1:], (8, 4, 1)):
            with pytest.raises(ValueError, match="state of shape"):
                DynamicRowCache(table, num_sets=1, rule=rule, state=torch.zeros(shape))
        with pytest.raises(ValueError, match="state must live in PINNED"):
            DynamicRowCache(table, num_sets=1, rule=rule, state=torch.zeros(good))
        # a good rule without a state gets as far as the table's own check
        with pytest.raises(ValueError, match="host_table must live in PINNED"):
            DynamicRowCache(table, num_sets=1, rule=rule)
    with pytest.raises(ValueError, match="contiguous"):
        DynamicRowCache(table, num_sets=1, rule="adagrad", state=torch.zeros((4, 8)).t())
    # the defaults are today's constructor
    with pytest.raises(ValueError, match="host_table must live in PINNED"):
        DynamicRowCache(table, "cuda", 1)


def test_the_new_entry_points_are_declared_in_plain_c_and_exported():
    from cuembed_amd import _lib
    L = _lib.lib()
    with open(os.path.join(ROOT, "include", "cuembed_amd.h")) as f:
        header = re.sub(r"\s+", " ", f.read())
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
        assert re.search(r"\bvoid %s ?\(" % name, header), name
    # the new parameters, as the issue names them
    plane = "float* state, float* state_cache, int64_t state_row_bytes);"
    assert header.count(plane) == 2
    assert re.search(r"cuembed_sparse_row_update_placed ?\([^)]*const int64_t\* state_ids\);", header)
    assert L.cuembed_sparse_row_update_placed.argtypes[:-1] == L.cuembed_sparse_row_update.argtypes
    assert L.cuembed_row_cache_prefetch_with_state.argtypes[:-3] == L.cuembed_row_cache_prefetch.argtypes
    assert L.cuembed_row_cache_flush_with_state.argtypes[:-3] == L.cuembed_row_cache_flush.argtypes


@pytest.mark.parametrize("num_sets, dirty_evictions, unplaced, dirty_slots", [(1, 219, 1010, 64), (4, 422, 0, 256)])
def test_what_the_training_sequence_contains(num_sets, dirty_evictions, unplaced, dirty_slots):
    """CacheModel on the training-parity sequence (each batch prefetched once for read and once for update)."""
    model = S.training_placement(num_sets)
    assert model.counters["write_backs"] == dirty_evictions
    assert model.counters["unplaced"] == unplaced
    assert int(model.dirty.sum()) == dirty_slots
    assert "dirty_eviction" in model.events and "hit" in model.events


@pytest.mark.parametrize("rule", S.RULES)
@pytest.mark.parametrize("case", S.TRAINING_CASES, ids=M.case_id)
def test_the_model_keeps_every_rows_state_current_through_training(case, rule):
    """run_training asserts after every prefetch and update that the current copy of every row's weights and state is
    what the updates produced, that the host state moves only by write-back (or an update in place), and that a clean
    eviction writes nothing.  Here: the sequence contains a dirty eviction and a hit for update everywhere, an
    unplaced update in the one-set case; before the flush the host arrays are stale, after it they alone are current."""
    model = S.run_training(S.StateCacheModel(M.ROWS, case["width"], case["num_sets"], rule, 0.5))
    placement = S.training_placement(case["num_sets"])
    assert model.place.counters == placement.counters and np.array_equal(model.place.tags, placement.tags)
    t = model.totals
    assert t["dirty_evicted"] == placement.counters["write_backs"] > 0
    assert t["hits_for_update"] > 0 and t["updates_in_cache"] > 0
    assert t["updates_in_host"] == placement.counters["unplaced"] - unplaced_by_reads(case["num_sets"])
    assert (t["updates_in_host"] > 0) == (case["num_sets"] == 1)
    assert not np.array_equal(model.host_s, model.true_s) and not np.array_equal(model.host_w, model.true_w)
    model.flush()
    assert np.array_equal(model.host_s, model.true_s) and np.array_equal(model.host_w, model.true_w)
    assert int(model.place.dirty.sum()) == 0
    # ... and the cache is not needed any more
    model.invalidate()
    w, s = model.current()
    assert np.array_equal(s, model.true_s) and np.array_equal(w, model.true_w)


def unplaced_by_reads(num_sets):
    """Unplaced rows of the training sequence's forward prefetches (they are read over PCIe; nothing is updated)."""
    model, total = M.CacheModel(M.ROWS, num_sets), 0
    for idx in S.training_batches():
        before = model.counters["unplaced"]
        model.prefetch(idx)
        total += model.counters["unplaced"] - before
        model.prefetch(np.unique(idx), for_update=True)
    return total


@pytest.mark.parametrize("rule", S.RULES)
def test_an_evicted_accumulator_comes_back_in_the_model(rule):
    """Update rows 0..39, read 64 other rows through the one set, update rows 0..39 again: all 40 are evicted dirty by
    the read, and the write-back -- not a flush -- carries their state to the host."""
    model = S.StateCacheModel(M.ROWS, 8, 1, rule, 0.5)
    rng = np.random.default_rng(1)
    model.apply_update(S.EVICT_UPDATED, rng.standard_normal((40, 8)))
    assert model.totals["updates_in_cache"] == 40 and not np.array_equal(model.host_s[:40], model.true_s[:40])
    before = model.host_s.copy()
    model.prefetch(S.EVICT_READ)
    S.check_prefetch(model, before)
    assert sorted(model.last["dirty_evicted"]) == S.EVICT_UPDATED.tolist()            # 40 write-backs ...
    assert model.place.counters["write_backs"] == 40 and model.place.counters["unplaced"] == 0
    assert (model.place.slot_of_row[S.EVICT_UPDATED] < 0).all()                       # ... 0 of them still resident
    assert np.array_equal(model.host_s[:40], model.true_s[:40])
    assert (model.host_s[:40] != 0.5).reshape(40, -1).all()         # a re-initialised state would be 0.5 again
    before = model.host_s.copy()
    model.apply_update(S.EVICT_UPDATED, rng.standard_normal((40, 8)))
    S.check_update(model, before, S.EVICT_UPDATED)
    # the second fill evicts 40 of the rows that were only read: clean, nothing is written, the host state stays
    assert len(model.last["clean_evicted"]) == 40 and not model.last["dirty_evicted"]
    assert np.array_equal(model.host_s, before)
    assert model.totals["filled"] == 40 + 64 + 40
    model.flush()
    assert np.array_equal(model.host_s, model.true_s) and np.array_equal(model.host_w, model.true_w)
    assert (model.host_s[40:] == 0.5).all()


@pytest.mark.parametrize("rule", S.RULES)
def test_a_set_that_overflows_trains_correctly_in_the_model(rule):
    rows = M.conflict_rows(S.OVERFLOW_SETS, S.OVERFLOW_SET, S.OVERFLOW_ROWS)
    model = S.StateCacheModel(M.ROWS, 8, S.OVERFLOW_SETS, rule, 0.5)
    rng = np.random.default_rng(2)
    model.apply_update(rows[:5], rng.standard_normal((5, 8)))
    model.apply_update(rows, rng.standard_normal((70, 8)))
    assert model.place.counters["hits"] == 5 and model.place.counters["unplaced"] == 6
    assert model.totals["updates_in_host"] == 6 and model.totals["hits_for_update"] == 5
    left_out = rows[model.place.slot_of_row[rows] < 0]
    assert left_out.size == 6
    # the six rows without a way are current in the host arrays already, the 64 resident ones only after the flush
    assert np.array_equal(model.host_s[left_out], model.true_s[left_out])
    assert np.array_equal(model.host_w[left_out], model.true_w[left_out])
    resident = np.setdiff1d(rows, left_out)
    assert not np.array_equal(model.host_s[resident], model.true_s[resident])
    model.flush()
    assert np.array_equal(model.host_s, model.true_s) and np.array_equal(model.host_w, model.true_w)


def test_reads_carry_state_in_the_model():
    """A forward-only fill brings the state along: a later update that hits finds it in the cache."""
    model = S.StateCacheModel(M.ROWS, 8, 4, "rowwise_adagrad", 0.5)
    model.host_s[:] = model.true_s[:] = np.arange(M.ROWS) + 0.5          # (a state that differs row by row)
    read = np.arange(100, 160)
    model.prefetch(read)
    assert model.totals["filled"] == 60 and int(model.place.dirty.sum()) == 0
    slots = model.place.slot_of_row[read]
    assert np.array_equal(model.cache_s[slots], read + 0.5)
    model.apply_update(read[::3], np.ones((20, 8)))
    assert model.totals["hits_for_update"] == 20 and model.totals["filled"] == 60
    assert int(model.place.dirty.sum()) == 20 and WAYS * 4 >= 60
    model.flush()
    assert np.array_equal(model.host_s[read[::3]], read[::3] + 1.5)      # mean of 1^2 over the row = 1
    untouched = np.setdiff1d(np.arange(M.ROWS), read[::3])
    assert np.array_equal(model.host_s[untouched], untouched + 0.5)


def test_the_cpp_known_answer_program_has_a_build_of_its_own():
    from cuembed_amd import build
    assert callable(build.build_row_cache_state_test)
    assert os.path.exists(os.path.join(ROOT, "tests", "cpp", "row_cache_state_kat.hip"))
