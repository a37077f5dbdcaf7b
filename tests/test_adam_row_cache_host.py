"""AdamRowCache without a GPU: the argument checks (raised before the table's memory or any device is looked at), the
four new entry points, the host model of tests/adam_row_cache_reference.py -- its invariants on the sequences the GPU
tests run, and what those sequences contain -- and that what was there before is as it was."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import adam_row_cache_reference as AR
import dynamic_row_cache_reference as M
import row_cache_state_reference as S
from cuembed_amd.row_cache import WAYS, AdamRowCache, DynamicRowCache

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("cuembed_row_cache_prefetch_with_states", "cuembed_row_cache_flush_with_states",
               "cuembed_sparse_row_adam_placed", "cuembed_translate_indices_for_row_cache_planes")


def test_argument_errors_come_before_any_device_check():
    """The table is an unpinned CPU tensor: whatever is wrong with the hyper-parameters or the moments is reported
    before the table's memory (ValueError "PINNED") or a device is looked at."""
    table = torch.zeros((8, 4), dtype=torch.float16)
    with pytest.raises(TypeError, match="host_table must be a torch.Tensor"):
        AdamRowCache(np.zeros((8, 4), np.float32))
    with pytest.raises(TypeError, match="num_sets must be an int"):
        AdamRowCache(table, num_sets=1.0)
    with pytest.raises(ValueError, match="num_sets must be in"):
        AdamRowCache(table, num_sets=0)
    with pytest.raises(ValueError, match="multiple of 4 bytes"):
        AdamRowCache(torch.zeros((8, 3), dtype=torch.float16), num_sets=1)
    for betas in ((1.0, 0.5), (0.9, -0.1), (0.9,), "ab"):
        with pytest.raises(ValueError, match="betas"):
            AdamRowCache(table, num_sets=1, betas=betas)
    with pytest.raises(ValueError, match="must not be negative"):
        AdamRowCache(table, num_sets=1, eps=-1.0)
    with pytest.raises(ValueError, match="must not be negative"):
        AdamRowCache(table, num_sets=1, weight_decay=-0.5)
    for rowwise, good_sq in ((False, (8, 4)), (True, (8,))):
        for name, good in (("exp_avg", (8, 4)), ("exp_avg_sq", good_sq)):
            with pytest.raises(TypeError, match="%s must be a torch.Tensor" % name):
                AdamRowCache(table, num_sets=1, rowwise=rowwise, **{name: np.zeros(good, np.float32)})
            for dtype in (torch.float16, torch.float64):
                with pytest.raises(TypeError, match="%s must be float32" % name):
                    AdamRowCache(table, num_sets=1, rowwise=rowwise, **{name: torch.zeros(good, dtype=dtype)})
            wrong = [(7,) + good[1:], good + (1,), (8,) if len(good) == 2 else (8, 4)]
            for shape in wrong:
                with pytest.raises(ValueError, match="%s of shape" % name):
                    AdamRowCache(table, num_sets=1, rowwise=rowwise, **{name: torch.zeros(shape)})
            with pytest.raises(ValueError, match="%s must live in PINNED" % name):
                AdamRowCache(table, num_sets=1, rowwise=rowwise, **{name: torch.zeros(good)})
        # good arguments get as far as the table's own check
        with pytest.raises(ValueError, match="host_table must live in PINNED"):
            AdamRowCache(table, "cuda", 1, rowwise)
    with pytest.raises(ValueError, match="contiguous"):
        AdamRowCache(table, num_sets=1, exp_avg=torch.zeros((4, 8)).t())


def test_it_is_a_new_class_and_rule_keeps_its_values():
    assert issubclass(AdamRowCache, DynamicRowCache)
    table = torch.zeros((8, 4), dtype=torch.float16)
    for bad in ("adam", "rowwise_adam"):
        with pytest.raises(ValueError, match="rule must be one of"):
            DynamicRowCache(table, num_sets=1, rule=bad)
    for text in ("2 * W + 8 * W", "2 * W + 4 * W + 4", "prefer"):
        assert text in re.sub(r"\s+", " ", AdamRowCache.__doc__), text


def test_the_new_entry_points_are_declared_in_plain_c_and_exported():
    from cuembed_amd import _lib
    L = _lib.lib()
    with open(os.path.join(ROOT, "include", "cuembed_amd.h")) as f:
        header = re.sub(r"\s+", " ", f.read())
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
        assert re.search(r"\bvoid %s ?\(" % name, header), name
    # the new parameters, as the issue names them
    planes = "int64_t state_row_bytes, float* state2, float* state2_cache, int64_t state2_row_bytes);"
    assert header.count(planes) == 2
    assert re.search(r"cuembed_sparse_row_adam_placed ?\([^)]*cuembed_stream_t stream, const int64_t\* exp_avg_ids, "
                     r"const int64_t\* exp_avg_sq_ids\);", header)
    assert L.cuembed_sparse_row_adam_placed.argtypes[:-2] == L.cuembed_sparse_row_adam.argtypes
    assert L.cuembed_row_cache_prefetch_with_states.argtypes[:-3] == L.cuembed_row_cache_prefetch_with_state.argtypes
    assert L.cuembed_row_cache_flush_with_states.argtypes[:-3] == L.cuembed_row_cache_flush_with_state.argtypes
    translate = L.cuembed_translate_indices_for_row_cache_planes.argtypes
    assert translate[:5] == L.cuembed_translate_indices_for_row_cache.argtypes[:5]
    assert translate[5:] == [ctypes.c_int64, ctypes.c_void_p] * 3 + [ctypes.c_void_p]


def test_one_plane_structs_are_unaffected():
    """RowCache's second plane is appended with zero defaults: the known-answer program of the one-plane cache fills
    the struct member by member and names none of the new ones."""
    with open(os.path.join(ROOT, "cuembed_amd", "csrc", "cuembed", "include", "row_cache.hpp")) as f:
        struct = re.search(r"struct RowCache \{(.*?)\n\};", f.read(), re.S).group(1)
    members = re.findall(r"^\s+[\w: \*]+?\b(\w+) = [^;]+;", struct, re.M)
    assert members[-6:] == ["state", "state_cache", "state_row_bytes", "state2", "state2_cache", "state2_row_bytes"]
    assert re.search(r"float\* state2 = nullptr;", struct) and re.search(r"int64_t state2_row_bytes = 0;", struct)
    with open(os.path.join(ROOT, "tests", "cpp", "row_cache_state_kat.hip")) as f:
        assert "state2" not in f.read()


@pytest.mark.parametrize("rule", AR.RULES)
@pytest.mark.parametrize("case", AR.TRAINING_CASES, ids=M.case_id)
def test_the_model_keeps_every_rows_moments_current_through_training(case, rule):
    """run_training asserts after every prefetch and update that the current copy of every row's weights and moments is
    what the updates produced, that the host moves only by write-back (or an update in place), and that a clean
    eviction writes nothing.  Here: the sequence contains a dirty eviction and a hit for update everywhere and unplaced
    updates in the one-set case (every row a forward fills is updated in the same step, so its evictions are all dirty:
    the clean ones are in the evicted-moments sequence below); before the flush every host plane is stale, after it
    the host alone is current."""
    model = AR.run_training(AR.AdamCacheModel(M.ROWS, case["width"], case["num_sets"], rule, 0.01))
    placement = S.training_placement(case["num_sets"])
    assert model.place.counters == placement.counters and np.array_equal(model.place.tags, placement.tags)
    assert model.step_number == S.TRAINING_STEPS
    t = model.totals
    assert t["dirty_evicted"] == placement.counters["write_backs"] > 0
    assert t["hits_for_update"] > 0 and t["updates_in_cache"] > 0
    assert (t["updates_in_host"] > 0) == (case["num_sets"] == 1)
    assert {"dirty_eviction", "hit"} <= model.place.events
    assert ("unplaced" in model.place.events) == (case["num_sets"] == 1)
    assert model.host_is_stale_everywhere()
    model.flush()
    assert model.host_is_current() and int(model.place.dirty.sum()) == 0
    # ... and the cache is not needed any more
    model.invalidate()
    now = model.current()
    assert all(np.array_equal(now[k], model.true[k]) for k in AR.PLANES)


@pytest.mark.parametrize("rule", AR.RULES)
def test_evicted_moments_come_back_in_the_model(rule):
    """Update rows 0..39, read 64 other rows through the one set, update rows 0..39 again: all 40 are evicted dirty by
    the read, and the write-back -- not a flush -- carries the weights and both moments to the host."""
    model = AR.AdamCacheModel(M.ROWS, 8, 1, rule)
    assert not np.array_equal(model.host["m"][:, 0], model.host["v"].reshape(M.ROWS, -1)[:, 0])
    rng = np.random.default_rng(1)
    model.apply_update(S.EVICT_UPDATED, rng.standard_normal((40, 8)))
    assert model.totals["updates_in_cache"] == 40
    assert all(not np.array_equal(model.host[k][:40], model.true[k][:40]) for k in AR.PLANES)
    before = {k: model.host[k].copy() for k in AR.PLANES}
    model.prefetch(S.EVICT_READ)
    AR.check_prefetch(model, before)
    assert sorted(model.last["dirty_evicted"]) == S.EVICT_UPDATED.tolist()            # 40 write-backs ...
    assert model.place.counters["write_backs"] == 40 and model.place.counters["unplaced"] == 0
    assert (model.place.slot_of_row[S.EVICT_UPDATED] < 0).all()                       # ... 0 of them still resident
    assert all(np.array_equal(model.host[k][:40], model.true[k][:40]) for k in AR.PLANES)
    assert all((model.host[k][:40] != model.initial[k][:40]).all() for k in AR.PLANES)
    before = {k: model.host[k].copy() for k in AR.PLANES}
    model.apply_update(S.EVICT_UPDATED, rng.standard_normal((40, 8)))
    AR.check_update(model, before, S.EVICT_UPDATED)
    # the second fill evicts 40 of the rows that were only read: clean, nothing is written, the host stays
    assert len(model.last["clean_evicted"]) == 40 and not model.last["dirty_evicted"]
    assert all(np.array_equal(model.host[k], before[k]) for k in AR.PLANES)
    assert model.totals["filled"] == 40 + 64 + 40 and model.step_number == 2
    model.flush()
    assert model.host_is_current()
    assert all(np.array_equal(model.host[k][40:], model.initial[k][40:]) for k in AR.PLANES)


@pytest.mark.parametrize("rule", AR.RULES)
def test_a_set_that_overflows_trains_correctly_in_the_model(rule):
    rows = M.conflict_rows(S.OVERFLOW_SETS, S.OVERFLOW_SET, S.OVERFLOW_ROWS)
    model = AR.AdamCacheModel(M.ROWS, 8, S.OVERFLOW_SETS, rule)
    rng = np.random.default_rng(2)
    model.apply_update(rows[:5], rng.standard_normal((5, 8)))
    model.apply_update(rows, rng.standard_normal((70, 8)))
    assert model.place.counters["hits"] == 5 and model.place.counters["unplaced"] == 6
    assert model.totals["updates_in_host"] == 6 and model.totals["hits_for_update"] == 5
    left_out = rows[model.place.slot_of_row[rows] < 0]
    resident = np.setdiff1d(rows, left_out)
    assert left_out.size == S.OVERFLOW_ROWS - WAYS == 6
    # the six rows without a way are current in the host arrays already, the 64 resident ones only after the flush
    for k in AR.PLANES:
        assert np.array_equal(model.host[k][left_out], model.true[k][left_out])
        assert not np.array_equal(model.host[k][resident], model.true[k][resident])
    model.flush()
    assert model.host_is_current()


def test_reads_carry_both_moments_in_the_model():
    """A forward-only fill brings both moment rows along: a later update that hits finds them in the cache."""
    model = AR.AdamCacheModel(M.ROWS, 8, 4, "rowwise_adam")
    read = np.arange(100, 160)
    model.prefetch(read)
    assert model.totals["filled"] == 60 and int(model.place.dirty.sum()) == 0
    slots = model.place.slot_of_row[read]
    assert np.array_equal(model.cache["m"][slots], model.initial["m"][read])
    assert np.array_equal(model.cache["v"][slots], model.initial["v"][read])
    model.apply_update(read[::3], np.ones((20, 8)))
    assert model.totals["hits_for_update"] == 20 and model.totals["filled"] == 60
    model.flush()
    assert model.host_is_current()
    untouched = np.setdiff1d(np.arange(M.ROWS), read[::3])
    assert all(np.array_equal(model.host[k][untouched], model.initial[k][untouched]) for k in AR.PLANES)
    assert all((model.host[k][read[::3]] != model.initial[k][read[::3]]).all() for k in AR.PLANES)


def test_the_cpp_known_answer_program_has_a_build_of_its_own():
    from cuembed_amd import build
    assert callable(build.build_row_cache_adam_test)
    assert os.path.exists(os.path.join(ROOT, "tests", "cpp", "row_cache_adam_kat.hip"))
