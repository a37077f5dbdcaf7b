"""DynamicRowCache without a GPU: the set function, the argument checks (raised before any device is asked for), the
host model's coverage of the GPU cases, and the build lists."""
import ctypes

import numpy as np
import pytest
import torch

import dynamic_row_cache_reference as M
from cuembed_amd import build
from cuembed_amd.row_cache import DynamicRowCache, cache_set_of


def test_cache_set_of_is_a_pure_function_into_the_sets():
    ids = np.arange(10_000)
    for num_sets in (1, 3, 4, 16, 1000, 1 << 24):
        sets = cache_set_of(ids, num_sets)
        assert sets.dtype == np.int64 and sets.min() >= 0 and sets.max() < num_sets
        assert np.array_equal(sets, cache_set_of(ids, num_sets))
        assert [cache_set_of(int(r), num_sets) for r in ids[:500]] == sets[:500].tolist()      # int == array
    far = [(1 << 31) - 1, 1 << 31, (1 << 40) + 3, (1 << 62) - 1]
    assert [cache_set_of(r, 1000) for r in far] == cache_set_of(np.array(far), 1000).tolist()
    assert all(isinstance(cache_set_of(r, 16), int) for r in (0, 7, 1 << 40))
    # not row % num_sets, and it spreads consecutive ids: every one of 16 sets is populated, none starved
    spread = np.bincount(cache_set_of(ids, 16), minlength=16)
    assert spread.min() > 0 and spread.min() > 10_000 // 16 // 2
    assert not np.array_equal(cache_set_of(ids, 16), ids % 16)
    for bad in (0, -1, (1 << 24) + 1):
        with pytest.raises(ValueError, match="num_sets"):
            cache_set_of(3, bad)


def test_the_library_computes_the_same_sets():
    from cuembed_amd import _lib
    L = _lib.lib()
    rows = list(range(0, 5000, 37)) + [(1 << 31) + 5, (1 << 40) + 3]
    for num_sets in (1, 4, 16, 1000):
        assert [L.cuembed_cache_set_of(r, num_sets) for r in rows] == cache_set_of(np.array(rows), num_sets).tolist()
    assert int(L.cuembed_row_cache_workspace_bytes(320, 5000, 4)) > 320 * 8 * 3
    assert int(L.cuembed_row_cache_workspace_bytes(0, 5000, 4)) >= 0


def test_argument_errors_come_before_any_device_check():
    table = torch.zeros((8, 4), dtype=torch.float32)            # (not pinned: no GPU is needed to get this far)
    with pytest.raises(ValueError, match="PINNED"):
        DynamicRowCache(table, num_sets=1)
    with pytest.raises(TypeError, match="float32, float16 or bfloat16"):
        DynamicRowCache(table.double(), num_sets=1)
    with pytest.raises(TypeError, match="float32, float16 or bfloat16"):
        DynamicRowCache(table.long(), num_sets=1)
    for bad in (0, -4, (1 << 24) + 1):
        with pytest.raises(ValueError, match="num_sets"):
            DynamicRowCache(table, num_sets=bad)
    for bad in (1.5, "4", True):
        with pytest.raises(TypeError, match="num_sets"):
            DynamicRowCache(table, num_sets=bad)
    with pytest.raises(ValueError, match="2-D"):
        DynamicRowCache(torch.zeros(8), num_sets=1)
    with pytest.raises(ValueError, match="contiguous"):
        DynamicRowCache(torch.zeros((4, 8)).t(), num_sets=1)
    with pytest.raises(ValueError, match="multiple of 4"):
        DynamicRowCache(torch.zeros((8, 3), dtype=torch.float16), num_sets=1)
    with pytest.raises(TypeError, match="Tensor"):
        DynamicRowCache(np.zeros((8, 4), np.float32), num_sets=1)


@pytest.mark.parametrize("num_sets", [1, 4])
def test_the_gpu_cases_contain_every_event_class(num_sets):
    """What the GPU state-parity test can only show if it happens: a hit, a clean eviction, a dirty eviction with
    write-back, an unplaced row, a hit protected in a set that overflows in the same batch, an empty way taken and an
    index outside the table.  One set sees them all in the shared sequence; four sets see all but the overflow, which
    the GPU suite's set-overflow test forces with rows of one set."""
    case = next(c for c in M.CASES if c["num_sets"] == num_sets)
    model, snapshots = M.model_trace(case)
    assert len(snapshots) == M.STEPS and model.clock == M.STEPS + 1
    want = M.EVENTS if num_sets == 1 else M.EVENTS - {"unplaced", "protected_hit"}
    assert want <= model.events, sorted(want - model.events)
    if num_sets == 4:
        forced = M.CacheModel(M.ROWS, 4)
        rows = M.conflict_rows(4, 2, 70)
        forced.prefetch(rows[:5])
        forced.prefetch(rows)
        assert {"unplaced", "protected_hit"} <= forced.events and forced.counters["unplaced"] == 70 - 64
    # the model's own invariants: slot_of_row and tags are inverse to each other, stamps never pass the clock
    tagged = np.nonzero(model.tags.reshape(-1) >= 0)[0]
    assert np.array_equal(model.slot_of_row[model.tags.reshape(-1)[tagged]], tagged)
    assert (model.slot_of_row >= 0).sum() == tagged.size and model.stamps.max() < model.clock
    assert model.counters["hits"] + model.counters["misses"] == sum(
        np.unique(b[(b >= 0) & (b < M.ROWS)]).size for b in M.batches())


def test_the_model_flushes_and_invalidates():
    model = M.CacheModel(100, 1)
    model.prefetch([3, 5, 5, 7], for_update=True)
    model.prefetch([9])
    assert model.dirty.sum() == 3 and model.counters["misses"] == 4
    model.flush()
    assert model.dirty.sum() == 0 and model.counters["write_backs"] == 3 and (model.tags >= 0).sum() == 4
    model.invalidate()
    assert (model.tags == -1).all() and (model.slot_of_row == -1).all() and model.clock == 3


def test_the_new_unit_is_built_and_declared():
    assert "c_api_row_cache.hip" in build.UNITS
    L = ctypes.CDLL(build.build())
    for name in ("cuembed_row_cache_workspace_bytes", "cuembed_row_cache_prefetch", "cuembed_row_cache_flush",
                 "cuembed_cache_set_of"):
        assert hasattr(L, name), name
