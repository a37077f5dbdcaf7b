"""Host model of cuembed_amd.row_cache.DynamicRowCache's contract (numpy, no GPU), and the case table that the host and
the GPU tests share.  The model keeps the cache's state -- tags, stamps, dirty, slot_of_row, clock, counters -- and
records which kinds of event each prefetch produced, so that a CPU test can require the GPU cases to cover them all."""
import itertools

import numpy as np

from cuembed_amd.row_cache import WAYS, cache_set_of

COUNTERS = ("hits", "misses", "evictions", "write_backs", "unplaced")
EVENTS = {"hit", "clean_eviction", "dirty_eviction", "unplaced", "protected_hit", "empty_way", "out_of_table"}


class CacheModel:
    def __init__(self, rows, num_sets):
        self.rows, self.num_sets = rows, num_sets
        self.tags = np.full((num_sets, WAYS), -1, np.int64)
        self.stamps = np.zeros((num_sets, WAYS), np.uint32)
        self.dirty = np.zeros((num_sets, WAYS), np.uint8)
        self.slot_of_row = np.full(rows, -1, np.int32)
        self.clock = 1
        self.counters = dict.fromkeys(COUNTERS, 0)
        self.events = set()

    def prefetch(self, indices, for_update=False):
        idx = np.asarray(indices, np.int64).reshape(-1)
        t = self.clock
        inside = (idx >= 0) & (idx < self.rows)
        if not inside.all():
            self.events.add("out_of_table")
        distinct = np.unique(idx[inside])
        resident = self.slot_of_row[distinct] >= 0
        for slot in self.slot_of_row[distinct[resident]]:                       # 1. hits first
            self.stamps.flat[slot] = t
            if for_update:
                self.dirty.flat[slot] = 1
            self.events.add("hit")
        self.counters["hits"] += int(resident.sum())
        self.counters["misses"] += int((~resident).sum())
        hit_sets = set(cache_set_of(distinct[resident], self.num_sets).tolist())
        for row in distinct[~resident]:                                         # 2. then the misses, ascending
            s = int(cache_set_of(int(row), self.num_sets))
            free = np.nonzero(self.stamps[s] < t)[0]
            if free.size == 0:
                self.counters["unplaced"] += 1
                self.events.add("unplaced")
                if s in hit_sets:
                    self.events.add("protected_hit")
                continue
            way = int(free[np.argmin(self.stamps[s][free])])                    # smallest (stamp, way)
            old = int(self.tags[s, way])
            if old >= 0:                                                        # 3. placing a row
                self.counters["evictions"] += 1
                self.slot_of_row[old] = -1
                if self.dirty[s, way]:
                    self.counters["write_backs"] += 1
                self.events.add("dirty_eviction" if self.dirty[s, way] else "clean_eviction")
            else:
                self.events.add("empty_way")
            self.tags[s, way], self.stamps[s, way], self.dirty[s, way] = row, t, int(for_update)
            self.slot_of_row[row] = s * WAYS + way
        self.clock += 1

    def flush(self):
        self.counters["write_backs"] += int(((self.tags >= 0) & (self.dirty != 0)).sum())
        self.dirty[:] = 0

    def invalidate(self):
        self.tags[:], self.stamps[:], self.dirty[:], self.slot_of_row[:] = -1, 0, 0, -1


# ---- the cases of the GPU tests ---------------------------------------------------------------------------------
ROWS, BATCH, HOTS, STEPS = 5000, 64, 5, 6
#: (element type, width): rows of 64 and 48 bytes move in 16-byte lanes, of 40 bytes in 8-byte and of 12 bytes in 4-byte
#: lanes
SHAPES = [("f32", 16), ("f16", 24), ("f16", 20), ("f16", 6)]
CASES = [dict(kind=kind, width=width, num_sets=num_sets, index=index)
         for (kind, width), num_sets, index in itertools.product(SHAPES, (1, 4), ("i32", "i64"))]
#: which prefetches of the state-parity sequence are for_update
FOR_UPDATE = (False, True, False, True, False, False)


def case_id(case):
    return "%s-w%d-s%d-%s" % (case["kind"], case["width"], case["num_sets"], case["index"])


def batches(seed=0, foreign=True, rows=ROWS):
    """STEPS skewed batches of BATCH x HOTS lookups: 60 % from a hot set of 40 rows that drifts from step to step, the
    rest uniform over the table.  foreign=True plants indices outside the table (never to be run through a forward)."""
    rng = np.random.default_rng(1234 + seed)
    hot = rng.choice(rows, 40, replace=False)
    out = []
    for step in range(STEPS):
        hot[rng.integers(0, 40, 8)] = rng.integers(0, rows, 8)        # the hot set drifts
        idx = np.where(rng.random((BATCH, HOTS)) < 0.6, hot[rng.integers(0, 40, (BATCH, HOTS))],
                       rng.integers(0, rows, (BATCH, HOTS))).astype(np.int64)
        if foreign and step % 2 == 1:
            idx[3, 1], idx[40, 4] = -1, rows + step
        out.append(idx)
    return out


def model_trace(case, seed=0):
    """The model after the state-parity sequence of a case, with a snapshot after every prefetch."""
    model = CacheModel(ROWS, case["num_sets"])
    snapshots = []
    for idx, for_update in zip(batches(seed), FOR_UPDATE):
        model.prefetch(idx, for_update)
        snapshots.append((model.tags.copy(), model.stamps.copy(), model.dirty.copy(), model.slot_of_row.copy(),
                          dict(model.counters), model.clock))
    return model, snapshots


def conflict_rows(num_sets, target_set, count, rows=ROWS):
    """The first `count` table rows that cache_set_of maps to `target_set`."""
    ids = np.arange(rows)
    found = ids[cache_set_of(ids, num_sets) == target_set]
    assert found.size >= count
    return found[:count]
