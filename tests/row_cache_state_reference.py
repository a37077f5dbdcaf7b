"""Host model of a DynamicRowCache with a state plane (numpy, no GPU; not a test module).

dynamic_row_cache_reference.CacheModel decides WHERE every row is; this model wraps it and carries the VALUES: a host
and a cached array for the weights and for the optimizer state, moved by the contract of the row exchange --

    fill             host -> cache, weights and state, for_update or not;
    dirty eviction   cache -> host, weights and state;
    clean eviction   nothing is written;
    flush            every dirty slot cache -> host, weights and state;

-- and optimizer_reference.step applied to whichever copy of a row is current: the cached one when the row is resident,
the host one when its set had no way for it.  Next to that it keeps `true_w` / `true_s`, the same steps applied to plain
arrays that never move: what the updates produced.  The arithmetic is fp64 on both sides and the same operations on the
same values, so the two agree EXACTLY wherever the data movement is right; the model checks movement, not the
kernel's rounding (the GPU tests compare bits with the sparse step on device tensors).

The sequences at the bottom are the ones the GPU tests run, so that a CPU test can show what they contain."""
import numpy as np

import dynamic_row_cache_reference as M
import optimizer_reference as R
from cuembed_amd.row_cache import WAYS

RULES = ("adagrad", "rowwise_adagrad")
LR = 0.25


class StateCacheModel:
    def __init__(self, rows, width, num_sets, rule, initial_accumulator_value=0.0, seed=11):
        assert rule in RULES
        self.rule, self.rows, self.width = rule, rows, width
        self.place = M.CacheModel(rows, num_sets)
        rng = np.random.default_rng(seed)
        state_shape = (rows, width) if rule == "adagrad" else (rows,)
        self.host_w = rng.standard_normal((rows, width))
        self.host_s = np.full(state_shape, float(initial_accumulator_value))
        self.cache_w = np.full((num_sets * WAYS, width), np.nan)                # (a slot never filled holds nothing)
        self.cache_s = np.full((num_sets * WAYS,) + state_shape[1:], np.nan)
        self.true_w, self.true_s = self.host_w.copy(), self.host_s.copy()
        #: what the last prefetch did: rows evicted dirty (written back), rows evicted clean, rows filled
        self.last = dict(dirty_evicted=[], clean_evicted=[], filled=[])
        self.totals = dict(dirty_evicted=0, clean_evicted=0, filled=0, updates_in_cache=0, updates_in_host=0,
                           hits_for_update=0)

    # ---- movement ------------------------------------------------------------------------------------------------
    def prefetch(self, indices, for_update=False):
        tags, dirty = self.place.tags.reshape(-1).copy(), self.place.dirty.reshape(-1).copy()
        resident_before = self.place.slot_of_row >= 0
        self.place.prefetch(indices, for_update)
        after = self.place.tags.reshape(-1)
        self.last = dict(dirty_evicted=[], clean_evicted=[], filled=[])
        changed = np.nonzero(after != tags)[0]
        for slot in changed:                                   # victims first: cache -> host, both planes
            old = int(tags[slot])
            if old >= 0 and dirty[slot]:
                self.host_w[old], self.host_s[old] = self.cache_w[slot], self.cache_s[slot]
                self.last["dirty_evicted"].append(old)
            elif old >= 0:
                self.last["clean_evicted"].append(old)
        for slot in changed:                                   # then the fills: host -> cache, both planes
            new = int(after[slot])
            self.cache_w[slot], self.cache_s[slot] = self.host_w[new], self.host_s[new]
            self.last["filled"].append(new)
        # no row is both written back and fetched by one prefetch: the two loops need no order among themselves
        assert not set(self.last["dirty_evicted"]) & set(self.last["filled"])
        for key, rows in self.last.items():
            self.totals[key] += len(rows)
        if for_update:
            idx = np.asarray(indices, np.int64).reshape(-1)
            idx = np.unique(idx[(idx >= 0) & (idx < self.rows)])
            self.totals["hits_for_update"] += int(resident_before[idx].sum())

    def flush(self):
        slots = np.nonzero((self.place.tags.reshape(-1) >= 0) & (self.place.dirty.reshape(-1) != 0))[0]
        rows = self.place.tags.reshape(-1)[slots]
        self.host_w[rows], self.host_s[rows] = self.cache_w[slots], self.cache_s[slots]
        self.place.flush()

    def invalidate(self):
        self.place.invalidate()
        self.cache_w[:], self.cache_s[:] = np.nan, np.nan

    # ---- the step ------------------------------------------------------------------------------------------------
    def apply_update(self, ids, grads, lr=LR):
        """prefetch(ids, for_update=True), then the rule on the current copy of every named row (ids distinct)."""
        ids = np.asarray(ids, np.int64).reshape(-1)
        assert np.unique(ids).size == ids.size
        grads = np.asarray(grads, np.float64).reshape(ids.size, self.width)
        self.prefetch(ids, for_update=True)
        slots = self.place.slot_of_row[ids]
        cached, direct = slots >= 0, slots < 0
        for w, s, at, g in ((self.cache_w, self.cache_s, slots[cached], grads[cached]),
                            (self.host_w, self.host_s, ids[direct], grads[direct]),       # no way: in place, over PCIe
                            (self.true_w, self.true_s, ids, grads)):
            if at.size:
                w[at], _, s[at] = R.step(self.rule, w[at], g, s[at], lr)
        self.totals["updates_in_cache"] += int(cached.sum())
        self.totals["updates_in_host"] += int(direct.sum())

    # ---- what is current -----------------------------------------------------------------------------------------
    def current(self):
        """(weights, state) with every row taken from its current copy: the slot of a resident row, else the host."""
        w, s = self.host_w.copy(), self.host_s.copy()
        slots = np.nonzero(self.place.tags.reshape(-1) >= 0)[0]
        rows = self.place.tags.reshape(-1)[slots]
        w[rows], s[rows] = self.cache_w[slots], self.cache_s[slots]
        return w, s


# ---- the sequences of tests/test_gpu_row_cache_state.py --------------------------------------------------------------
#: (element type, width, sets, index type) of the training-parity test: 48-byte rows in one set, 64-byte rows in four,
#: and 12-byte rows -- 4-byte lanes, several slices per lane -- in four
TRAINING_CASES = [dict(kind="f16", width=24, num_sets=1, index="i32"), dict(kind="f32", width=16, num_sets=4, index="i64"),
                  dict(kind="f16", width=6, num_sets=4, index="i32")]
TRAINING_STEPS = 5
EVICT_UPDATED = np.arange(40)                    # "an evicted accumulator comes back": rows updated, ...
EVICT_READ = np.arange(1000, 1064)               # ... 64 rows read through the one set, which evicts all 40 dirty
OVERFLOW_SETS, OVERFLOW_SET, OVERFLOW_ROWS = 4, 2, 70


def training_batches():
    return M.batches(seed=2, foreign=False)[:TRAINING_STEPS]


def training_placement(num_sets):
    """CacheModel after the training-parity sequence: every batch prefetched once for the forward and its distinct
    rows once for the update."""
    model = M.CacheModel(M.ROWS, num_sets)
    for idx in training_batches():
        model.prefetch(idx)
        model.prefetch(np.unique(idx), for_update=True)
    return model


def run_training(model, seed=5):
    """The training-parity sequence on a StateCacheModel, with its invariants asserted after every step."""
    rng = np.random.default_rng(seed)
    for idx in training_batches():
        before = model.host_s.copy()
        model.prefetch(idx)
        check_prefetch(model, before)
        ids = np.unique(idx)
        before = model.host_s.copy()
        model.apply_update(ids, rng.standard_normal((ids.size, model.width)))
        check_update(model, before, ids)
    return model


def check_prefetch(model, host_state_before):
    """After a prefetch: the current copy of every row is what the updates produced, the host state changed only where
    a dirty row was written back, and a clean eviction wrote nothing."""
    w, s = model.current()
    assert np.array_equal(w, model.true_w) and np.array_equal(s, model.true_s)
    moved = np.nonzero((model.host_s != host_state_before).reshape(model.rows, -1).any(axis=1))[0]
    assert set(moved.tolist()) <= set(model.last["dirty_evicted"])
    clean = np.asarray(model.last["clean_evicted"], np.int64)
    assert np.array_equal(model.host_s[clean], host_state_before[clean])
    assert np.array_equal(model.host_s[clean], model.true_s[clean])           # (it was current all along)


def check_update(model, host_state_before, ids):
    """After an update: as check_prefetch, except that rows without a way were updated in the host arrays."""
    w, s = model.current()
    assert np.array_equal(w, model.true_w) and np.array_equal(s, model.true_s)
    direct = ids[model.place.slot_of_row[ids] < 0]
    moved = np.nonzero((model.host_s != host_state_before).reshape(model.rows, -1).any(axis=1))[0]
    assert set(moved.tolist()) <= set(model.last["dirty_evicted"]) | set(direct.tolist())
