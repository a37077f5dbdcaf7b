"""Host model of an AdamRowCache (numpy, no GPU; not a test module): row_cache_state_reference.StateCacheModel's
counterpart with TWO state arrays.

dynamic_row_cache_reference.CacheModel decides WHERE every row is; this model wraps it and carries the VALUES: a host
and a cached array for the weights, for exp_avg and for exp_avg_sq, moved by the contract of the row exchange --

    fill             host -> cache, weights and both moments, for_update or not;
    dirty eviction   cache -> host, weights and both moments;
    clean eviction   nothing is written;
    flush            every dirty slot cache -> host, weights and both moments;

-- and adam_reference.step applied to whichever copy of a row is current: the cached one when the row is resident, the
host one when its set had no way for it.  Next to that it keeps `true_w` / `true_m` / `true_v`, the same steps applied to
plain arrays that never move: what the updates produced.  The arithmetic is fp64 on both sides and the same operations
on the same values, so the two agree EXACTLY wherever the data movement is right; the model checks movement, not the
kernel's rounding (the GPU tests compare bits with the sparse Adam step on device tensors).  The initial moments differ
row by row and from each other, so that a plane that is swapped, re-initialised or moved with the other's row size shows.

The sequences are those of row_cache_state_reference (the ones the GPU tests run)."""
import numpy as np

import adam_reference as A
import dynamic_row_cache_reference as M
import row_cache_state_reference as S
from cuembed_amd.row_cache import WAYS

RULES = A.RULES
LR = 0.05
BETAS = (0.9, 0.999)
PLANES = ("w", "m", "v")


def initial_moments(rows, width, rule, seed=13):
    """(exp_avg [rows, width], exp_avg_sq [rows, width] or [rows]) that differ row by row and from each other; the
    second moment is positive.  float32 values (what an AdamRowCache is given), as float64."""
    rng = np.random.default_rng(seed)
    m = rng.uniform(-1.0, 1.0, (rows, width)).astype(np.float32)
    v = rng.uniform(0.25, 2.0, (rows, width) if rule == "adam" else (rows,)).astype(np.float32)
    return m.astype(np.float64), v.astype(np.float64)


class AdamCacheModel:
    def __init__(self, rows, width, num_sets, rule, weight_decay=0.0, seed=11):
        assert rule in RULES
        self.rule, self.rows, self.width, self.weight_decay = rule, rows, width, weight_decay
        self.place = M.CacheModel(rows, num_sets)
        self.step_number = 0
        m, v = initial_moments(rows, width, rule)
        self.host = dict(w=np.random.default_rng(seed).standard_normal((rows, width)), m=m, v=v)
        #: (a slot never filled holds nothing)
        self.cache = {k: np.full((num_sets * WAYS,) + a.shape[1:], np.nan) for k, a in self.host.items()}
        self.true = {k: a.copy() for k, a in self.host.items()}
        self.initial = {k: a.copy() for k, a in self.host.items()}
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
        for slot in changed:                                   # victims first: cache -> host, all three planes
            old = int(tags[slot])
            if old >= 0 and dirty[slot]:
                for k in PLANES:
                    self.host[k][old] = self.cache[k][slot]
                self.last["dirty_evicted"].append(old)
            elif old >= 0:
                self.last["clean_evicted"].append(old)
        for slot in changed:                                   # then the fills: host -> cache, all three planes
            new = int(after[slot])
            for k in PLANES:
                self.cache[k][slot] = self.host[k][new]
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
        for k in PLANES:
            self.host[k][rows] = self.cache[k][slots]
        self.place.flush()

    def invalidate(self):
        self.place.invalidate()
        for k in PLANES:
            self.cache[k][:] = np.nan

    # ---- the step ------------------------------------------------------------------------------------------------
    def apply_update(self, ids, grads, lr=LR):
        """The clock moves on (on every call), prefetch(ids, for_update=True), then the rule on the current copy of
        every named row (ids distinct)."""
        ids = np.asarray(ids, np.int64).reshape(-1)
        assert np.unique(ids).size == ids.size
        grads = np.asarray(grads, np.float64).reshape(ids.size, self.width)
        self.step_number += 1
        sc = A.scalars(lr, A.bias_factor(self.step_number, BETAS), BETAS, 1e-8, self.weight_decay)
        self.prefetch(ids, for_update=True)
        slots = self.place.slot_of_row[ids]
        cached, direct = slots >= 0, slots < 0
        for arrays, at, g in ((self.cache, slots[cached], grads[cached]),
                              (self.host, ids[direct], grads[direct]),          # no way: in place, over PCIe
                              (self.true, ids, grads)):
            if at.size:
                r = A.step(self.rule, arrays["w"][at], g, arrays["m"][at], arrays["v"][at], sc)
                arrays["w"][at], arrays["m"][at], arrays["v"][at] = r["w"], r["m"], r["v"]
        self.totals["updates_in_cache"] += int(cached.sum())
        self.totals["updates_in_host"] += int(direct.sum())

    # ---- what is current -----------------------------------------------------------------------------------------
    def current(self):
        """{plane: array} with every row taken from its current copy: the slot of a resident row, else the host."""
        out = {k: a.copy() for k, a in self.host.items()}
        slots = np.nonzero(self.place.tags.reshape(-1) >= 0)[0]
        rows = self.place.tags.reshape(-1)[slots]
        for k in PLANES:
            out[k][rows] = self.cache[k][slots]
        return out

    def host_is_current(self):
        return all(np.array_equal(self.host[k], self.true[k]) for k in PLANES)

    def host_is_stale_everywhere(self):
        """Every plane of the host differs from what the updates produced."""
        return all(not np.array_equal(self.host[k], self.true[k]) for k in PLANES)


# ---- the sequences of tests/test_gpu_row_cache_adam.py ---------------------------------------------------------------
#: row_cache_state_reference's cases and one bf16 case: 16-byte rows, one lane each, of the third element type
TRAINING_CASES = S.TRAINING_CASES + [dict(kind="bf16", width=8, num_sets=4, index="i64")]
WEIGHT_DECAYS = (0.0, 0.01)


def run_training(model, seed=5):
    """The training-parity sequence on an AdamCacheModel, with its invariants asserted after every step."""
    rng = np.random.default_rng(seed)
    for idx in S.training_batches():
        before = {k: model.host[k].copy() for k in PLANES}
        model.prefetch(idx)
        check_prefetch(model, before)
        ids = np.unique(idx)
        before = {k: model.host[k].copy() for k in PLANES}
        model.apply_update(ids, rng.standard_normal((ids.size, model.width)))
        check_update(model, before, ids)
    return model


def _moved(model, before):
    """Rows whose host copy of any plane changed."""
    rows = set()
    for k in PLANES:
        rows |= set(np.nonzero((model.host[k] != before[k]).reshape(model.rows, -1).any(axis=1))[0].tolist())
    return rows


def check_prefetch(model, host_before):
    """After a prefetch: the current copy of every row is what the updates produced in all three planes, the host
    changed only where a dirty row was written back, and a clean eviction wrote nothing."""
    now = model.current()
    for k in PLANES:
        assert np.array_equal(now[k], model.true[k]), k
    assert _moved(model, host_before) <= set(model.last["dirty_evicted"])
    clean = np.asarray(model.last["clean_evicted"], np.int64)
    for k in PLANES:
        assert np.array_equal(model.host[k][clean], host_before[k][clean])
        assert np.array_equal(model.host[k][clean], model.true[k][clean])           # (it was current all along)


def check_update(model, host_before, ids):
    """After an update: as check_prefetch, except that rows without a way were updated in the host arrays."""
    now = model.current()
    for k in PLANES:
        assert np.array_equal(now[k], model.true[k]), k
    direct = ids[model.place.slot_of_row[ids] < 0]
    assert _moved(model, host_before) <= set(model.last["dirty_evicted"]) | set(direct.tolist())
