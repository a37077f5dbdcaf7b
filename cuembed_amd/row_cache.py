"""Table-row caching hook for tables that do not live in this GPU's HBM (extension; the reference
lists an embedding cache as future work, README.md:111-112).

    table = torch.empty((rows, width), dtype=torch.float16).pin_memory()      # host-resident, read over PCIe
    cached = CachedHostTable(table, device="cuda:0", capacity_rows=1_000_000)
    cached.cache_most_frequent(sample_of_recent_indices)                       # the caller's policy
    out = cached.forward(indices, num_hots=64)                                 # == EmbeddingForward on the table

How it works (cuembed::TranslateIndicesForRowCache): EmbeddingForward addresses a row as
params + int64(index) * width, so an index of (cache_rows - params) / width + slot reaches row
`slot` of a device buffer through the table's own base pointer.  The indices of a batch are
rewritten with one small kernel (slot_of_row[] lookup) and the unmodified forward kernel then reads
cached rows from HBM and only the others over PCIe.  Results are bit-identical to running on the
table itself as long as the cached copies are current: there is no staleness guard, the caller must
call refresh() after updating table rows.  Lookup indices outside the table are passed through untouched.

DynamicRowCache (below) is the cache that manages itself: set-associative, LRU, write-back, filled and evicted on the
device from each batch's own indices, so that a host-resident table can be read AND trained with no host read-back:

    cache = DynamicRowCache(table, device="cuda:0", num_sets=16384)              # 64 ways per set: 1,048,576 rows
    out = cache.forward(indices, num_hots=64)                                    # prefetch + translate + forward
    cache.apply_sgd(inverse_mapping, grad_embedding, lr=0.1, last_id=remapped[-1:])   # sparse SGD step through the cache
    cache.flush()                                                                # dirty rows back to the host table

With rule="adagrad" / "rowwise_adagrad" the optimizer's fp32 state rides on the cache slots as a second plane and
cache.apply_update(...) is that rule's step through the cache; cache.state is the host side of the state.

AdamRowCache is the same cache for the Adam family: the two moments ride on the cache slots as two state planes, and
cache.apply_update(...) is SparseAdamUpdater.apply through the cache (clock, prefetch, one translate for the three
planes, one placed Adam launch).

Both take stochastic_rounding=True, seed=... for a float16 / bfloat16 table: the step through the cache then rounds
stochastically with the bits of (seed, cache.rounding_step, TABLE ROW, column) -- the step carries the batch's own ids
next to the translated ones to name them -- and gives, bit for bit, what optim.SparseUpdater / SparseAdamUpdater with
stochastic_rounding=True and the same seed give on device copies."""
import ctypes

import torch

from . import _lib
from . import ops as _ops
from .optim import _check_rounding


class CachedHostTable:
    def __init__(self, host_table, device="cuda", capacity_rows=1 << 20):
        if host_table.is_cuda or not host_table.is_pinned() or host_table.dim() != 2 or not host_table.is_contiguous():
            raise ValueError("host_table must be a contiguous 2-D tensor in PINNED host memory (tensor.pin_memory())")
        if host_table.dtype not in _ops._ELEM:
            raise TypeError("table must be float32, float16 or bfloat16")
        self.table = host_table
        self.device = torch.device(device)
        if self.device.index is None:   # "cuda" -> the current device, so that it compares equal to tensor.device
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.rows, self.width = host_table.shape
        self.capacity = int(capacity_rows)
        row_bytes = self.width * host_table.element_size()
        if row_bytes % 4:
            raise ValueError("row size must be a multiple of 4 bytes")
        # the cache must differ from the table by a whole number of rows: over-allocate by one row
        # and start where (cache - table) % row_bytes == 0
        self._raw = torch.empty(((self.capacity + 1) * row_bytes,), dtype=torch.uint8, device=self.device)
        shift = (host_table.data_ptr() - self._raw.data_ptr()) % row_bytes
        self.cache = self._raw[shift:shift + self.capacity * row_bytes].view(host_table.dtype).view(self.capacity, self.width)
        assert (self.cache.data_ptr() - host_table.data_ptr()) % row_bytes == 0
        self.cache_row_offset = (self.cache.data_ptr() - host_table.data_ptr()) // row_bytes
        self.slot_of_row = torch.full((self.rows,), -1, dtype=torch.int32, device=self.device)
        self.cached_ids = torch.empty((0,), dtype=torch.int64, device=self.device)

    def cache_rows(self, row_ids):
        """Make `row_ids` (distinct table rows, at most capacity_rows) the cached set.  Raises on more ids
        than the cache holds and on ids outside the table (one host read-back; this is not the step path)."""
        row_ids = row_ids.to(device=self.device, dtype=torch.int64).reshape(-1)
        if row_ids.numel() > self.capacity:
            raise ValueError("%d rows do not fit a cache of %d rows" % (row_ids.numel(), self.capacity))
        if row_ids.numel() and (int(row_ids.min()) < 0 or int(row_ids.max()) >= self.rows):
            raise IndexError("row ids must lie in [0, %d)" % self.rows)
        self.slot_of_row.fill_(-1)
        self.slot_of_row[row_ids] = torch.arange(row_ids.numel(), dtype=torch.int32, device=self.device)
        self.cached_ids = row_ids
        self.refresh()

    def cache_most_frequent(self, indices):
        """Policy helper: cache the most frequently looked-up rows of a sample of indices."""
        counts = torch.bincount(indices.to(self.device).reshape(-1).long(), minlength=self.rows)
        k = min(self.capacity, int((counts > 0).sum().item()))
        self.cache_rows(torch.topk(counts, k).indices)

    def refresh(self):
        """Re-copy the cached rows from the host table (after the table was updated)."""
        if self.cached_ids.numel():
            ids = self.cached_ids.cpu()
            self.cache[: ids.numel()].copy_(self.table[ids].pin_memory(), non_blocking=True)

    def translate(self, indices):
        """indices (int32 / int64 device tensor) -> int64 indices that address cached rows in HBM."""
        return self._translate(indices, self.cache_row_offset)

    def _translate(self, indices, row_offset):
        """translate() for a plane whose slots lie `row_offset` of its rows from its home tensor."""
        _ops._check_dev("indices", indices, self.device)
        it = _ops._index_code("indices", indices)
        out = torch.empty(indices.shape, dtype=torch.int64, device=self.device)
        if indices.numel():
            with torch.cuda.device(self.device):
                _lib.lib().cuembed_translate_indices_for_row_cache(
                    ctypes.c_void_p(indices.data_ptr()), it, indices.numel(), ctypes.c_void_p(self.slot_of_row.data_ptr()),
                    self.rows, row_offset, ctypes.c_void_p(out.data_ptr()), _ops._stream(indices))
        return out

    def forward(self, indices, offsets=None, weights=None, batch_size=None, num_hots=0, mode="sum", use_cache=True,
                out=None):
        """EmbeddingForward on the host-resident table (zero-copy over PCIe), cached rows from HBM.
        use_cache=False reads every row from the host table (for comparison)."""
        if mode not in _ops._MODES:
            raise ValueError("mode must be 'sum', 'mean' or 'concat'")
        m = _ops._MODES[mode]
        idx = self.translate(indices) if use_cache else indices
        _ops._check_dev("indices", idx, self.device)
        it = _ops._index_code("indices", idx)
        ot = 0
        if offsets is not None:
            _ops._check_dev("offsets", offsets, self.device)
            ot = _ops._index_code("offsets", offsets)
            if batch_size is None:
                batch_size = offsets.numel() - 1
        elif batch_size is None:
            batch_size = idx.numel() // num_hots
        if weights is not None:
            _ops._check_dev("weights", weights, self.device)
            if weights.dtype != self.table.dtype:
                raise TypeError("weights must have the table's dtype")
        shape = (batch_size, num_hots, self.width) if m == _ops.CONCAT else (batch_size, self.width)
        if out is None:
            out = torch.empty(shape, dtype=self.table.dtype, device=self.device)
        if batch_size > 0:
            with torch.cuda.device(self.device):
                _lib.lib().cuembed_embedding_forward(
                    ctypes.c_void_p(self.table.data_ptr()), _ops._ELEM[self.table.dtype], self.width, _ops._ptr(idx), it,
                    _ops._ptr(offsets), ot, _ops._ptr(weights), batch_size, num_hots, m, 0, _ops._ptr(out),
                    _ops._stream(idx))
        return out


WAYS = 64    # cuembed::kRowCacheWays: one wavefront owns one set, lane = way
_MASK64 = (1 << 64) - 1
_MIX1, _MIX2 = 0x9E3779B97F4A7C15, 0xD6E8FEB86659FD93
#: names of the cache's device words (cuembed::RowCacheWord), in order
STAT_WORDS = ("clock", "hits", "misses", "evictions", "write_backs", "unplaced", "moves", "batch_count", "overflow")


def cache_set_of(row, num_sets):
    """The set of a table row (cuembed::CacheSetOf, mirrored on the host): two multiply / xor-shift rounds of the 64-bit
    row id, reduced to [0, num_sets) by multiply-shift, so num_sets need not be a power of two:

        h = row * 0x9E3779B97F4A7C15;  h ^= h >> 32;  h *= 0xD6E8FEB86659FD93;  h ^= h >> 32      (mod 2**64)
        set = ((h >> 32) * num_sets) >> 32

    `row`: an int (returns an int) or anything numpy makes an integer array of (returns an int64 array)."""
    num_sets = int(num_sets)
    if not 1 <= num_sets <= 1 << 24:
        raise ValueError("num_sets must be in [1, 2**24], got %d" % num_sets)
    if isinstance(row, int):
        h = ((row & _MASK64) * _MIX1) & _MASK64
        h ^= h >> 32
        h = (h * _MIX2) & _MASK64
        h ^= h >> 32
        return ((h >> 32) * num_sets) >> 32
    import numpy as np
    h = np.asarray(row).astype(np.int64).astype(np.uint64) * np.uint64(_MIX1)      # (array arithmetic wraps mod 2**64)
    h ^= h >> np.uint64(32)
    h *= np.uint64(_MIX2)
    h ^= h >> np.uint64(32)
    return (((h >> np.uint64(32)) * np.uint64(num_sets)) >> np.uint64(32)).astype(np.int64)


def _check_table_arguments(host_table, num_sets):
    """What a device-managed cache asks of its table and its size, short of where the table lives."""
    if not isinstance(host_table, torch.Tensor):
        raise TypeError("host_table must be a torch.Tensor")
    if host_table.dtype not in _ops._ELEM:
        raise TypeError("table must be float32, float16 or bfloat16")
    if isinstance(num_sets, bool) or not isinstance(num_sets, int):
        raise TypeError("num_sets must be an int")
    if not 1 <= num_sets <= 1 << 24:
        raise ValueError("num_sets must be in [1, 2**24], got %d" % num_sets)
    if host_table.dim() != 2 or not host_table.is_contiguous() or host_table.shape[0] < 1:
        raise ValueError("host_table must be a contiguous 2-D tensor with at least one row")
    if (host_table.shape[1] * host_table.element_size()) % 4:
        raise ValueError("row size must be a multiple of 4 bytes")


def _check_pinned(name, t):
    if t.is_cuda or not t.is_pinned():
        raise ValueError("%s must live in PINNED host memory (tensor.pin_memory())" % name)


class DynamicRowCache(CachedHostTable):
    """Device-managed cache of a host-resident table: `num_sets` sets of 64 ways (capacity_rows = 64 * num_sets) in HBM,
    LRU per set, write-back.  All state lives on the device -- tags int64 [S, 64] (-1 = empty), stamps uint32 [S, 64]
    (0 = never used), dirty uint8 [S, 64], slot_of_row int32 [rows], a clock word (first value 1) and counter words --
    and every call but stats() is stream-ordered with no host read-back.

    prefetch(indices, for_update=False), with t the clock and D the distinct rows of `indices` inside [0, rows):
      1. hits first: every resident row of D gets stamp = t; a row of this batch is never evicted by this batch;
      2. then the misses of each set (cache_set_of) in ascending row id: each takes the way with the smallest
         (stamp, way) among ways with stamp < t; if there is none the row stays uncached and `unplaced` goes up by one;
      3. placing a row: a valid dirty victim is stored to the host table, slot_of_row[old] = -1, the new row is loaded
         host -> cache, tag / stamp / slot_of_row are set and dirty = for_update;
      4. for_update=True marks resident hits dirty too;
      5. clock += 1.
    Indices outside the table are ignored by prefetch and passed through by translate.

    A set holds at most 64 rows of one batch: size the cache so that no set sees more; rows that
    do not fit are served from the host table over PCIe -- reads and updates alike -- so nothing is ever wrong or lost,
    only slower, and stats()["unplaced"] says how often.

    The cached copy of a dirty row is the only current one: read the host table only after flush() and a synchronise.

    rule="adagrad" / "rowwise_adagrad" (ops.UPDATE_RULES) gives the cache a STATE PLANE: the rule's fp32 state -- `state`,
    a pinned contiguous float32 host tensor [rows, width] resp. [rows], allocated and filled with
    initial_accumulator_value when None, exposed as cache.state -- is cached slot for slot next to the rows, in a device
    buffer a whole number of state rows away from the host tensor.  A state row moves with its table row: host -> cache
    on EVERY fill (a forward-only fill too: a later update that hits uses the cached state), cache -> host when a dirty
    row is evicted or flushed; one dirty byte covers both planes, the counters count rows.  apply_update() is the rule's
    step through the cache.  Like the table, cache.state is current only after flush() and a synchronise.  Per-element
    Adagrad triples the bytes that the fill of a 16-bit row moves over PCIe (2 * width of row, 4 * width of state):
    row-wise Adagrad, four bytes a row, is the rule to prefer behind the cache.

    stochastic_rounding=True, seed=... (float16 / bfloat16 tables; optim.SparseUpdater's arguments, checks and
    messages): apply_update() / apply_sgd() round stochastically with the bits of (seed, rounding_step, table row,
    column).  cache.rounding_step is an int64 device word that starts at 0 and is advanced on the device after every
    apply_update() / apply_sgd(), also one with no entries or count=0; fill it to resume a run.  It is None without
    stochastic rounding.  Where a row sits -- which slot, or the host table -- does not show in its bits."""

    def __init__(self, host_table, device="cuda", num_sets=1024, rule="sgd", state=None, initial_accumulator_value=0.0,
                 eps=1e-8, stochastic_rounding=False, seed=0):
        _check_table_arguments(host_table, num_sets)
        if stochastic_rounding:
            _check_rounding(host_table, seed)
        if not isinstance(rule, str) or rule not in _ops.UPDATE_RULES:
            raise ValueError("rule must be one of %r, got %r" % (sorted(_ops.UPDATE_RULES), rule))
        state_shape = {"sgd": None, "adagrad": tuple(host_table.shape), "rowwise_adagrad": (host_table.shape[0],)}[rule]
        if state is not None:
            if rule == "sgd":
                raise ValueError("rule='sgd' takes no state")
            if not isinstance(state, torch.Tensor):
                raise TypeError("state must be a torch.Tensor")
            if state.dtype != torch.float32:
                raise TypeError("state must be float32, got %s" % state.dtype)
            if tuple(state.shape) != state_shape or not state.is_contiguous():
                raise ValueError("rule=%r needs a contiguous state of shape %r, got %r" % (rule, state_shape,
                                                                                         tuple(state.shape)))
            _check_pinned("state", state)
        if host_table.is_cuda or not host_table.is_pinned():
            raise ValueError("host_table must live in PINNED host memory (tensor.pin_memory())")
        super().__init__(host_table, device=device, capacity_rows=WAYS * num_sets)
        self.rule, self.eps = rule, float(eps)
        self.state = self.state_cache = None
        self.state_row_bytes = self.state_row_offset = 0
        if state_shape is not None:
            if state is None:
                state = torch.full(state_shape, float(initial_accumulator_value), dtype=torch.float32).pin_memory()
            self.state = state
            self.state_row_bytes = 4 * (self.width if rule == "adagrad" else 1)
            self._raw_state, self.state_cache, self.state_row_offset = self._plane_behind(state, WAYS * num_sets)
        self.num_sets = num_sets
        self.capacity_rows = WAYS * num_sets
        self.row_bytes = self.width * host_table.element_size()
        self.tags = torch.full((num_sets, WAYS), -1, dtype=torch.int64, device=self.device)
        self.stamps = torch.zeros((num_sets, WAYS), dtype=torch.int32, device=self.device).view(torch.uint32)
        self.dirty = torch.zeros((num_sets, WAYS), dtype=torch.uint8, device=self.device)
        self.words = torch.tensor([1] + [0] * 15, dtype=torch.int64).to(self.device)
        self._work = None
        self.stochastic_rounding, self.seed = bool(stochastic_rounding), seed
        self.rounding_step = (torch.zeros((1,), dtype=torch.int64, device=self.device) if self.stochastic_rounding
                              else None)

    # the caller-managed policy of the base class would bypass tags / stamps / dirty
    def cache_rows(self, row_ids):
        raise RuntimeError("DynamicRowCache fills itself from the batches it sees: use prefetch() / forward()")

    cache_most_frequent = cache_rows

    def refresh(self):
        raise RuntimeError("DynamicRowCache is write-back: use flush() / invalidate()")

    def _state(self):
        p = ctypes.c_void_p
        return (p(self.table.data_ptr()), p(self.cache.data_ptr()), self.row_bytes, self.rows, self.num_sets,
                p(self.tags.data_ptr()), p(self.stamps.data_ptr()), p(self.dirty.data_ptr()),
                p(self.slot_of_row.data_ptr()), p(self.words.data_ptr()))

    def _plane_behind(self, home, slots):
        """(raw buffer, cached plane, row offset) of a state tensor `home` ([rows, width] or [rows] float32): `slots`
        of its rows on the device, like the cached table rows -- over-allocated by one row so that the plane can start
        where (plane - home) % row_bytes == 0, row_offset = (plane - home) / row_bytes."""
        row_bytes = 4 * (home.shape[1] if home.dim() == 2 else 1)
        raw = torch.empty(((slots + 1) * row_bytes,), dtype=torch.uint8, device=self.device)
        shift = (home.data_ptr() - raw.data_ptr()) % row_bytes
        plane = raw[shift:shift + slots * row_bytes].view(torch.float32)
        if home.dim() == 2:
            plane = plane.view(slots, home.shape[1])
        assert (plane.data_ptr() - home.data_ptr()) % row_bytes == 0
        return raw, plane, (plane.data_ptr() - home.data_ptr()) // row_bytes

    def _plane(self):
        p = ctypes.c_void_p
        return (p(self.state.data_ptr()), p(self.state_cache.data_ptr()), self.state_row_bytes)

    def _call_with_planes(self, name, args):
        """The entry point `name` of the cache's planes: the table's alone, or with the state plane."""
        with torch.cuda.device(self.device):
            if self.state is None:
                getattr(_lib.lib(), name)(*args)
            else:
                getattr(_lib.lib(), name + "_with_state")(*(args + self._plane()))

    def _counts(self, ids, count, last_id):
        """(num_valid, count word, word is int64, last_id word) of a prefetch, validated."""
        if count is not None and last_id is not None:
            raise ValueError("give at most one of count= and last_id=")
        n = ids.numel()
        if isinstance(count, torch.Tensor):
            if count.dtype not in _ops._INDEX or count.numel() != 1:
                raise TypeError("count must be an int or a one-element int32 / int64 tensor")
            _ops._check_dev("count", count, self.device)
            return -1, count, count.dtype == torch.int64, None
        if last_id is not None:
            if not isinstance(last_id, torch.Tensor) or last_id.dtype != ids.dtype or last_id.numel() != 1:
                raise TypeError("last_id must be a one-element tensor of the indices' dtype")
            _ops._check_dev("last_id", last_id, self.device)
            return -1, None, False, last_id
        num_valid = n if count is None else int(count)
        if not 0 <= num_valid <= n:
            raise ValueError("count must be in [0, indices.numel()]")
        return num_valid, None, False, None

    def prefetch(self, indices, for_update=False, count=None, last_id=None):
        """Make the rows that `indices` (int32 / int64 device tensor, any shape) name resident -- the contract is in the
        class docstring.  Only the first `count` entries (an int, or a one-element device tensor) or last_id + 1 entries
        (a one-element device tensor of the indices' dtype) count; default: all.  Returns None; no read-back."""
        _ops._check_dev("indices", indices, self.device)
        it = _ops._index_code("indices", indices)
        num_valid, count_word, word64, last_word = self._counts(indices, count, last_id)
        n = indices.numel()
        if n > 2 ** 31 - 1:
            raise ValueError("at most 2**31 - 1 lookups per prefetch")
        L = _lib.lib()
        need = int(L.cuembed_row_cache_workspace_bytes(n, self.rows, self.num_sets))
        if self._work is None or self._work.numel() < need:
            self._work = torch.empty((max(need, 1),), dtype=torch.uint8, device=self.device)
        lwork = ctypes.c_size_t(self._work.numel())
        args = self._state() + (_ops._ptr(indices), it, n, num_valid, _ops._ptr(count_word), int(word64),
                                _ops._ptr(last_word), int(bool(for_update)), ctypes.c_void_p(self._work.data_ptr()),
                                ctypes.byref(lwork), _ops._stream(indices))
        self._call_with_planes("cuembed_row_cache_prefetch", args)
        return None

    def forward(self, indices, offsets=None, weights=None, batch_size=None, num_hots=0, mode="sum", use_cache=True,
                out=None):
        """prefetch(indices) + translate + EmbeddingForward on the host table's base pointer: bit-identical to
        embedding_forward on a device copy of the table.  use_cache=False reads every row from the host table without
        touching the cache (dirty rows are then stale there until flush())."""
        if mode not in _ops._MODES:
            raise ValueError("mode must be 'sum', 'mean' or 'concat'")
        if use_cache:
            self.prefetch(indices)
        return super().forward(indices, offsets=offsets, weights=weights, batch_size=batch_size, num_hots=num_hots,
                               mode=mode, use_cache=use_cache, out=out)

    def apply_sgd(self, ids, rows, lr, count=None, last_id=None):
        """Sparse SGD step through the cache: table[ids[k], :] -= lr * rows[k, :] for every valid entry k of the
        compressed gradient (ids, rows) = (inverse_mapping, grad_embedding) of embedding_backward; count / last_id as
        for sparse_row_update (device-side, no read-back).  prefetch(ids, for_update=True) first, so resident rows
        are updated in HBM and marked dirty; rows their set has no way for are updated in place in the host table
        over PCIe: no update is dropped.  ids must name distinct rows (a coalesced gradient).  lr: a float or a
        one-element float32 device tensor."""
        if self.rule != "sgd":
            raise RuntimeError("this cache trains with rule=%r: use apply_update()" % self.rule)
        self._apply(ids, rows, lr, count, last_id)

    def apply_update(self, ids, rows, lr, count=None, last_id=None):
        """The cache's rule through the cache: for every valid entry k of the compressed gradient (ids, rows), row
        ids[k] of the table and its state are updated by `rule` (ops.sparse_row_update's arithmetic, eps from the
        constructor) -- arguments as for apply_sgd, which this is on a rule="sgd" cache.  prefetch(ids,
        for_update=True) first; then the ids are translated twice, once per plane, and one launch of the sparse step
        updates resident rows and their state in HBM.  Rows their set has no way for are updated in place in the host
        table AND the host state over PCIe: no update is dropped.  No read-back.

        The one rounding to the table's type is to nearest, or, on a cache with stochastic_rounding=True, stochastic
        with the bits of (seed, rounding_step, table row, column): the launch is then the named step, which carries
        the caller's ids as int64 next to the translated ones to name the bits (int64 ids are passed as they are,
        int32 ids cost one elementwise widening launch), and rounding_step is advanced on the device afterwards -- on
        every call, like SparseUpdater.apply."""
        self._apply(ids, rows, lr, count, last_id)

    def _check_step(self, ids, rows, lr):
        """The arguments of a step, validated: (lr as a float, lr as a device word or None)."""
        for name, t in (("ids", ids), ("rows", rows)):
            if not isinstance(t, torch.Tensor):
                raise TypeError("%s must be a torch.Tensor" % name)
        _ops._index_code("ids", ids)
        if rows.dtype != self.table.dtype:
            raise TypeError("rows must have the table's dtype (%s), got %s" % (self.table.dtype, rows.dtype))
        if ids.dim() != 1 or rows.dim() != 2 or rows.shape[1] != self.width or rows.shape[0] != ids.numel():
            raise ValueError("ids must be [entries] and rows [entries, width]")
        lr_word = None
        if isinstance(lr, torch.Tensor):
            if lr.dtype != torch.float32 or lr.numel() != 1:
                raise TypeError("a device-side lr must be a one-element float32 tensor")
            lr_word, lr = lr, 0.0
            _ops._check_dev("lr", lr_word, self.device)
        _ops._check_dev("rows", rows, self.device)
        return lr, lr_word

    def _apply(self, ids, rows, lr, count, last_id):
        lr, lr_word = self._check_step(ids, rows, lr)
        _ops._check_alignment("table", self.table.data_ptr(), self.table.element_size(), self.width,
                              others=(("rows", rows.data_ptr()),),
                              state=(("state", self.state.data_ptr()),) if self.rule == "adagrad" else (), max_lanes=None)
        self.prefetch(ids, for_update=True, count=count, last_id=last_id)
        n = ids.numel()
        if n == 0:
            return self._advance_rounding_step()
        translated = self.translate(ids)
        # the count of valid entries as the prefetch resolved it on the device: one int64 word
        resolved = self.words[STAT_WORDS.index("batch_count"):STAT_WORDS.index("batch_count") + 1]
        args = (ctypes.c_void_p(self.table.data_ptr()), _ops._ELEM[self.table.dtype], self.width, _ops._ptr(self.state),
                _ops.UPDATE_RULES[self.rule], _ops._ptr(translated), _ops._INDEX[torch.int64], _ops._ptr(rows), n, 1, -1,
                _ops._ptr(resolved), 1, None, float(lr), _ops._ptr(lr_word), self.eps if self.state is not None else 0.0,
                _ops._stream(ids))
        state_ids = None if self.state is None else self._translate(ids, self.state_row_offset)
        if self.stochastic_rounding:
            names = self._row_names(ids)
            with torch.cuda.device(self.device):
                _lib.lib().cuembed_sparse_row_update_placed_stochastic(
                    *(args[:-1] + (self.seed, 0, _ops._ptr(self.rounding_step), args[-1], _ops._ptr(state_ids),
                                   _ops._ptr(names))))
            return self._advance_rounding_step()
        if self.state is None:
            with torch.cuda.device(self.device):
                _lib.lib().cuembed_sparse_row_update(*args)
            return None
        with torch.cuda.device(self.device):
            _lib.lib().cuembed_sparse_row_update_placed(*(args + (_ops._ptr(state_ids),)))
        return None

    @staticmethod
    def _row_names(ids):
        """The table rows that name the rounding bits of a step's entries: the caller's ids as int64 (int64 ids as
        they are; int32 ids through one elementwise widening launch)."""
        return ids if ids.dtype == torch.int64 else ids.to(torch.int64)

    def _advance_rounding_step(self):
        """One apply = one step of the rounding bits: on the device, after the step in stream order."""
        if self.stochastic_rounding:
            self.rounding_step.add_(1)
        return None

    def flush(self):
        """Store every dirty cached row to the host table and clear the dirty bytes (stream-ordered: synchronise
        before reading the table on the host)."""
        args = self._state() + (ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream),)
        self._call_with_planes("cuembed_row_cache_flush", args)

    def invalidate(self):
        """Drop every cached row (and its cached state) WITHOUT writing dirty ones back.  The clock and the counters go
        on."""
        self.tags.fill_(-1)
        self.stamps.view(torch.int32).zero_()
        self.dirty.zero_()
        self.slot_of_row.fill_(-1)

    def stats(self):
        """The device counters as a dict (STAT_WORDS).  The only call that synchronises."""
        words = self.words.cpu().tolist()
        return dict(zip(STAT_WORDS, words))


class AdamRowCache(DynamicRowCache):
    """DynamicRowCache for a table trained with the Adam family: lazy Adam (torch.optim.SparseAdam's formula) or, with
    rowwise=True, row-wise Adam -- optim.SparseAdamUpdater's counterpart for a table in pinned host memory, as
    DynamicRowCache(rule="adagrad") is SparseUpdater's.  The result is bit for bit the table and the moments that
    SparseAdamUpdater produces on device copies -- with round to nearest, or, with stochastic_rounding=True and the same
    seed, with stochastic rounding: cache.rounding_step is DynamicRowCache's.

    The moments live in pinned host memory like the table -- cache.exp_avg float32 [rows, width], cache.exp_avg_sq
    float32 [rows, width], or [rows] with rowwise=True: the shapes SparseAdamUpdater owns; zero-filled and pinned when not
    given -- and are cached slot for slot next to the rows as TWO STATE PLANES (cache.exp_avg_cache,
    cache.exp_avg_sq_cache), each a whole number of its own rows away from its host tensor.  Both moment rows move with
    their table row: host -> cache on EVERY fill (a forward-only fill too), cache -> host when a dirty row is evicted
    or flushed; one dirty byte covers all three planes, the counters count rows, and placement is DynamicRowCache's.
    Like the table, the moments are current on the host only after flush() and a synchronise; invalidate() drops the
    cached ones without write-back.

    The bias-factor clock is SparseAdamUpdater's and lives on the device: cache.powers float64 [3] = (t, beta1^t,
    beta2^t), starting at (0, 1, 1), and cache.bias_factor float32 [1].  apply_update() advances it on every call.

    What a fill costs over PCIe, for a 16-bit row of width W: 2 * W + 8 * W bytes with lazy Adam (the row and two
    moment rows: five times the row), 2 * W + 4 * W + 4 bytes with row-wise Adam (the row, exp_avg's row and one word).
    Row-wise Adam is the rule to prefer behind the cache for that reason."""

    def __init__(self, host_table, device="cuda", num_sets=1024, rowwise=False, betas=(0.9, 0.999), eps=1e-8,
                 weight_decay=0.0, bias_correction=True, exp_avg=None, exp_avg_sq=None, stochastic_rounding=False, seed=0):
        _check_table_arguments(host_table, num_sets)
        if stochastic_rounding:
            _check_rounding(host_table, seed)
        betas = _ops._check_betas(betas)
        if not float(eps) >= 0.0 or not float(weight_decay) >= 0.0:
            raise ValueError("eps and weight_decay must not be negative")
        rowwise = bool(rowwise)
        rows, width = host_table.shape
        shapes = dict(exp_avg=(rows, width), exp_avg_sq=(rows,) if rowwise else (rows, width))
        for name, t in (("exp_avg", exp_avg), ("exp_avg_sq", exp_avg_sq)):
            if t is None:
                continue
            if not isinstance(t, torch.Tensor):
                raise TypeError("%s must be a torch.Tensor" % name)
            if t.dtype != torch.float32:
                raise TypeError("%s must be float32, got %s" % (name, t.dtype))
            if tuple(t.shape) != shapes[name] or not t.is_contiguous():
                raise ValueError("rowwise=%r needs a contiguous %s of shape %r, got %r" % (rowwise, name, shapes[name],
                                                                                         tuple(t.shape)))
            _check_pinned(name, t)
        super().__init__(host_table, device=device, num_sets=num_sets, eps=eps, stochastic_rounding=stochastic_rounding,
                         seed=seed)
        self.rule = "rowwise_adam" if rowwise else "adam"        # (apply_sgd points to apply_update)
        self.rowwise, self.betas, self.weight_decay = rowwise, betas, float(weight_decay)
        self.bias_correction = bool(bias_correction)
        self.exp_avg = torch.zeros(shapes["exp_avg"], dtype=torch.float32).pin_memory() if exp_avg is None else exp_avg
        self.exp_avg_sq = (torch.zeros(shapes["exp_avg_sq"], dtype=torch.float32).pin_memory() if exp_avg_sq is None
                           else exp_avg_sq)
        slots = WAYS * num_sets
        self._raw_exp_avg, self.exp_avg_cache, self.exp_avg_row_offset = self._plane_behind(self.exp_avg, slots)
        self._raw_exp_avg_sq, self.exp_avg_sq_cache, self.exp_avg_sq_row_offset = self._plane_behind(self.exp_avg_sq, slots)
        self.powers, self.bias_factor = _ops.new_adam_clock(self.device)
        self._one = None if self.bias_correction else torch.ones((1,), dtype=torch.float32, device=self.device)
        self._placed = None

    def _call_with_planes(self, name, args):
        p = ctypes.c_void_p
        planes = (p(self.exp_avg.data_ptr()), p(self.exp_avg_cache.data_ptr()), 4 * self.width,
                  p(self.exp_avg_sq.data_ptr()), p(self.exp_avg_sq_cache.data_ptr()), 4 if self.rowwise else 4 * self.width)
        with torch.cuda.device(self.device):
            getattr(_lib.lib(), name + "_with_states")(*(args + planes))

    def apply_update(self, ids, rows, lr, count=None, last_id=None):
        """One Adam step through the cache, call for call SparseAdamUpdater.apply: for every valid entry k of the
        compressed gradient (ids, rows) -- arguments as for DynamicRowCache.apply_sgd -- row ids[k] of the table and
        its two moments are updated by ops.sparse_row_adam's arithmetic.  In order: the clock advances on the device
        (on EVERY call, also one with no entries or count=0); prefetch(ids, for_update=True); ONE launch translates
        the ids for the three planes; ONE launch of the sparse Adam step with placed moments updates resident rows and
        their moments in HBM, with the count the prefetch resolved.  Rows their set has no way for are updated in
        place in the host table AND both host moments over PCIe: no update is dropped.  lr: a float or a one-element
        float32 device tensor.  bias_correction=False feeds a constant 1 (the clock still counts).  No read-back.

        The rounding is to nearest, or, on a cache with stochastic_rounding=True, stochastic with the bits of (seed,
        rounding_step, table row, column): the launch is then the named placed step, which carries the caller's ids
        as int64 next to the three translated arrays (int64 ids as they are, int32 ids through one elementwise
        widening launch), and rounding_step is advanced on the device afterwards -- on every call, like
        SparseAdamUpdater.apply."""
        lr, lr_word = self._check_step(ids, rows, lr)
        state = (("exp_avg", self.exp_avg.data_ptr()),)
        if not self.rowwise:
            state += (("exp_avg_sq", self.exp_avg_sq.data_ptr()),)
        _ops._check_alignment("table", self.table.data_ptr(), self.table.element_size(), self.width,
                              others=(("rows", rows.data_ptr()),), state=state, max_lanes=None)
        _ops.adam_clock_advance(self.powers, self.bias_factor, self.betas)
        self.prefetch(ids, for_update=True, count=count, last_id=last_id)
        n = ids.numel()
        if n == 0:
            return self._advance_rounding_step()
        if self._placed is None or self._placed.shape[1] < n:
            self._placed = torch.empty((3, n), dtype=torch.int64, device=self.device)
        placed = [self._placed[k, :n] for k in range(3)]
        # the count of valid entries as the prefetch resolved it on the device: one int64 word
        resolved = self.words[STAT_WORDS.index("batch_count"):STAT_WORDS.index("batch_count") + 1]
        beta1, beta2 = self.betas
        bias = self.bias_factor if self.bias_correction else self._one
        L = _lib.lib()
        with torch.cuda.device(self.device):
            L.cuembed_translate_indices_for_row_cache_planes(
                _ops._ptr(ids), _ops._INDEX[ids.dtype], n, _ops._ptr(self.slot_of_row), self.rows,
                self.cache_row_offset, _ops._ptr(placed[0]), self.exp_avg_row_offset, _ops._ptr(placed[1]),
                self.exp_avg_sq_row_offset, _ops._ptr(placed[2]), _ops._stream(ids))
            step = (ctypes.c_void_p(self.table.data_ptr()), _ops._ELEM[self.table.dtype], self.width,
                    ctypes.c_void_p(self.exp_avg.data_ptr()), ctypes.c_void_p(self.exp_avg_sq.data_ptr()),
                    _ops.ADAM_RULES[self.rule], _ops._ptr(placed[0]), _ops._INDEX[torch.int64], _ops._ptr(rows), n, 1, -1,
                    _ops._ptr(resolved), 1, None, float(lr), _ops._ptr(lr_word), 1.0, _ops._ptr(bias), beta1,
                    1.0 - beta1, beta2, 1.0 - beta2, self.eps, self.weight_decay)
            if self.stochastic_rounding:
                names = self._row_names(ids)
                L.cuembed_sparse_row_adam_placed_stochastic(
                    *(step + (self.seed, 0, _ops._ptr(self.rounding_step), _ops._stream(ids), _ops._ptr(placed[1]),
                              _ops._ptr(placed[2]), _ops._ptr(names))))
            else:
                L.cuembed_sparse_row_adam_placed(*(step + (_ops._stream(ids), _ops._ptr(placed[1]), _ops._ptr(placed[2]))))
        return self._advance_rounding_step()
