"""Shapes and bags of the grouped-forward tests (numpy, no GPU): a group of three tables of 5,000, 17 and 300 rows --
table 0 the largest, each filled from its own seed, the ids of table t drawn in [0, rows_t) -- and the bag layouts at
which a grouped kernel can go wrong: the table choice, the output row, and table boundaries that fall inside a
wavefront and inside a workgroup (B = 1, 5, 1,023: no multiple of the samples of either).

Bag g = t * B + b belongs to table t and sample b; the result is [B, T, W].
"""
import numpy as np

ROWS = (5000, 17, 300)
BATCHES = (1, 5, 1023)
BAG_LENGTHS = (0, 1, 7, 8, 9, 33, 64)
FIXED_HOTS = (1, 7, 26)             # 26: staged in LDS, as are 1 and 7
MODES = [("sum", False), ("sum", True), ("mean", False), ("mean", True)]   # (mode, weighted)


def table_values(t, rows, width):
    """fp32 values of table t (its own seed), U(-1, 1): arbitrary bits, so that a sum depends on its order."""
    rng = np.random.default_rng(1000 + t)
    return rng.uniform(-1.0, 1.0, (rows, width)).astype(np.float32)


def draw_ids(rng, rows, lengths):
    """One id array for bags of `lengths`, table by table ([T][B] lengths), ids of table t in [0, rows[t])."""
    parts = [rng.integers(0, rows[t], int(np.sum(lengths[t]))) for t in range(len(lengths))]
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)


def csr_lengths(rng, num_tables, batch, variant):
    """[T, B] bag lengths drawn from BAG_LENGTHS.
    "ragged":       empty bags on both sides of each table boundary (the last bag of table t and the first of table
                    t + 1), where a table has at least three bags;
    "empty_table":  all bags of table 1 are empty."""
    lengths = rng.choice(BAG_LENGTHS, size=(num_tables, batch))
    if variant == "ragged":
        if batch >= 3:
            lengths[:, 0] = 0
            lengths[:, -1] = 0
            lengths[:, 1] = 64          # ... next to full ones
    elif variant == "empty_table":
        if num_tables > 1:
            lengths[1, :] = 0
    else:
        raise ValueError(variant)
    return lengths


def weights_for(rng, nnz):
    """Per-lookup weights, U(0.1, 1) in fp32 (rounded to the tables' type by the caller)."""
    return rng.uniform(0.1, 1.0, nnz).astype(np.float32)


def layouts(batch, rows=ROWS, seed=0):
    """[(name, ids int64 [nnz], offsets int64 [T * B + 1] or None, num_hots, weights fp32 [nnz])] for a batch size."""
    num_tables = len(rows)
    out = []
    for k, hot in enumerate(FIXED_HOTS):
        rng = np.random.default_rng(seed * 100 + k)
        lengths = np.full((num_tables, batch), hot)
        ids = draw_ids(rng, rows, lengths)
        out.append(("h%d" % hot, ids, None, hot, weights_for(rng, ids.size)))
    for k, variant in enumerate(("ragged", "empty_table")):
        rng = np.random.default_rng(seed * 100 + 50 + k)
        lengths = csr_lengths(rng, num_tables, batch, variant)
        ids = draw_ids(rng, rows, lengths)
        offsets = np.concatenate([[0], np.cumsum(lengths.reshape(-1))]).astype(np.int64)
        out.append(("csr_" + variant, ids, offsets, 0, weights_for(rng, ids.size)))
    return out


def table_slice(t, batch, ids, offsets, num_hots, weights):
    """The single-table problem of table t: (ids, offsets or None, weights)."""
    if offsets is None:
        lo, hi = t * batch * num_hots, (t + 1) * batch * num_hots
        return ids[lo:hi], None, weights[lo:hi]
    off = offsets[t * batch:(t + 1) * batch + 1]
    lo, hi = int(off[0]), int(off[-1])
    return ids[lo:hi], off - off[0], weights[lo:hi]
