"""The two kernels of the grouped backward against numpy, exactly: keys + sample ids (cuembed::GroupedBackwardKeys) for
every layout of grouped_cases -- empty bags on both sides of every table boundary, an all-empty table, boundaries inside
a wavefront and a workgroup -- every batch, index / offset / key type, T = 1 and 3; and the table cuts of a compressed
gradient (cuembed::GroupedTableCuts) against np.searchsorted for every count source."""
import numpy as np
import pytest
import torch

import grouped_cases as C

pytestmark = pytest.mark.gpu

INTS = {"i32": (np.int32, torch.int32), "i64": (np.int64, torch.int64)}


@pytest.fixture(scope="module")
def ce():
    import cuembed_amd
    assert torch.cuda.is_available()
    return cuembed_amd


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def group_of(ce, rows):
    return ce.TableGroup([torch.zeros((r, 2), dtype=torch.float32, device="cuda") for r in rows])


def expected(rows, batch, ids, offsets, hot):
    """(keys, sample_ids) in int64 by numpy: bag g = t * batch + b of every lookup from the offsets."""
    T = len(rows)
    base = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
    lengths = np.full(T * batch, hot, dtype=np.int64) if offsets is None else np.diff(offsets)
    bag = np.repeat(np.arange(T * batch, dtype=np.int64), lengths)
    t, b = bag // batch, bag % batch
    return base[t] + ids, b * T + t


@pytest.mark.parametrize("batch", C.BATCHES)
@pytest.mark.parametrize("num_tables", [1, 3])
def test_keys_and_sample_ids_equal_numpy(ce, batch, num_tables):
    rows = C.ROWS[:num_tables]
    group = group_of(ce, rows)
    for name, ids, offsets, hot, _ in C.layouts(batch, rows=rows):
        want_keys, want_sids = expected(rows, batch, ids, offsets, hot)
        for i_name, (i_np, _) in INTS.items():
            for o_name, (o_np, _) in INTS.items():
                if offsets is None and o_name == "i64":
                    continue                                     # fixed hotness has no offsets
                for k_name, (k_np, k_t) in INTS.items():
                    keys, sids = ce.grouped_backward_keys(group, dev(ids.astype(i_np)),
                                                          None if offsets is None else dev(offsets.astype(o_np)),
                                                          num_hots=hot, key_dtype=k_t)
                    tag = (name, i_name, o_name, k_name)
                    assert keys.dtype == k_t and sids.dtype == k_t and keys.numel() == ids.size, tag
                    assert np.array_equal(keys.cpu().numpy(), want_keys.astype(k_np)), tag
                    assert np.array_equal(sids.cpu().numpy(), want_sids.astype(k_np)), tag


def test_default_key_type_out_buffers_and_unaligned_views(ce):
    """int32 keys by default whatever the indices' type; out= buffers are written in place; buffers that are not
    aligned to four entries take the scalar path and give the same values."""
    batch = 5
    group = group_of(ce, C.ROWS)
    for name, ids, offsets, hot, _ in C.layouts(batch):
        want_keys, want_sids = expected(C.ROWS, batch, ids, offsets, hot)
        off = None if offsets is None else dev(offsets)
        keys, sids = ce.grouped_backward_keys(group, dev(ids), off, num_hots=hot)
        assert keys.dtype == torch.int32 and sids.dtype == torch.int32
        assert np.array_equal(keys.cpu().numpy(), want_keys) and np.array_equal(sids.cpu().numpy(), want_sids), name
        n = ids.size
        pool = torch.full((2 * n + 8,), -7, dtype=torch.int32, device="cuda")
        out = (pool[1:1 + n], pool[n + 3:2 * n + 3])              # 4 and 12 bytes past a 16-byte boundary
        shifted = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), dev(ids)])[1:]
        got = ce.grouped_backward_keys(group, shifted, off, num_hots=hot, out=out)
        assert got[0] is out[0] and got[1] is out[1]
        assert np.array_equal(out[0].cpu().numpy(), want_keys) and np.array_equal(out[1].cpu().numpy(), want_sids), name
        assert pool[0] == -7 and bool((pool[1 + n:n + 3] == -7).all()) and bool((pool[2 * n + 3:] == -7).all()), name


def test_keys_of_an_empty_batch(ce):
    group = group_of(ce, C.ROWS)
    off = torch.zeros(3 * 5 + 1, dtype=torch.int64, device="cuda")
    keys, sids = ce.grouped_backward_keys(group, torch.zeros(0, dtype=torch.int64, device="cuda"), off)
    assert keys.numel() == 0 and sids.numel() == 0


def test_the_torch_op_agrees_with_the_function(ce):
    from cuembed_amd import cuembed_pyt  # noqa: F401  (loads the ops)
    batch = 5
    group = group_of(ce, C.ROWS)
    for name, ids, offsets, hot, _ in C.layouts(batch):
        idx = dev(ids) if offsets is not None else dev(ids).view(3, batch, hot)
        for narrow in (True, False):
            want = ce.grouped_backward_keys(group, dev(ids), dev(offsets), num_hots=hot,
                                            key_dtype=torch.int32 if narrow else torch.int64)
            got = torch.ops.cuembed_pyt.cuembed_grouped_backward_keys(idx, dev(offsets), group.row_base_device, 3, batch,
                                                                      hot, narrow)
            assert got[0].dtype == want[0].dtype and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), name


CUT_ROWS = (5000, 17, 300)


def gradient_ids(rng, skip_table=None, pad=9):
    """Ascending global ids of a compressed gradient (some rows of every table but `skip_table`) + `pad` entries of room
    past the count that name rows of the batch again, as a padded gradient does."""
    base = np.concatenate([[0], np.cumsum(CUT_ROWS)])
    parts = [base[t] + np.sort(rng.choice(CUT_ROWS[t], size=min(CUT_ROWS[t], 11), replace=False))
             for t in range(len(CUT_ROWS)) if t != skip_table]
    valid = np.concatenate(parts).astype(np.int64)
    return base.astype(np.int64), valid, np.concatenate([valid, valid[:pad]])


@pytest.mark.parametrize("id_type", ["i32", "i64"])
def test_table_cuts_equal_searchsorted(ce, id_type):
    from cuembed_amd import cuembed_pyt  # noqa: F401
    np_t, torch_t = INTS[id_type]
    rng = np.random.default_rng(5)
    for skip in (None, 1, 0, 2):                                   # table 1 (or the first, or the last) has no entry
        base, valid, stored = gradient_ids(rng, skip)
        ids = dev(stored.astype(np_t))
        base_d = dev(base)
        count = valid.size
        want = np.searchsorted(valid, base, side="left")
        assert want[0] == 0 and want[-1] == count
        if skip is not None:
            assert want[skip] == want[skip + 1]
        sources = [dict(count=count),
                   dict(count=torch.tensor([count], dtype=torch.int32, device="cuda")),
                   dict(count=torch.tensor([count], dtype=torch.int64, device="cuda")),
                   dict(last_id=torch.tensor([count - 1], dtype=torch_t, device="cuda"))]
        for kw in sources:
            cuts = ce.grouped_table_cuts(ids, base_d, **kw)
            assert cuts.dtype == torch.int64 and np.array_equal(cuts.cpu().numpy(), want), (skip, kw)
        # all entries (no count): the padding belongs to the searched range, which is then not ascending -- only an
        # unpadded array is a valid input
        assert np.array_equal(ce.grouped_table_cuts(dev(valid.astype(np_t)), base_d).cpu().numpy(), want)
        # a count of zero, below zero, above the capacity: all-zero cuts
        for kw in (dict(count=0), dict(count=torch.tensor([0], dtype=torch.int32, device="cuda")),
                   dict(last_id=torch.tensor([-1], dtype=torch_t, device="cuda")),
                   dict(count=torch.tensor([-3], dtype=torch.int64, device="cuda")),
                   dict(count=torch.tensor([stored.size + 1], dtype=torch.int32, device="cuda")),
                   dict(last_id=torch.tensor([stored.size], dtype=torch_t, device="cuda"))):
            assert not ce.grouped_table_cuts(ids, base_d, **kw).any(), kw
        # the torch op: a count word, and a last id
        word = torch.tensor([count], dtype=torch.int32, device="cuda")
        assert np.array_equal(torch.ops.cuembed_pyt.cuembed_grouped_table_cuts(ids, word, base_d).cpu().numpy(), want)
        last = torch.tensor([count - 1], dtype=torch_t, device="cuda")
        assert np.array_equal(torch.ops.cuembed_pyt.cuembed_grouped_table_cuts(ids, last, base_d, True).cpu().numpy(), want)


def test_table_cuts_of_more_tables_than_threads(ce):
    """300 tables of 3 rows: the one workgroup's threads take more than one table each."""
    rng = np.random.default_rng(6)
    base = np.arange(301, dtype=np.int64) * 3
    valid = np.sort(rng.choice(900, size=400, replace=False)).astype(np.int64)
    cuts = ce.grouped_table_cuts(dev(valid), dev(base))
    assert np.array_equal(cuts.cpu().numpy(), np.searchsorted(valid, base, side="left"))
