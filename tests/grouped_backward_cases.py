"""Helpers of the grouped-backward GPU tests: device copies of the grouped_cases layouts, exactly representable
gradients, and the single-table pipeline (row ids -> transpose -> remap -> embedding_backward) that a grouped result is
compared with, table by table."""
import numpy as np
import torch

import grouped_cases as C

DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def exact_weights(rng, nnz):
    """Per-lookup weights in {0.5, 0.25} (fp32)."""
    return rng.choice(np.array([0.5, 0.25], dtype=np.float32), size=nnz)


def exact_grad_y(rng, batch, num_tables, width, kind):
    """Integer grad_y in [-4, 4] (fp32 values).  Results then have the same bits however a row's lookups are cut into
    partial sums, AS LONG AS every partial sum is representable in the gradient's type: integers below 2^11 (fp16) or
    2^8 (bf16), multiples of 0.25 below 2^9 (fp16) or 2^6 (bf16).  The 17-row table at B = 1,023 sums ~1,500 lookups per
    row -- a random walk of sigma ~100 for uniform integers, fine for fp16 and fp32 and too much for bf16's 8 bits -- so
    for bf16 one value in 16 is non-zero (sigma ~25, ~10 weighted); representable() checks the final sums."""
    values = rng.integers(-4, 5, (batch, num_tables, width)).astype(np.float32)
    if kind == "bf16":
        values *= rng.integers(0, 16, values.shape) == 0
    return values


def representable(kind, weighted, exact):
    """True if the fp64 sums `exact` (and so, with overwhelming likelihood, the prefixes of the same walks) are exactly
    representable in the gradient's type."""
    limit = {"f32": 2.0 ** 22, "f16": 2.0 ** 9 if weighted else 2.0 ** 11, "bf16": 2.0 ** 6 if weighted else 2.0 ** 8}[kind]
    return float(np.abs(exact).max(initial=0.0)) < limit


def global_problem(rows, batch, ids, offsets, hot):
    """(keys, sample_ids) of a grouped call by numpy (int64)."""
    T = len(rows)
    base = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
    lengths = np.full(T * batch, hot, dtype=np.int64) if offsets is None else np.diff(offsets)
    bag = np.repeat(np.arange(T * batch, dtype=np.int64), lengths)
    t, b = bag // batch, bag % batch
    return base[t] + ids, b * T + t


def fp64_sums(keys, sample_ids, grad_2d, weights, total_rows):
    """(exact, scale, walk, run_len) per global row: the fp64 sum of the terms grad_y[sample] * weight, the sum of
    their magnitudes, the root of the sum of their squares, and the number of lookups."""
    terms = grad_2d[sample_ids] * (1.0 if weights is None else weights[:, None])
    width = grad_2d.shape[1]
    exact, scale, walk = (np.zeros((total_rows, width)) for _ in range(3))
    np.add.at(exact, keys, terms)
    np.add.at(scale, keys, np.abs(terms))
    np.add.at(walk, keys, terms * terms)
    return exact, scale, np.sqrt(walk), np.bincount(keys, minlength=total_rows)


def single_table(ce, rows_t, grad_t, ids, offsets, hot, weights, compressed, reference_sums=False):
    """The single-table pipeline on table t's own bags (device tensors; offsets start at 0): the dense [rows_t, W]
    gradient, or (inverse_mapping, rows) of the compressed one."""
    width = grad_t.shape[1]
    nnz = ids.numel()
    if nnz == 0:
        if not compressed:
            return torch.zeros((rows_t, width), dtype=grad_t.dtype, device="cuda")
        return torch.zeros(0, dtype=ids.dtype, device="cuda"), torch.zeros((0, width), dtype=grad_t.dtype, device="cuda")
    if offsets is None:
        sample_ids = ce.extract_row_ids_from_fixed(grad_t.shape[0], hot, dtype=ids.dtype)
    else:
        sample_ids = ce.extract_row_ids_from_csr(offsets, nnz=nnz, dtype=ids.dtype)
    t_idx, t_sid, t_w = ce.transpose(sample_ids, ids, weights, num_categories=rows_t)
    if not compressed:
        grad, _ = ce.embedding_backward(grad_t, rows_t, t_idx, t_sid, None, t_w, reference_sums=reference_sums)
        return grad
    remap = ce.compute_compressed_grad_indices(t_idx)
    num_unique = int(remap[-1].item()) + 1
    rows, inv = ce.embedding_backward(grad_t, num_unique, t_idx, t_sid, remap, t_w)
    return inv, rows


def table_problem(t, batch, ids, offsets, hot, weights_d=None, index_dtype=np.int32):
    """grouped_cases.table_slice on the device: (ids, offsets or None, weights or None) of table t; `weights_d` is the
    device tensor of all lookups' weights, of which table t's slice is returned."""
    position = np.arange(ids.size, dtype=np.float32)          # (table_slice cuts it like the weights)
    i, o, p = C.table_slice(t, batch, ids, offsets, hot, position)
    lo = int(p[0]) if p.size else 0
    w = None if weights_d is None else weights_d[lo:lo + i.size].contiguous()
    return dev(i.astype(index_dtype)), None if o is None else dev(o.astype(index_dtype)), w
