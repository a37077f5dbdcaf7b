"""Where a non-finite row of a fused 8-bit table reaches, in embedding_forward_quantized,
embedding_forward_quantized_grouped and embedding_forward_quantized_mixed_group, with no arithmetic model: the rows of
forward_edge_cases.poisoned_rows hold a +Inf or -Inf bias or a NaN scale in the fused bytes, so they dequantize to Inf or
NaN in every column and nothing later makes that finite.  From ids and offsets alone:

    (a) an output element is non-finite if and only if its bag looks up a poisoned row -- with weight 0.0 or -0.0 as well;
    (b) the rows of `out` that belong to clean bags equal, bit for bit, the same call on the tables whose poisoned rows
        hold their original finite bytes;
    (c) the grouped and the mixed result equal torch.cat of the single-table calls: a NaN by class, the rest by bits.

A lookup too many -- the neighbouring bag's, the next table's, a lane past `hot` that feeds in index 0 (row 0 is
poisoned) with weight 0 -- turns a clean bag non-finite and fails (a) and (b).  Clean bags stand between poisoned ones
inside a table, across every table boundary and across a workgroup boundary.  Groups A, B and C of
test_gpu_quantized_mixed_group.py and three-table groups of widths 8, 36 and 64; B in {5, 300}; fixed hotness 9 and CSR;
fp32 and fp16 output; sum and mean, weighted and not; both index types.  test_forward_edges_host.py asserts without a GPU
that at least half of the bags of every case are clean.

Not here: an fp32 bit model of the quantized walk (no value of a clean bag is predicted, only that the poison does not
change it), the group optimizer steps on IEEE edges, the exchange kernels, far rows of the quantized mixed forward.
"""
import numpy as np
import pytest
import torch

import forward_edge_cases as F

pytestmark = pytest.mark.gpu

ident = lambda v: "w" + "_".join(map(str, v)) if isinstance(v, tuple) else str(v)


@pytest.fixture(scope="module")
def ce():
    import cuembed_amd
    assert torch.cuda.is_available()
    return cuembed_amd


def ibits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def same_but_nan_by_class(got, want):
    nan = torch.isnan(want)
    return bool(torch.equal(torch.isnan(got), nan)) and bool(torch.equal(ibits(got)[~nan], ibits(want)[~nan]))


def check_reach(got, calm, bad_rows, label):
    """(a) and (b) on one [B, W] result: bad_rows [B] bool, calm the result on the unpoisoned tables."""
    finite = torch.isfinite(got)
    assert bool(finite[~bad_rows].all()), label + ("a clean bag is not finite",)
    assert not bool(finite[bad_rows].any()), label + ("an element of a poisoned bag is finite",)
    assert torch.equal(ibits(got)[~bad_rows], ibits(calm)[~bad_rows]), label + ("a clean bag changed with the poison",)
    return int((~bad_rows).sum()) * got.shape[1], int(bad_rows.sum()) * got.shape[1]


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("batch", F.Q_BATCHES, ids=lambda b: "b%d" % b)
@pytest.mark.parametrize("family,widths", F.Q_CASES, ids=ident)
def test_a_poisoned_row_reaches_its_own_bags_only(ce, family, widths, batch, out_dtype):
    T, D = len(widths), sum(widths)
    tabs = F.quantized_tables(widths)
    calm_tables = [torch.from_numpy(np.array(c)).cuda() for c, _, _ in tabs]
    bad_tables = [torch.from_numpy(np.array(b)).cuda() for _, b, _ in tabs]
    if family == "same":
        make, call = ce.TableGroup, ce.embedding_forward_quantized_grouped
    else:
        make, call = ce.QuantizedMixedTableGroup, ce.embedding_forward_quantized_mixed_group
    calm_group, bad_group = make(calm_tables), make(bad_tables)
    cols = np.concatenate([[0], np.cumsum(widths)])
    by_bits = by_class = calls = 0
    for layout, (it, ot) in zip(F.Q_LAYOUTS, ((torch.int32, torch.int32), (torch.int64, torch.int64))):
        p = F.quantized_case(family, widths, batch, layout)
        hot = p["hot"]
        bad_rows = torch.from_numpy(np.array(p["poisoned"])).cuda()                     # [T, B]
        d_ids = torch.from_numpy(np.array(p["ids"])).to(it).cuda()
        d_off = None if hot else torch.from_numpy(np.array(p["offsets"])).to(ot).cuda()
        w_all = torch.from_numpy(np.array(p["weights"])).to(out_dtype).cuda()
        for mode, weighted in F.MODES:
            kw = dict(num_hots=hot, mode=mode, out_dtype=out_dtype)
            w = w_all if weighted else None
            singles = []
            for t in range(T):                # ---- embedding_forward_quantized, table by table
                i, o, _ = F.GC.table_slice(t, batch, p["ids"], p["offsets"], hot, p["ids"])
                lo = t * batch * hot if hot else int(p["offsets"][t * batch])
                args = (torch.from_numpy(np.array(i)).to(it).cuda(), None if hot else torch.from_numpy(np.array(o)).to(ot).cuda(),
                        None if w is None else w[lo:lo + i.size].contiguous())
                got = ce.embedding_forward_quantized(bad_tables[t], *args, batch_size=batch, **kw)
                calm = ce.embedding_forward_quantized(calm_tables[t], *args, batch_size=batch, **kw)
                assert got.shape == (batch, widths[t]) and got.dtype == out_dtype
                a, b = check_reach(got, calm, bad_rows[t], (layout, mode, weighted, "single", t))
                by_bits, by_class, calls = by_bits + a, by_class + b, calls + 1
                singles.append(got)
            cat = torch.cat(singles, dim=1)
            for row_loads in (None, "streaming"):        # ---- the group call
                label = (layout, mode, weighted, row_loads, call.__name__)
                got = call(bad_group, d_ids, d_off, w, batch_size=batch, row_loads=row_loads, **kw).reshape(batch, D)
                calm = call(calm_group, d_ids, d_off, w, batch_size=batch, row_loads=row_loads, **kw).reshape(batch, D)
                for t in range(T):
                    a, b = check_reach(got[:, cols[t]:cols[t + 1]], calm[:, cols[t]:cols[t + 1]], bad_rows[t], label + (t,))
                    by_bits, by_class = by_bits + a, by_class + b
                assert same_but_nan_by_class(got, cat), label + ("vs torch.cat of the single-table calls",)
                calls += 1
    print("%s + embedding_forward_quantized %s B=%d %s: %d calls, %d elements by bits, %d by class"
          % (call.__name__, widths, batch, out_dtype, calls, by_bits, by_class))
    assert by_class > 0 and by_bits >= by_class
