"""IEEE edge values through the plain GROUP forwards -- embedding_forward_grouped and embedding_forward_mixed_group -- bit
for bit against the CPU oracle (oracle.embedding_forward once per table, concatenated: fp32 accumulation in lookup order,
one rounding) and against torch.cat of T single-table embedding_forward calls, on the tables and bags of
forward_edge_cases.py: +-0, +-Inf, NaN, subnormals, values near the maximum and exact ties in half of every table's rows,
weights of 0.0 and -0.0 on +Inf rows, clean bags between bags that begin and end with a +Inf row -- inside a table, across
a table boundary and across a workgroup boundary -- means whose weights sum to exactly 0, empty bags beside non-finite
ones.  On such data a lookup, lane or column too many is 0 * Inf = NaN in a bag whose result is finite in the oracle.

Comparison rule (backward_edge_model.compare): where the oracle has a NaN the device has a NaN, payload and sign free;
everywhere else the bits are identical.  Every call writes into an `out` pre-filled with a NaN pattern: every element is
written, and an empty bag reads as +0 bits.  test_forward_edges_host.py asserts, without a GPU, that at most a quarter
of the oracle's elements are NaN and at least half of the bags are clean in every case.

Every case runs fixed hotness 1 / 7 / 26 and two CSR layouts, sum and mean, weighted and not, both index types (CSR: all
four index / offset pairs), row_loads default and "streaming".

Not here: the quantized forwards (test_gpu_quantized_forward_edges.py), an fp32 bit model of the quantized walk, the group
optimizer steps on IEEE edges, the exchange kernels, far rows of the quantized mixed forward.
"""
import numpy as np
import pytest
import torch

import backward_edge_model as M
import forward_edge_cases as F
from test_forward_edges_host import DTYPE, GROUPS, case_problem, ident

pytestmark = pytest.mark.gpu

INT = {"i32": (np.int32, torch.int32), "i64": (np.int64, torch.int64)}
NAN_FILL = {"f32": 0x7fc00abc, "f16": 0x7e5a, "bf16": 0x7fda}


@pytest.fixture(scope="module")
def ce():
    import cuembed_amd
    assert torch.cuda.is_available()
    return cuembed_amd


def on_device(bits, kind):
    a = np.array(bits, order="C")          # (a copy: the cached problems are read-only)
    return torch.from_numpy(a.view(np.int16 if a.dtype.itemsize == 2 else np.int32)).cuda().view(DTYPE[kind])


def device_bits(t):
    t = t.detach().contiguous()
    wide = t.element_size() == 4
    return t.view(torch.int32 if wide else torch.int16).cpu().numpy().view(np.uint32 if wide else np.uint16)


def prefilled(kind, shape):
    return on_device(np.full(shape, NAN_FILL[kind], dtype=M.BITS[kind]), kind)


def single_table_cat(ce, dev_tables, p, d_weights, mode):
    """[B, D] bit patterns: torch.cat of T calls of ce.embedding_forward."""
    batch, hot = p["batch"], p["hot"]
    per_table = []
    for t, table in enumerate(dev_tables):
        i, o, _ = F.GC.table_slice(t, batch, p["ids"], p["offsets"], hot, p["ids"])
        lo = t * batch * hot if p["offsets"] is None else int(p["offsets"][t * batch])
        w = None if d_weights is None else d_weights[lo:lo + i.size].contiguous()
        per_table.append(ce.embedding_forward(table, torch.from_numpy(np.array(i)).cuda(),
                                              None if o is None else torch.from_numpy(np.array(o)).cuda(), w,
                                              batch_size=batch, num_hots=hot, mode=mode))
    return device_bits(torch.cat(per_table, dim=1))


@pytest.mark.parametrize("batch", F.BATCHES, ids=lambda b: "b%d" % b)
@pytest.mark.parametrize("family,widths", GROUPS, ids=ident)
@pytest.mark.parametrize("kind", F.KINDS)
def test_group_forward_on_edge_values_has_the_oracles_bits(ce, oracle, kind, family, widths, batch):
    by_bits = by_class = calls = 0
    for layout in F.LAYOUTS:
        p = case_problem(ce, family, kind, widths, batch, layout)
        group_widths = p["widths"]
        T, D, hot = len(group_widths), sum(group_widths), p["hot"]
        dev_tables = [on_device(bits, kind) for _, bits in F.tables(kind, group_widths)]
        if family == "same":
            group, call = ce.TableGroup(dev_tables), ce.embedding_forward_grouped
        else:
            group, call = ce.MixedTableGroup(dev_tables), ce.embedding_forward_mixed_group
            if widths is None:       # the column loop: one lane more than a workgroup has
                assert group_widths[0] * DTYPE[kind].itemsize // group.lane_bytes() == 257
        want = F.expected(oracle, p)
        w_dev = on_device(M.to_bits(kind, p["weights"]), kind)
        types = [(i, o) for i in INT for o in INT] if hot == 0 else [(i, "i32") for i in INT]
        for mode, weighted in F.MODES:
            w = w_dev if weighted else None
            cat = single_table_cat(ce, dev_tables, p, w, mode)
            M.compare(kind, cat, want[mode, weighted], (layout, mode, weighted, "single-table calls vs the oracle"))
            for it, ot in types:
                d_ids = torch.from_numpy(p["ids"].astype(INT[it][0])).cuda()
                d_off = None if hot else torch.from_numpy(p["offsets"].astype(INT[ot][0])).cuda()
                for row_loads in (None, "streaming"):
                    label = (layout, mode, weighted, it, ot, row_loads)
                    out = prefilled(kind, (batch, T, group_widths[0]) if family == "same" else (batch, D))
                    back = call(group, d_ids, d_off, w, batch_size=batch, num_hots=hot, mode=mode, row_loads=row_loads,
                                out=out)
                    assert back.data_ptr() == out.data_ptr()
                    got = device_bits(out).reshape(batch, D)
                    a, b = M.compare(kind, got, want[mode, weighted], label + ("vs the oracle",))
                    M.compare(kind, got, cat, label + ("vs single-table calls",))
                    by_bits, by_class, calls = by_bits + a, by_class + b, calls + 1
    print("%s %s %s B=%d: %d calls, %d elements by bits, %d by class"
          % (call.__name__, kind, group_widths, batch, calls, by_bits, by_class))
    assert by_class > 0 and by_class <= F.NAN_CAP * (by_bits + by_class)
