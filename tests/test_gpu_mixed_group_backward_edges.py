"""embedding_backward_mixed_group and mixed_group_mean_scale on non-finite and signed-zero gradients, against
backward_edge_model.py (mixed_group_problem): a planted +Inf, -Inf or NaN element of grad_y [B, D] must reach exactly the
(row, column) pairs that look it up -- the plants sit at the first and last column of a table's slice, directly beside
the neighbouring table's columns, so a lane active past W_t or a source offset that is off by one table carries one into
rows of the wrong table -- a sum of zeros is +0, and the mean's scale gives Inf * 0 = NaN and -x * 0 = -0 in empty bags and
in bags whose weights sum to exactly 0.

Comparison rule (backward_edge_model.compare): where the model is NaN the device is NaN; everywhere else the bits are
identical.  Columns at or past W_t of an entry of the padded gradient are unspecified and stay uncompared.
test_mixed_group_backward_edges_host.py asserts, without a GPU, that the plants are looked up and that at most one
expected element in four is NaN.

Not here: the group optimizer steps on IEEE edges, the exchange kernels, and the forwards (test_gpu_forward_edges.py).
"""
import numpy as np
import pytest
import torch

import backward_edge_model as M
import mixed_group_backward_reference as MR
from test_mixed_group_backward_edges_host import mixed_model, scaled_grad_y

pytestmark = pytest.mark.gpu

TORCH = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
ident = lambda v: "w" + "_".join(map(str, v)) if isinstance(v, tuple) else str(v)


@pytest.fixture(scope="module")
def ce():
    import cuembed_amd
    assert torch.cuda.is_available()
    return cuembed_amd


def on_device(bits, kind):
    a = np.array(bits, order="C")          # (a copy: the cached problems are read-only)
    return torch.from_numpy(a.view(np.int16 if a.dtype.itemsize == 2 else np.int32)).cuda().view(TORCH[kind])


def device_bits(t):
    t = t.detach().contiguous()
    wide = t.element_size() == 4
    return t.view(torch.int32 if wide else torch.int16).cpu().numpy().view(np.uint32 if wide else np.uint16)


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


_GROUPS = {}


def group_of(ce, kind, widths):
    """(the backward reads no table value)"""
    if (kind, widths) not in _GROUPS:
        _GROUPS[kind, widths] = ce.MixedTableGroup([torch.zeros(M.MIXED_ROWS[t], w, dtype=TORCH[kind], device="cuda")
                                                    for t, w in enumerate(widths)])
    return _GROUPS[kind, widths]


@pytest.mark.parametrize("widths", M.MIXED_WIDTHS, ids=ident)
@pytest.mark.parametrize("batch", M.GROUP_BATCHES)
@pytest.mark.parametrize("kind", ["f32", "f16", "bf16"])
def test_mixed_group_backward_on_planted_data(ce, kind, batch, widths):
    """Sum and mean, weighted and not, the four layouts: the ids are exactly the looked-up global rows, every entry equals
    the model in the columns [0, W_t) of its table, grad_y is left alone and the overflow word stays down."""
    group = group_of(ce, kind, widths)
    base = MR.row_base(M.MIXED_ROWS[:len(widths)])
    ce.capacity_overflowed(reset=True)
    by_bits = by_class = 0
    for layout in M.GROUP_LAYOUTS:
        p = M.mixed_group_problem(kind, batch, widths, layout)
        grad_y, offsets, ids = on_device(p["grad_y_bits"], kind), dev(p["offsets"]), dev(p["ids"])
        keys = np.unique(M.mixed_group_keys(batch, p)[0])
        table_of_key = np.searchsorted(base, keys, side="right") - 1
        for weighted in (False, True):
            w_d = on_device(p["weights_bits"], kind) if weighted else None
            for mode in ("sum", "mean"):
                sums = mixed_model(kind, batch, widths, layout, mode, weighted)[2]
                label = (layout, weighted, mode)
                g = ce.embedding_backward_mixed_group(group, grad_y, ids, offsets, w_d, num_hots=p["hot"], mode=mode)
                count = int(g.last_id.item()) + 1
                assert count == keys.size and np.array_equal(g.ids[:count].cpu().numpy(), keys), label
                got = device_bits(g.rows[:count])
                for t, w in enumerate(widths):
                    mine = table_of_key == t
                    want = M.to_bits(kind, sums[t].value[keys[mine] - base[t]])
                    a, b = M.compare(kind, got[mine, :w], want, label + (t,))
                    by_bits, by_class = by_bits + a, by_class + b
                assert np.array_equal(device_bits(grad_y), p["grad_y_bits"]), label
    assert not ce.capacity_overflowed(reset=True)
    print("embedding_backward_mixed_group %s B=%d %s: %d elements by bits, %d by class" % (kind, batch, widths, by_bits, by_class))
    assert by_class > 0


@pytest.mark.parametrize("widths", M.MIXED_WIDTHS, ids=ident)
@pytest.mark.parametrize("batch", M.GROUP_BATCHES)
@pytest.mark.parametrize("kind", ["f32", "f16", "bf16"])
def test_mixed_group_mean_scale_on_planted_data(ce, kind, batch, widths):
    """Inf * 0 = NaN and -x * 0 = -0 in bags that are empty or whose weights sum to 0: the model's bits per table slice,
    out of place and in place."""
    group = group_of(ce, kind, widths)
    by_bits = by_class = 0
    for layout in M.GROUP_LAYOUTS:
        p = M.mixed_group_problem(kind, batch, widths, layout)
        grad_y, offsets = on_device(p["grad_y_bits"], kind), dev(p["offsets"])
        for weighted in (False, True):
            w_d = on_device(p["weights_bits"], kind) if weighted else None
            want = M.to_bits(kind, scaled_grad_y(kind, batch, p, weighted))
            got = ce.mixed_group_mean_scale(group, grad_y, offsets, w_d, num_hots=p["hot"])
            assert got.data_ptr() != grad_y.data_ptr()
            a, b = M.compare(kind, device_bits(got), want, (layout, weighted))
            assert b > 0
            by_bits, by_class = by_bits + a, by_class + b
            assert np.array_equal(device_bits(grad_y), p["grad_y_bits"])          # the source is left alone
            work = grad_y.clone()
            back = ce.mixed_group_mean_scale(group, work, offsets, w_d, num_hots=p["hot"], out=work)
            assert back is work
            M.compare(kind, device_bits(work), want, (layout, weighted, "in place"))
    print("mixed_group_mean_scale %s B=%d %s: %d elements by bits, %d by class" % (kind, batch, widths, by_bits, by_class))
