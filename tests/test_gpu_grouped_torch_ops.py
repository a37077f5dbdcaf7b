"""The grouped forward as torch ops (cuembed_pyt::cuemb_embedding_grouped and its quantized twin): they exist, their
fake implementations give the right shape and dtype, the modules agree with the functions, and one call is captured
into a HIP graph and replayed on new indices."""
import numpy as np
import pytest
import torch

import grouped_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ce():
    import cuembed_amd
    assert torch.cuda.is_available()
    return cuembed_amd


@pytest.fixture(scope="module")
def pyt():
    from cuembed_amd import cuembed_pyt
    return cuembed_pyt


@pytest.fixture(scope="module")
def problem():
    width, batch = 128, 5
    tables = [torch.from_numpy(C.table_values(t, rows, width).astype(np.float16)).cuda() for t, rows in enumerate(C.ROWS)]
    layouts = {name: (torch.from_numpy(ids).cuda(), None if off is None else torch.from_numpy(off).cuda(), hot,
                      torch.from_numpy(w.astype(np.float16)).cuda())
               for name, ids, off, hot, w in C.layouts(batch)}
    return width, batch, tables, layouts


def test_the_ops_exist_and_agree_with_the_functions(ce, pyt, problem):
    width, batch, tables, layouts = problem
    assert hasattr(torch.ops.cuembed_pyt, "cuemb_embedding_grouped")
    assert hasattr(torch.ops.cuembed_pyt, "cuemb_embedding_quantized_grouped")
    group = ce.TableGroup(tables)
    qgroup = ce.TableGroup([ce.quantize_rows(t) for t in tables])
    for name, (ids, off, hot, w) in layouts.items():
        idx = ids if off is not None else ids.view(len(tables), batch, hot)
        for mode in ("sum", "mean"):
            for weights in (None, w):
                want = ce.embedding_forward_grouped(group, ids, off, weights, num_hots=hot, mode=mode)
                got = pyt.cuemb_embedding_grouped(group, idx, off, weights, mode=mode)
                assert got.dtype == want.dtype and torch.equal(got, want), (name, mode)
                raw = torch.ops.cuembed_pyt.cuemb_embedding_grouped(tables, group.table_ptrs, idx, off, weights, mode)
                assert torch.equal(raw, want), (name, mode)
                for out_dtype in (torch.float16, torch.float32):
                    qw = None if weights is None else weights.to(out_dtype)
                    want = ce.embedding_forward_quantized_grouped(qgroup, ids, off, qw, num_hots=hot, mode=mode,
                                                                  out_dtype=out_dtype)
                    got = pyt.cuemb_embedding_quantized_grouped(qgroup, idx, off, qw, mode=mode, out_dtype=out_dtype)
                    assert got.dtype == out_dtype and torch.equal(got, want), (name, mode, out_dtype)


def test_the_ops_reject_what_the_functions_reject(ce, pyt, problem):
    width, batch, tables, layouts = problem
    group = ce.TableGroup(tables)
    ids, off, _, _ = layouts["csr_ragged"]
    with pytest.raises(RuntimeError):
        torch.ops.cuembed_pyt.cuemb_embedding_grouped(tables, group.table_ptrs, ids, off, None, "concat")
    with pytest.raises(RuntimeError):     # offsets of a length that is not num_tables * batch + 1
        torch.ops.cuembed_pyt.cuemb_embedding_grouped(tables, group.table_ptrs, ids, off[:-1], None, "sum")
    with pytest.raises(RuntimeError):     # one pointer per table
        torch.ops.cuembed_pyt.cuemb_embedding_grouped(tables, group.table_ptrs[:2].contiguous(), ids, off, None, "sum")
    with pytest.raises(RuntimeError):     # one width per group
        torch.ops.cuembed_pyt.cuemb_embedding_grouped(tables[:2] + [tables[2][:, :64].contiguous()], group.table_ptrs, ids,
                                                      off, None, "sum")
    needs_grad = [t.clone().requires_grad_(True) for t in tables]
    with pytest.raises(RuntimeError):     # forward only
        pyt.cuemb_embedding_grouped(ce.TableGroup(needs_grad), ids, off)
    with pytest.raises(RuntimeError):
        ce.embedding_forward_grouped(needs_grad, ids, off)
    with torch.no_grad():
        assert torch.equal(pyt.cuemb_embedding_grouped(ce.TableGroup(needs_grad), ids, off),
                           ce.embedding_forward_grouped(group, ids, off))


def test_fake_implementations_give_shape_and_dtype(ce, pyt, problem):
    from torch._subclasses.fake_tensor import FakeTensorMode
    width, batch, tables, layouts = problem
    T = len(tables)
    with FakeTensorMode():
        f_tables = [torch.empty((rows, width), dtype=torch.float16, device="cuda") for rows in C.ROWS]
        q_tables = [torch.empty((rows, width + 8), dtype=torch.uint8, device="cuda") for rows in C.ROWS]
        ptrs = torch.empty((T,), dtype=torch.int64, device="cuda")
        ids = torch.empty((40,), dtype=torch.int32, device="cuda")
        off = torch.empty((T * batch + 1,), dtype=torch.int64, device="cuda")
        fixed = torch.empty((T, batch, 7), dtype=torch.int32, device="cuda")
        for idx, o in ((ids, off), (fixed, None)):
            out = torch.ops.cuembed_pyt.cuemb_embedding_grouped(f_tables, ptrs, idx, o, None, "sum")
            assert tuple(out.shape) == (batch, T, width) and out.dtype == torch.float16 and out.device.type == "cuda"
            for dt in (torch.float16, torch.float32):
                out = torch.ops.cuembed_pyt.cuemb_embedding_quantized_grouped(q_tables, ptrs, idx, o, None, "mean", dt)
                assert tuple(out.shape) == (batch, T, width) and out.dtype == dt


def test_the_modules_agree_with_the_functions(ce, problem):
    width, batch, tables, layouts = problem
    bags = ce.EmbeddingBagGroup(tables, mode="mean")
    qbags = ce.QuantizedEmbeddingBagGroup.from_float(tables, mode="sum", out_dtype=torch.float32)
    assert bags.num_tables == 3 and bags.embedding_dim == width and qbags.embedding_dim == width
    for name, (ids, off, hot, w) in layouts.items():
        idx = ids if off is not None else ids.view(len(tables), batch, hot)
        assert torch.equal(bags(idx, off, w), ce.embedding_forward_grouped(bags.group, ids, off, w, num_hots=hot, mode="mean"))
        w32 = w.float()
        assert torch.equal(qbags(idx, off, w32),
                           ce.embedding_forward_quantized_grouped(qbags.group, ids, off, w32, num_hots=hot, mode="sum",
                                                                  out_dtype=torch.float32))
        for t, table in enumerate(tables):
            assert torch.equal(qbags.group.tables[t], ce.quantize_rows(table))


def test_one_grouped_call_under_hip_graph_capture(ce, pyt):
    """One linear stream, no parallel branches; the indices are rewritten in place between replays; the replayed result
    equals the eager one."""
    width, batch, T = 128, 64, 3
    tables = [torch.from_numpy(C.table_values(t, rows, width).astype(np.float16)).cuda() for t, rows in enumerate(C.ROWS)]
    group = ce.TableGroup(tables)
    rng = np.random.default_rng(3)
    lengths = np.full((T, batch), 9)
    offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(lengths.reshape(-1))])).cuda()
    idx = torch.from_numpy(C.draw_ids(rng, C.ROWS, lengths)).cuda()
    out = torch.empty((batch, T, width), dtype=torch.float16, device="cuda")
    static = {}

    def step():
        ce.embedding_forward_grouped(group, idx, offsets, mode="sum", out=out)
        static["op"] = pyt.cuemb_embedding_grouped(group, idx, offsets, mode="sum")

    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        step()                               # warm-up outside capture (library / module loading)
        torch.cuda.current_stream().synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            step()
    for seed in (4, 5):
        idx.copy_(torch.from_numpy(C.draw_ids(np.random.default_rng(seed), C.ROWS, lengths)).cuda())
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        eager = ce.embedding_forward_grouped(group, idx, offsets, mode="sum")
        assert torch.equal(out, eager) and torch.equal(static["op"], eager), seed
