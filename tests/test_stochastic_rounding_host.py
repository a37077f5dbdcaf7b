"""Stochastic rounding of the sparse optimizer step, on the CPU: the random bits (Philox4x32-10) and the rounding rules of
the library -- the same __host__ __device__ text the kernel runs, reached through the C ABI's host helpers -- against the
numpy reference (tests/stochastic_rounding_reference.py); the symptom the feature cures and the cure, on the reference;
the ABI; and the argument contract."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import stochastic_rounding_reference as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cuembed_amd.h")
DTYPE = {"fp16": torch.float16, "bf16": torch.bfloat16}

KNOWN_ANSWERS = [      # Random123's known answers: (counter, key) -> output
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def _lib_round(kind, x, r):
    """The library's rule on arrays: uint16 patterns."""
    import cuembed_amd as ce
    x, r = np.broadcast_arrays(np.asarray(x, dtype=np.float32), np.asarray(r, dtype=np.int32))
    out = ce.stochastic_round_array(DTYPE[kind], torch.from_numpy(np.ascontiguousarray(x)).reshape(-1),
                                    torch.from_numpy(np.ascontiguousarray(r)).reshape(-1))
    return out.numpy().astype(np.uint16).reshape(x.shape)


# ---- the bits ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("counter,key,want", KNOWN_ANSWERS)
def test_philox_known_answers(counter, key, want):
    import cuembed_amd as ce
    got = [int(w) for w in S.philox4x32_10(counter, key)]
    assert got == list(want)
    # through the library: counter = (row lo, row hi, group, step lo), key = (seed lo, seed hi ^ step hi)
    row = counter[0] | (counter[1] << 32)
    row = row - 2 ** 64 if row >= 2 ** 63 else row                   # (the row travels as int64)
    step = counter[3]                                                # step hi = 0: key[1] = seed hi
    assert ce.stochastic_rounding_words(key[0] | (key[1] << 32), step, row, counter[2]) == want
    # ... and with the key's high word split between seed and step
    step_hi = 0x5a5a5a5a
    seed = key[0] | ((key[1] ^ step_hi) << 32)
    assert ce.stochastic_rounding_words(seed, step | (step_hi << 32), row, counter[2]) == want


def test_fields_follow_the_layout():
    import cuembed_amd as ce
    seed, step = 0x1234567, 41
    f = S.fields(seed, step, [7, 2 ** 33 + 5], 21)
    for i, row in enumerate((7, 2 ** 33 + 5)):
        for c in range(21):
            w = ce.stochastic_rounding_words(seed, step, row, c // 8)
            assert int(f[i, c]) == (w[(c % 8) // 2] >> (16 * (c % 2))) & 0xFFFF
    assert len({int(v) for v in f.reshape(-1)}) > 35         # 42 fields, (almost) all different


# ---- the rules --------------------------------------------------------------------------------------------------------
def _finite_patterns(kind):
    p = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    return p[np.isfinite(S.to_f32(p, kind))]


@pytest.mark.parametrize("kind", ["fp16", "bf16"])
def test_representable_values_are_unchanged_for_every_field(kind):
    p = _finite_patterns(kind)
    if kind == "fp16":
        assert p.size == 63488
    x = S.to_f32(p, kind)
    for r in (0, 1, 0x1FFF, 0xFFFF):
        assert np.array_equal(_lib_round(kind, x, r), p), "r = %#x" % r      # (patterns: the sign of zero included)
        assert np.array_equal(S.stochastic(x, r, kind), p)
    import cuembed_amd as ce
    assert ce.stochastic_round(DTYPE[kind], -0.0, 0xFFFF) == 0x8000 and ce.stochastic_round(DTYPE[kind], 0.0, 0xFFFF) == 0


def _fp16_probe_values():
    rng = np.random.default_rng(5)
    vals = []
    for e in range(-24, 16):                                  # every binade of fp16, subnormals included (e < -14)
        vals += list(np.ldexp(1.0 + rng.random(5), e))
    vals += list(np.ldexp(rng.random(20), -24))               # below the smallest subnormal
    vals += [2.0 ** -14 - 2.0 ** -30, 2.0 ** -14 + 2.0 ** -30, 2.0 ** -14 - 2.0 ** -25, 1023.75 * 2.0 ** -24,
             2.0 ** -25, 2.0 ** -37, 2.0 ** -38, 1e-40, 2.0 ** -149]              # the subnormal / normal boundary, tiny values
    vals += [65504.0 + 1.0, 65504.0 + 31.99, 65519.0, 65520.0, 65535.0, 65535.996, 65536.0, 1e5, 3e38]   # up to overflow
    vals += [1.0 + 2.0 ** -11, 1.0 + 2.0 ** -23, 1.0 - 2.0 ** -24, 0.1, 1.0 / 3.0]
    v = np.array(vals, dtype=np.float32)
    return np.concatenate([v, -v])


def _bf16_probe_values():
    rng = np.random.default_rng(6)
    bits = rng.integers(0, 0x7F800000, size=80, dtype=np.int64).astype(np.uint32)     # anywhere, finite
    sub = rng.integers(1, 0x00800000, size=20, dtype=np.int64).astype(np.uint32)      # fp32 subnormals
    edge = np.array([0x7F7F0001, 0x7F7FFFFF, 0x7F7F8000, 0x00000001, 0x007FFFFF, 0x00800000, 0x3F800001, 0x3F80FFFF],
                    dtype=np.uint32)                                                  # the top binade up to overflow, ...
    b = np.concatenate([bits, sub, edge])
    return np.concatenate([b, b | np.uint32(0x80000000)]).view(np.float32)


@pytest.mark.parametrize("kind", ["fp16", "bf16"])
def test_rule_equals_the_reference_for_every_field(kind):
    x = _fp16_probe_values() if kind == "fp16" else _bf16_probe_values()
    assert x.size >= 200
    nr = 8192 if kind == "fp16" else 65536
    r = np.arange(nr, dtype=np.int32)
    got = _lib_round(kind, x[:, None], r[None, :])
    want = S.stochastic(x[:, None], r[None, :], kind)
    assert np.array_equal(got, want)
    # among all fields exactly t (fp16) / the low 16 bits (bf16) round away from zero, the rest towards it
    down = got[:, 0]                                                         # r = 0 truncates
    ups = (got != down[:, None]).sum(axis=1)
    if kind == "bf16":
        t = x.view(np.uint32) & np.uint32(0xFFFF)
    else:
        a = np.abs(x).astype(np.float64)
        _, ex = np.frexp(a)
        q = np.where(a >= 2.0 ** -14, np.ldexp(1.0, ex - 11), 2.0 ** -24)
        m = a / q
        t = np.floor((m - np.floor(m)) * 8192).astype(np.int64)
        t = np.where(a >= 65536.0, 0, t)             # past the top binade both "neighbours" are inf
    assert np.array_equal(ups, t)
    # the results are the two neighbours of x in the table's type: towards zero, and -- where any field rounds up -- the
    # next pattern (fp16's subnormal range drops fraction bits past the 13th, so a tiny fraction may never round up)
    mag = (got & np.uint16(0x7FFF)).astype(np.int64)
    low = mag.min(axis=1)
    assert np.array_equal(mag.max(axis=1), low + (t > 0))
    ax = np.abs(x).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        below = S.to_f32(low.astype(np.uint16), kind).astype(np.float64)
        above = S.to_f32((low + 1).astype(np.uint16), kind).astype(np.float64)
    finite_result = low < (0x7C00 if kind == "fp16" else 0x7F80)
    assert ((below <= ax) & (ax < above))[finite_result].all()
    assert ((got >> 15) == np.signbit(x)[:, None]).all()


@pytest.mark.parametrize("kind", ["fp16", "bf16"])
def test_inf_nan_and_overflow(kind):
    inf = 0x7C00 if kind == "fp16" else 0x7F80
    big = np.float32(65535.0) if kind == "fp16" else np.array([0x7F7FFFFF], dtype=np.uint32).view(np.float32)[0]
    mask = 0x1FFF if kind == "fp16" else 0xFFFF
    for r in (0, 1, mask, 0xFFFF):
        assert int(_lib_round(kind, np.float32(np.inf), r)) == inf
        assert int(_lib_round(kind, np.float32(-np.inf), r)) == inf | 0x8000
        nan = int(_lib_round(kind, np.float32(np.nan), r))
        assert nan & inf == inf and nan & (0x03FF if kind == "fp16" else 0x007F) != 0
        assert np.isnan(S.to_f32(S.stochastic(np.float32(np.nan), r, kind), kind))
    assert int(_lib_round(kind, big, mask)) == inf and int(_lib_round(kind, -big, mask)) == inf | 0x8000
    assert int(_lib_round(kind, big, 0)) == inf - 1                            # the largest finite value
    assert int(S.stochastic(big, mask, kind)) == inf
    assert int(S.nearest(big, kind)) == inf                                    # as round-to-nearest does


# ---- the symptom and the cure, on the reference -----------------------------------------------------------------------
@pytest.fixture(scope="module", params=["fp16", "bf16"])
def walked(request):
    """64 x 256 table of 1.0, g = 1, lr = 2^-17 (fp16) / 2^-14 (bf16), seed 0x1234567, steps 0..511."""
    assert (S.WALK_ROWS, S.WALK_WIDTH, S.WALK_STEPS, S.WALK_SEED) == (64, 256, 512, 0x1234567)
    assert S.WALK_LR == {"fp16": 2.0 ** -17, "bf16": 2.0 ** -14}
    return (request.param,) + S.walk(request.param)


def test_round_to_nearest_loses_the_updates_and_stochastic_rounding_keeps_them(walked):
    kind, table, moves, plain = walked
    one = int(S.nearest(np.float32(1.0), kind))
    assert (plain == one).all()                    # the symptom: 512 updates of 1/64 of a spacing, all rounded away
    # every step moves an element one spacing down with probability exactly 1/64: moves ~ Binomial(512, 1/64)
    assert np.array_equal(one - table.astype(np.int64), moves)       # (below 1.0 the spacing halves: it stays in reach)
    n = moves.size
    mean, var = moves.mean(), moves.var(ddof=1)
    print("%s: mean %.4f variance %.4f" % (kind, mean, var))
    assert abs(mean - 8.0) <= 0.11                 # 5 sigma of the mean over 16,384 elements, sigma^2 = 7.875
    assert abs(var - 7.875) <= 0.45                # 5 standard errors
    z = (moves - mean) / moves.std()
    along_columns = float((z[:, 1:] * z[:, :-1]).mean())
    along_rows = float((z[1:, :] * z[:-1, :]).mean())
    print("%s: lag-1 correlation along columns %.4f, along rows %.4f" % (kind, along_columns, along_rows))
    assert abs(along_columns) < 0.039 and abs(along_rows) < 0.039      # 5 / sqrt(n): no bits shared inside a call / across rows
    assert n == 16384


# ---- ABI --------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("cuembed_sparse_row_update_stochastic", "cuembed_stochastic_rounding_words", "cuembed_stochastic_round")


def test_entry_points_are_declared_in_plain_c_and_exported():
    from cuembed_amd import build
    pre = subprocess.run(["gcc", "-E", "-P", HEADER], check=True, stdout=subprocess.PIPE, text=True).stdout
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, pre), name
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", HEADER], check=True)
    L = ctypes.CDLL(build.build())
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
    assert "c_api_optimizer_stochastic.hip" in build.UNITS and "c_api_optimizer.hip" in build.UNITS
    # the existing entry point keeps its declaration, and the new one is the same arguments + (seed, step, step_device)
    flat = re.sub(r"\s+", " ", pre)
    old = ("void cuembed_sparse_row_update(void* table, int elem_type, int embed_width, float* state, int rule, "
           "const void* ids, int index_type, const void* rows, int64_t piece_rows, int pieces, int64_t num_rows, "
           "const void* counts, int counts_are_int64, const void* last_id, float lr, const float* lr_device, float eps, "
           "cuembed_stream_t stream);")
    decl = re.search(r"void cuembed_sparse_row_update\(.*?\);", flat).group(0)
    assert decl == old
    new = re.search(r"void cuembed_sparse_row_update_stochastic\((.*?)\);", flat).group(1)
    assert new.startswith(re.search(r"\((.*), cuembed_stream_t stream\)", decl).group(1))
    assert re.search(r"float eps, \w+ seed, \w+ step, const \w+\s?\* ?step_device, cuembed_stream_t stream$", new)


# ---- argument contract (CPU tensors: every rejection comes before the device check) -----------------------------------
def _args(dtype=torch.float16, ncat=20, width=8, n=5):
    return torch.zeros((ncat, width), dtype=dtype), torch.arange(n, dtype=torch.int64), torch.zeros((n, width), dtype=dtype)


def test_sparse_row_update_rejects_stochastic_misuse_before_any_launch():
    import cuembed_amd as ce
    table, ids, rows = _args()
    f32 = _args(torch.float32)
    with pytest.raises(TypeError, match="float32 table"):
        ce.sparse_row_update(*f32, rule="sgd", lr=0.1, stochastic_rounding=True)
    for seed in (-1, 2 ** 64, 1.5, "7"):
        with pytest.raises(ValueError, match="seed"):
            ce.sparse_row_update(table, ids, rows, rule="sgd", lr=0.1, stochastic_rounding=True, seed=seed)
    for step in (-1, 2 ** 64, 0.5):
        with pytest.raises(ValueError, match="step"):
            ce.sparse_row_update(table, ids, rows, rule="sgd", lr=0.1, stochastic_rounding=True, step=step)
    with pytest.raises(TypeError, match="step"):
        ce.sparse_row_update(table, ids, rows, rule="sgd", lr=0.1, stochastic_rounding=True,
                             step=torch.zeros(1, dtype=torch.int32))
    with pytest.raises(TypeError, match="step"):
        ce.sparse_row_update(table, ids, rows, rule="sgd", lr=0.1, stochastic_rounding=True,
                             step=torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError, match="device"):
        ce.sparse_row_update(table, ids, rows, rule="sgd", lr=0.1, stochastic_rounding=True,
                             step=torch.zeros(1, dtype=torch.int64, device="meta"))
    # everything in order (the largest seed and step included): only the device is wrong
    with pytest.raises(RuntimeError, match="GPU"):
        ce.sparse_row_update(table, ids, rows, rule="sgd", lr=0.1, stochastic_rounding=True, seed=2 ** 64 - 1,
                             step=2 ** 64 - 1)
    with pytest.raises(RuntimeError, match="GPU"):
        ce.sparse_row_update(table, ids, rows, rule="sgd", lr=0.1, stochastic_rounding=True,
                             step=torch.zeros(1, dtype=torch.int64))
    # off: the keywords are not looked at, as before
    with pytest.raises(RuntimeError, match="GPU"):
        ce.sparse_row_update(*f32, rule="sgd", lr=0.1)
    with pytest.raises(TypeError):
        ce.stochastic_round(torch.float32, 1.0, 0)


def test_front_ends_take_and_check_the_keywords():
    from cuembed_amd import optim
    table = torch.zeros((20, 8), dtype=torch.bfloat16)
    with pytest.raises(TypeError, match="float32 table"):
        optim.SparseUpdater(table.float(), "sgd", 0.1, stochastic_rounding=True)
    with pytest.raises(ValueError, match="seed"):
        optim.SparseUpdater(table, "sgd", 0.1, stochastic_rounding=True, seed=-3)
    u = optim.SparseUpdater(table, "rowwise_adagrad", 0.1, stochastic_rounding=True, seed=9)
    assert u.rounding_step.dtype == torch.int64 and u.rounding_step.numel() == 1 and int(u.rounding_step) == 0
    assert optim.SparseUpdater(table, "sgd", 0.1).rounding_step is None
    p = torch.nn.Parameter(table.clone())
    for cls in (optim.SparseSGD, optim.SparseAdagrad, optim.RowwiseAdagrad):
        with pytest.raises(TypeError, match="float32 table"):
            cls([torch.nn.Parameter(table.float())], lr=0.1, stochastic_rounding=True)
        with pytest.raises(ValueError, match="seed"):
            cls([p], lr=0.1, stochastic_rounding=True, seed=2 ** 64)
        a = cls([p], 0.1, stochastic_rounding=True, seed=77)               # (lr stays positional)
        assert a.state[p]["rounding_step"] == 0 and a.param_groups[0]["seed"] == 77
        a.state[p]["rounding_step"] = 12
        b = cls([p], lr=0.1, stochastic_rounding=True, seed=1)
        b.load_state_dict(a.state_dict())
        assert b.state[p]["rounding_step"] == 12 and b.param_groups[0]["seed"] == 77
        assert "rounding_step" not in cls([p], lr=0.1).state[p]
