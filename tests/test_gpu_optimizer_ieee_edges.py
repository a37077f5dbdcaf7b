"""The sparse optimizer step on IEEE edge data, bit for bit against an independent model: cuembed_amd.sparse_row_update /
sparse_row_adam against optimizer_bits_reference.py (numpy float32, one IEEE operation per line, the row sum in the
kernel's lane order), two consecutive steps, the WHOLE table and every state tensor compared after each -- so the second
step starts from edge-valued state.

Comparison rule: where the model's value is NaN the device's must be NaN (payload and sign are free: x86 and the GPU
propagate NaNs differently); everywhere else the bits must be identical -- the sign of zero, infinities and subnormals
included.  The kernels' divisions and sqrtf are plain C++; that they are correctly rounded and keep subnormals rests on
compiler defaults and on the build's flags, which nothing else in the suite would miss.

The data (edge_problem) is bit patterns from an integer hash: 512 table rows, 200 valid entries naming distinct rows and
5 entries past the count.  The valid entries are, in this order,

  bulk (148)     finite only: random sign and mantissa, the exponent drawn per row from regimes in which squares
                 underflow to zero ("deep") or to subnormals ("small"), are ordinary ("mid"), come close to FLT_MAX
                 ("big") or overflow to infinity ("over"); an fp16 square cannot leave fp32's normal range (2^-48 ..
                 2^32), so fp16's regimes are the ends of its own range; the state is zero, ordinary or of the squares' size
  subnormal (12) subnormal gradients and weights of the table's type (some +-0), fp32 state that is subnormal (every
                 other row: ordinary): sqrt of a subnormal, a subnormal numerator
  zero (12)      g = +-0 on zero state (every other row: subnormal state) under weights +0, -0, subnormal and ordinary:
                 0 / 0 with eps = 0, and the sign of a zero result
  huge (10)      state near and at FLT_MAX under gradients of the "big" regime: s + g * g overflows (not for fp16)
  store (12)     weights at +-the largest finite value stepped outward by large gradients (SGD) or large first moments
                 swept over exponents (the Adam rules); weights just above the smallest normal stepped inward; exact
                 ties at the store of a 16-bit table (g = +-1.5625 * 2^j, lr * g = 2^(j - 6) to within 2^-25, j = -1 .. 2)
  special (6)    one +inf / -inf / NaN gradient element, one +inf / -inf weight, one infinite state element -- only
                 here: such an element turns a whole row NaN under the row-wise rules

What of this a rule and a type can reach, and the cap on the share of NaNs (they are compared by class only), is
edge_conditions below; test_optimizer_bits_host.py asserts it for every case from the model alone.
"""
import functools

import numpy as np
import pytest
import torch

import adam_reference as AR
import optimizer_bits_reference as B
from test_gpu_alignment_variants import lane_bytes, shifted
from test_gpu_optimizer_step_bits import BETAS, INDEX, LR, ROUNDINGS, RULES, SEED, STEPS, TORCH, permutation

pytestmark = pytest.mark.gpu

NCAT, N, TAIL = 512, 200, 5
#: width -> the body of the walk (test_gpu_optimizer_step_bits.WIDTHS): one slice with one or two entries in flight,
#: 4-byte or 8-byte lanes, four slices with a partial one, the run-time loop
WIDTHS = {"f16": (8, 50, 64, 1000, 2056), "bf16": (8, 50, 64, 1000, 2056), "f32": (8, 50, 64, 1000, 2048)}
EPSILONS = (1e-8, 0.0)
WEIGHT_DECAYS = {"sgd": (0.0,), "adagrad": (0.0,), "rowwise_adagrad": (0.0,), "adam": (0.0, 0.01), "rowwise_adam": (0.0, 0.01)}
SHIFTED_WIDTHS, SHIFTS = (64, 1000), (4, 8)
NAN_SHARE = 0.05

#: (exponent bits, mantissa bits) of a type
FORMAT = {"f32": (8, 23), "f16": (5, 10), "bf16": (8, 7)}
#: true exponents [lo, hi] of the bulk's regimes
REGIMES = {"wide": dict(deep=(-90, -76), small=(-74, -64), mid=(-6, 3), big=(60, 63), over=(64, 70)),
           "f16": dict(deep=(-14, -14), small=(-13, -10), mid=(-6, 3), big=(10, 13), over=(14, 15))}
#: regime of a bulk row by hash % 16
REGIME_OF = ("deep",) + ("small",) * 3 + ("mid",) * 7 + ("big",) * 3 + ("over",) * 2
CLASSES = (("bulk", 148), ("subnormal", 12), ("zero", 12), ("huge", 10), ("store", 12), ("special", 6))
assert sum(c for _, c in CLASSES) == N


def mix(rows, cols, salt):
    """uint32 [len(rows), len(cols)]: a multiplicative hash of (row, column, salt), in 64-bit integer arithmetic reduced
    mod 2^32 (the construction of test_gpu_optimizer_step_bits.hashed)."""
    mask = np.uint64(0xFFFFFFFF)
    r = np.asarray(rows, dtype=np.uint64).reshape(-1, 1)
    c = np.asarray(cols, dtype=np.uint64).reshape(1, -1)
    h = (r * np.uint64(0x9E3779B1) + c * np.uint64(0x85EBCA6B) + np.uint64((salt * 0xC2B2AE35 + 0x1B873593) & 0xFFFFFFFF)) & mask
    h = (h * np.uint64(0x27D4EB2F)) & mask
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(0x165667B1)) & mask
    h ^= h >> np.uint64(13)
    return h.astype(np.uint32)


def pattern(kind, sign, exponent, mantissa):
    """Bit patterns of `kind` from a sign (0 / 1), a TRUE exponent (below the smallest normal: subnormal, mantissa as
    given) and a mantissa field; everything broadcasts."""
    ebits, mbits = FORMAT[kind]
    bias = (1 << (ebits - 1)) - 1
    field = np.clip(np.asarray(exponent, dtype=np.int64) + bias, 0, (1 << ebits) - 2)
    m = np.asarray(mantissa, dtype=np.int64) & ((1 << mbits) - 1)
    out = (np.asarray(sign, dtype=np.int64) << (ebits + mbits)) | (field << mbits) | m
    return out.astype(B.BITS[kind])


def special(kind, what):
    ebits, mbits = FORMAT[kind]
    top = ((1 << ebits) - 1) << mbits
    return {"+inf": top, "-inf": top | (1 << (ebits + mbits)), "nan": top | (1 << (mbits - 1)),
            "+max": top - 1, "-max": (top - 1) | (1 << (ebits + mbits))}[what]


def class_ranges():
    out, at = {}, 0
    for name, count in CLASSES:
        out[name] = np.arange(at, at + count)
        at += count
    return out


def drawn_exponents(kind, keys, salt, regime_names):
    """One true exponent per key, inside the regime its name gives."""
    regimes = REGIMES["f16" if kind == "f16" else "wide"]
    lo = np.array([regimes[r][0] for r in regime_names])
    hi = np.array([regimes[r][1] for r in regime_names])
    return lo + mix(keys, [0], salt)[:, 0].astype(np.int64) % (hi - lo + 1)


def fill(kind, keys, width, salt, exponent, zero_where=None):
    """Random sign and mantissa at the given true exponent(s) ([n] or [n, W]); zero_where: +-0 instead."""
    ebits, mbits = FORMAT[kind]
    h = mix(keys, np.arange(width), salt).astype(np.int64)
    e = np.asarray(exponent)
    e = e[:, None] if e.ndim == 1 else e
    out = pattern(kind, h >> 31, e, h >> 3)
    if zero_where is not None:
        out = np.where(zero_where, pattern(kind, h >> 31, -10_000, 0), out)
    return out


def subnormal(kind, keys, width, salt, signed=True):
    """Subnormals of `kind` with a non-zero random mantissa."""
    ebits, mbits = FORMAT[kind]
    h = mix(keys, np.arange(width), salt).astype(np.int64)
    return pattern(kind, (h >> 31) if signed else 0, -10_000, ((h >> 3) & ((1 << mbits) - 1)) | 1)


@functools.lru_cache(maxsize=None)
def edge_problem(kind, width):
    """The data of one (type, width), as read-only bit patterns: dict(table, ids, grads = [step 1, step 2],
    e = the per-element state's start for s / v, m = for exp_avg, r = the per-row state's start, classes, regimes)."""
    ebits, mbits = FORMAT[kind]
    cols = np.arange(width)
    ids = permutation(NCAT, N)
    unnamed = np.setdiff1d(np.arange(NCAT), ids)
    ids = np.concatenate([ids, ids[:3], unnamed[:TAIL - 3]])
    k_of = class_ranges()
    entries = np.arange(N)
    regime_names = np.array([REGIME_OF[h % 16] for h in mix(entries, [0], 11)[:, 0]])
    regime_names[k_of["huge"]] = "big"
    regime_names[~np.isin(entries, np.concatenate([k_of["bulk"], k_of["huge"]]))] = "mid"
    e_g = drawn_exponents(kind, entries, 12, regime_names)
    e_mid = drawn_exponents(kind, entries, 13, np.array(["mid"] * N))
    odd = (cols % 2 == 1)[None, :]
    big_mantissa = (1 << 23) - 1 - (mix(entries, cols, 14).astype(np.int64) & 0xFFFF)

    # ---- weights of the named rows, by entry; then the table
    w = fill(kind, entries, width, 20, np.where(odd, e_g[:, None], e_mid[:, None]))
    # ---- state: per element (s of Adagrad, v of Adam), m of the Adam rules, per row (s_r, v_r)
    with np.errstate(all="ignore"):
        matched = B.widen(fill(kind, entries, width, 21, e_g), kind)
        matched = np.minimum(matched * matched, np.finfo(np.float32).max).astype(np.float32).view(np.uint32)
    ordinary = pattern("f32", 0, -12 + mix(entries, cols, 22).astype(np.int64) % 15, mix(entries, cols, 23) >> 3)
    pick = (mix(entries, [0], 24)[:, 0] % 4)[:, None]
    e_state = np.where(pick == 1, matched, np.where(pick >= 2, ordinary, 0)).astype(np.uint32)
    m_state = np.where(pick >= 1, fill("f32", entries, width, 25, np.clip(e_g, -126, 100)), 0).astype(np.uint32)
    r_state = e_state[:, 0].copy()
    grads = []
    for t in STEPS:
        g = fill(kind, entries, width, 30 + t, e_g)

        # subnormal rows: every fourth gradient element +-0 (and, below, every fourth weight, at other columns)
        k = k_of["subnormal"]
        g[k] = np.where(cols % 4 == 3, fill(kind, k, width, 40 + t, 0, zero_where=True), subnormal(kind, k, width, 41 + t))
        # zero rows
        k = k_of["zero"]
        g[k] = fill(kind, k, width, 42 + t, 0, zero_where=True)
        # store rows: 0-1 large gradients swept over the four highest exponents, 2-5 the Adam rules' large moments under
        # the smallest gradients, 6-7 inward steps near the smallest normal, 8-11 exact ties at a 16-bit store
        k = k_of["store"]
        top = (1 << (ebits - 1)) - 1
        sweep = top - (np.arange(4)[:, None] + cols[None, :]) % 4
        g[k[0:2]] = fill(kind, k[0:2], width, 43 + t, sweep[0:2])
        g[k[2:6]] = fill(kind, k[2:6], width, 44 + t, 1 - top + 2)
        g[k[6:8]] = fill(kind, k[6:8], width, 45 + t, 1 - top + 7)
        j = (np.arange(4)[:, None] + cols[None, :]) % 4 - 1
        g[k[8:12]] = pattern(kind, mix(k[8:12], cols, 46 + t) >> 31, j, 0b1001 << (mbits - 4))       # +-1.5625 * 2^j
        # special rows: one element each
        k = k_of["special"]
        at = (7 * np.arange(6) + 3) % width
        g[k[0], at[0]] = special(kind, "+inf")
        g[k[1], at[1]] = special(kind, "-inf")
        g[k[2], at[2]] = special(kind, "nan")
        # entries past the count: magnitude 1
        tail = np.full((TAIL, width), pattern(kind, 0, 0, 0), dtype=B.BITS[kind])
        grads.append(np.concatenate([g, tail]))

    k = k_of["subnormal"]
    w[k] = np.where(cols % 4 == 2, fill(kind, k, width, 50, 0, zero_where=True), subnormal(kind, k, width, 51))
    even_row = (np.arange(len(k)) % 2 == 0)[:, None]
    e_state[k] = np.where(even_row, subnormal("f32", k, width, 52, signed=False), ordinary[k])
    m_state[k] = np.where(cols % 2 == 0, subnormal("f32", k, width, 53), 0)
    r_state[k] = e_state[k][:, 0]
    k = k_of["zero"]
    w[k] = np.select([cols % 4 == 0, cols % 4 == 1, cols % 4 == 2],
                     [pattern(kind, 0, -10_000, 0), pattern(kind, 1, -10_000, 0), subnormal(kind, k, width, 54)],
                     fill(kind, k, width, 55, e_mid[k]))
    even_row = (np.arange(len(k)) % 2 == 0)[:, None]
    e_state[k] = np.where(even_row, 0, subnormal("f32", k, width, 56, signed=False))
    m_state[k] = 0
    r_state[k] = e_state[k][:, 0]
    k = k_of["huge"]
    e_state[k] = np.where(cols % 4 == 0, special("f32", "+max"), pattern("f32", 0, 127, big_mantissa[k]))
    m_state[k] = fill("f32", k, width, 57, 60)
    r_state[k] = e_state[k][:, 1]
    w[k] = fill(kind, k, width, 58, e_mid[k])
    k = k_of["store"]
    top = (1 << (ebits - 1)) - 1
    outward = np.where(mix(k[0:6], cols, 59) >> 31, special(kind, "-max"), special(kind, "+max"))
    w[k[0:6]] = outward
    w[k[6:8]] = fill(kind, k[6:8], width, 60, 1 - top + (cols % 2)[None, :])
    tie_exponent = {"f32": 1, "bf16": 1, "f16": 4}[kind]      # half a unit in the last place of a 16-bit w is 2^-7 ...
    w[k[8:12]] = fill(kind, k[8:12], width, 61, tie_exponent)
    e_state[k] = ordinary[k]
    m_state[k] = 0
    # the Adam rules' outward steps: m = +-2^e swept over e = 100 .. 127 by (row, column), v small
    e_sweep = 100 + (np.arange(4)[:, None] * width + cols[None, :]) % 28
    m_state[k[2:6]] = fill("f32", k[2:6], width, 62, e_sweep)
    e_state[k[2:6]] = pattern("f32", 0, -40, mix(k[2:6], cols, 63) >> 3)
    # ... and Adagrad's tie: s = (4 - 1.5625^2) * 2^2j, so that sqrt(s + g * g) = 2^(j + 1) and d = lr * g / 2^(j + 1) = +-2^-7
    j = (np.arange(4)[:, None] + cols[None, :]) % 4 - 1
    e_state[k[8:12]] = pattern("f32", 0, 2 * j, 0x478000)       # 1.55859375 = 1 + 0x478000 / 2^23
    r_state[k] = e_state[k][:, 0]
    k = k_of["special"]
    at = (7 * np.arange(6) + 3) % width
    w[k[3], at[3]] = special(kind, "+inf")
    w[k[4], at[4]] = special(kind, "-inf")
    e_state[k[5], at[5]] = special("f32", "+inf")
    m_state[k[5], at[5]] = special("f32", "-inf")
    r_state[k[5]] = special("f32", "+inf")

    table = fill(kind, np.arange(NCAT), width, 70, drawn_exponents(kind, np.arange(NCAT), 71, np.array(["mid"] * NCAT)))
    table[ids[:N]] = w

    def spread(named, shape):
        full = pattern("f32", 0, -12 + mix(np.arange(NCAT), np.arange(shape[1]), 72).astype(np.int64) % 15,
                       mix(np.arange(NCAT), np.arange(shape[1]), 73) >> 3).astype(np.uint32)
        full[ids[:N]] = named
        return full
    out = dict(table=table, ids=ids, grads=grads, e=spread(e_state, (NCAT, width)), m=spread(m_state, (NCAT, width)),
               r=spread(r_state[:, None], (NCAT, 1))[:, 0].copy(), classes=k_of, regimes=regime_names)
    for a in [out["table"], out["ids"], out["e"], out["m"], out["r"]] + out["grads"]:
        a.setflags(write=False)
    return out


def start_state(rule, p):
    """The rule's state tensors (optimizer_bits_reference.STATE) at the start, as uint32 patterns."""
    return {"sgd": [], "adagrad": [p["e"]], "rowwise_adagrad": [p["r"]], "adam": [p["m"], p["e"]],
            "rowwise_adam": [p["m"], p["r"]]}[rule]


def variants(rule, kind, width):
    """(eps, weight_decay, shift) of every run of one parametrised case."""
    out = []
    for shift in (0,) + (SHIFTS if width in SHIFTED_WIDTHS else ()):
        for eps in EPSILONS:
            out += [(eps, wd, shift) for wd in WEIGHT_DECAYS[rule]]
    return out


def model_steps(rule, kind, width, rounding, eps, weight_decay, lane):
    """[(table, state, trace) after step 1, after step 2] from the model."""
    p = edge_problem(kind, width)
    table, state, out = p["table"], start_state(rule, p), []
    for t, g in zip(STEPS, p["grads"]):
        table, state, trace = B.step(rule, kind, table, state, p["ids"], g, B.valid_entries(N), lr=LR, eps=eps,
                                     bias_factor=AR.bias_factor(t, BETAS), betas=BETAS, weight_decay=weight_decay,
                                     lane=lane, rounding=rounding, seed=SEED, step=t)
        out.append((table, state, trace))
    return out


def edge_conditions(rule, kind, eps, weight_decay, rounding):
    """What the model's results on the NAMED rows must contain (test_optimizer_bits_host.py asserts it per case, over
    the two steps).  Everything the issue of this test lists, except where the arithmetic cannot reach it:

      * -0 in the table under the Adam rules with weight_decay != 0 on an fp32 table: w + -(decay * w) is +0 for w = -0,
        and a sum is -0 only if both terms are; a 16-bit table still gets -0 from a store that underflows;
      * a finite fp32 value that the 16-bit store rounds to infinity under Adagrad and row-wise Adagrad: they move a
        weight by at most lr (row-wise: lr * sqrt(W) < 0.5) per step, and from +-65504 the store needs 16, from +-max
        bf16 2^119;
      * subnormal and infinite state under SGD, which has none.
    Ties at the store are required where they can be built: SGD and Adagrad on a 16-bit table, rounded to nearest."""
    adam = rule in ("adam", "rowwise_adam")
    need = {"subnormal table", "+0", "-0", "+inf", "-inf", "nan"}
    if adam and weight_decay != 0 and kind == "f32":
        need.discard("-0")
    if rule != "sgd":
        need |= {"subnormal state", "infinite state"}
    if kind != "f32" and rule in ("sgd", "adam", "rowwise_adam"):
        need.add("store overflow")
    if kind != "f32" and rule in ("sgd", "adagrad") and rounding == "nearest":
        need.add("tie")
    return need


def edge_findings(kind, named, steps):
    """The set of conditions that the model's results (model_steps) show on the named rows."""
    ebits, mbits = FORMAT[kind]
    found = set()
    for table, state, trace in steps:
        t = table[named].astype(np.int64)
        exponent, mantissa, sign = (t >> mbits) & ((1 << ebits) - 1), t & ((1 << mbits) - 1), t >> (ebits + mbits)
        top = (1 << ebits) - 1
        checks = {"subnormal table": (exponent == 0) & (mantissa != 0), "+0": t == 0, "-0": (exponent == 0) & (mantissa == 0) & (sign == 1),
                  "+inf": (exponent == top) & (mantissa == 0) & (sign == 0), "-inf": (exponent == top) & (mantissa == 0) & (sign == 1),
                  "nan": (exponent == top) & (mantissa != 0)}
        x = trace["x"]
        order = np.argsort(trace["rows"])
        assert np.array_equal(trace["rows"][order], named)
        checks["store overflow"] = np.isfinite(x[order]) & (exponent == top) & (mantissa == 0)
        if kind != "f32":
            checks["tie"] = (x.view(np.uint32) & 0xFFFF == 0x8000) if kind == "bf16" else \
                ((x.view(np.uint32) & 0x1FFF == 0x1000) & (np.abs(x) >= 2.0 ** -14) & (np.abs(x) < 65504))
        for s in state:
            f = B.f32(s[named])
            checks["subnormal state"] = checks.get("subnormal state", False) | bool(((f != 0) & (np.abs(f) < 2.0 ** -126)).any())
            checks["infinite state"] = checks.get("infinite state", False) | bool(np.isinf(f).any())
        found |= {name for name, hit in checks.items() if np.any(hit)}
    return found


def small_cases():
    out = []
    for kind, widths in WIDTHS.items():
        for width in widths:
            for index in ("i32", "i64") if width == 64 else ("i32",):
                out += [(kind, width, index, rounding) for rounding in ROUNDINGS[kind]]
    return out


@pytest.fixture(scope="module")
def ce():
    import cuembed_amd
    assert torch.cuda.is_available()
    return cuembed_amd


def on_device(bits, kind):
    """Bit patterns -> a device tensor of the table's type (or, kind=None, fp32 state)."""
    a = np.array(bits, copy=True)                # (the problem's arrays are read-only)
    t = torch.from_numpy(a.view(np.int16 if a.dtype.itemsize == 2 else np.int32)).cuda()
    return t.view(torch.float32 if kind is None else TORCH[kind])


def device_bits(t):
    t = t.detach().contiguous()
    wide = t.element_size() == 4
    return t.view(torch.int32 if wide else torch.int16).cpu().numpy().view(np.uint32 if wide else np.uint16)


def assert_same(got, want, is_nan, label):
    """got / want: bit patterns; is_nan: the test of the patterns' type."""
    by_class = is_nan(want)
    assert is_nan(got)[by_class].all(), "%s: the model has NaNs where the device has none" % (label,)
    differs = (got != want) & ~by_class
    if differs.any():
        at = tuple(int(i) for i in np.argwhere(differs)[0])
        raise AssertionError("%s: %d elements differ, the first at %r: device %#x, model %#x" % (
            label, int(differs.sum()), at, int(got[at]), int(want[at])))
    return int((~by_class).sum()), int(by_class.sum())


def nan_test(kind):
    ebits, mbits = FORMAT[kind]
    return lambda bits: (np.asarray(bits).astype(np.int64) & ((1 << (ebits + mbits)) - 1)) > (((1 << ebits) - 1) << mbits)


@pytest.mark.parametrize("kind,width,index,rounding", small_cases())
@pytest.mark.parametrize("rule", RULES)
def test_two_steps_on_edge_data_equal_the_model(ce, rule, kind, width, index, rounding):
    p = edge_problem(kind, width)
    ids = torch.from_numpy(p["ids"].copy()).to(INDEX[index]).cuda()
    size = B.ELEM_SIZE[kind]
    for eps, weight_decay, shift in variants(rule, kind, width):
        table, table_ok = shifted(on_device(p["table"], kind), shift)
        state = [on_device(s, None) for s in start_state(rule, p)]
        lane = None
        for n, (t, g) in enumerate(zip(STEPS, p["grads"])):
            rows, rows_ok = shifted(on_device(g, kind), shift)
            if lane is None:
                lane = lane_bytes(size, width, table.data_ptr(), rows.data_ptr())
                assert lane == B.lane_bytes(kind, width, shift)
                want = model_steps(rule, kind, width, rounding, eps, weight_decay, lane)
            assert lane_bytes(size, width, table.data_ptr(), rows.data_ptr()) == lane
            kw = dict(count=N)
            if rounding == "stochastic":
                kw.update(stochastic_rounding=True, seed=SEED, step=t)
            if rule in ("adam", "rowwise_adam"):
                ce.sparse_row_adam(table, ids, rows, exp_avg=state[0], exp_avg_sq=state[1], lr=LR,
                                   bias_factor=AR.bias_factor(t, BETAS), betas=BETAS, eps=eps, weight_decay=weight_decay,
                                   rowwise=rule == "rowwise_adam", **kw)
            else:
                ce.sparse_row_update(table, ids, rows, rule=rule, lr=LR, state=state[0] if state else None, eps=eps, **kw)
            label = (rule, kind, width, index, rounding, "eps=%g" % eps, "wd=%g" % weight_decay, "shift=%d" % shift, "step %d" % t)
            assert_same(device_bits(table), want[n][0], nan_test(kind), label + ("table",))
            for which, (got, model) in enumerate(zip(state, want[n][1])):
                assert_same(device_bits(got), model, nan_test("f32"), label + ("state %d" % which,))
            assert np.array_equal(device_bits(rows), g)
            rows_ok()
        table_ok()
