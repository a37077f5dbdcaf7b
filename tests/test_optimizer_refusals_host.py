"""Which misuse of the twelve optimizer entry points of the C ABI aborts, and which call with nothing to do returns.

Every check in question runs on the host before the first HIP call (CurrentDeviceShape() inside DispatchUpdate), so the
table below needs no GPU: one child process per row loads libcuembed_amd.so with ctypes alone, with the GPU hidden from it
(HIP_VISIBLE_DEVICES=-1), and makes one call.  The parent asserts one of two outcomes:

  * refused: nonzero exit, "Check failed" on stderr, and in the failed condition a keyword that names the offending
    argument;
  * returns: exit status 0 and empty stderr.

Rows that must get past `table != nullptr` carry made-up addresses.  They are never dereferenced: the check under test
precedes every launch, and a check that stopped firing would end in a launch without a device, which fails and leaves
the row as a failed test.  The grouped entry points read their host pointer arrays, so those are real host memory (kind
"h" below) that holds made-up addresses.
"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "cuembed_amd", "lib", "libcuembed_amd.so")

# ---- the twelve signatures (include/cuembed_amd.h): "name:kind", kinds p = pointer, h = host array of pointers,
# i = int, l = int64_t, f = float, u = uint64_t
_COUNT = "piece_rows:l pieces:i num_rows:l counts:p counts64:i last_id:p lr:f lr_device:p"
_GROUP = ("num_tables:i elem:i width:i row_base:p rule:i ids:p idx:i rows:p total_entries:l num_rows:l counts:p "
          "counts64:i last_id:p lr:f lr_device:p")
_MOMENTS = "bias:f bias_device:p beta1:f omb1:f beta2:f omb2:f eps:f weight_decay:f"
_UPDATE = "table:p elem:i width:i state:p rule:i ids:p idx:i rows:p " + _COUNT + " eps:f"
_ADAM = "table:p elem:i width:i exp_avg:p exp_avg_sq:p rule:i ids:p idx:i rows:p " + _COUNT + " " + _MOMENTS
_UPDATE_GROUPED = "tables_host:h tables_device:p state_host:h state_device:p " + _GROUP + " eps:f"
_ADAM_GROUPED = ("tables_host:h tables_device:p exp_avg_host:h exp_avg_device:p exp_avg_sq_host:h exp_avg_sq_device:p " +
                 _GROUP + " " + _MOMENTS)
_ROUNDING = " seed:u step:u step_device:p"
SIGNATURES = {
    "update": _UPDATE + " stream:p",
    "update_placed": _UPDATE + " stream:p state_ids:p",
    "update_stochastic": _UPDATE + _ROUNDING + " stream:p",
    "update_placed_stochastic": _UPDATE + _ROUNDING + " stream:p state_ids:p row_names:p",
    "adam": _ADAM + " stream:p",
    "adam_placed": _ADAM + " stream:p exp_avg_ids:p exp_avg_sq_ids:p",
    "adam_stochastic": _ADAM + _ROUNDING + " stream:p",
    "adam_placed_stochastic": _ADAM + _ROUNDING + " stream:p exp_avg_ids:p exp_avg_sq_ids:p row_names:p",
    "update_grouped": _UPDATE_GROUPED + " stream:p",
    "update_grouped_stochastic": _UPDATE_GROUPED + " seeds:p step:u step_device:p stream:p",
    "adam_grouped": _ADAM_GROUPED + " stream:p",
    "adam_grouped_stochastic": _ADAM_GROUPED + " seeds:p step:u step_device:p stream:p",
}
ALL = list(SIGNATURES)
SINGLE = [f for f in ALL if "grouped" not in f]
GROUPED = [f for f in ALL if "grouped" in f]
STOCHASTIC = [f for f in ALL if "stochastic" in f]
ADAMS = [f for f in ALL if f.startswith("adam")]

F32, F16 = 0, 1
SGD, ADAGRAD, ROWWISE_ADAGRAD = 0, 1, 2
# made-up device addresses (16-byte aligned), never dereferenced
TABLE, IDS, ROWS, STATE, STATE2, WORD, NAMES, IDS1, IDS2, SEEDS, BASE, TABLES = (0x1000 * k for k in range(1, 13))


def defaults(fn):
    """A valid call with nothing to do: a 16-bit table of width 8, rule code 0, a host-known count of 0 entries."""
    d = dict(elem=F16, width=8, pieces=1, num_rows=0, num_tables=1, lr=0.1, bias=1.0, beta1=0.9, omb1=0.1, beta2=0.999,
             omb2=0.001, eps=1e-8)
    if fn in GROUPED:
        d.update(tables_host=[TABLE], tables_device=TABLES, row_base=BASE)
        if fn in ADAMS:
            d.update(exp_avg_device=STATE, exp_avg_sq_device=STATE2)
        if fn in STOCHASTIC:
            d.update(seeds=SEEDS)
    if fn.endswith("placed_stochastic"):
        d.update(row_names=NAMES)
        if fn in ADAMS:
            d.update(exp_avg_ids=IDS1, exp_avg_sq_ids=IDS2)
    return d


WORK = dict(piece_rows=8, num_rows=8)                                 # single table: 8 valid entries, all pointers null
BUFFERS = dict(WORK, table=TABLE, ids=IDS, rows=ROWS)                 # ... with made-up buffers
GROUPED_WORK = dict(total_entries=8, num_rows=8, ids=IDS, rows=ROWS)
PLACED_MOMENTS = dict(exp_avg_ids=IDS1, exp_avg_sq_ids=IDS2)

ROWS_OF_TABLE = []    # (id, function, overrides of defaults(function), keyword of the failed condition or None: returns)


def row(name, fn, keyword, **overrides):
    ROWS_OF_TABLE.append(("%s-%s" % (fn, name), fn, overrides, keyword))


for fn in ALL:
    row("nothing_to_do", fn, None)
    row("no_count_source", fn, "sources", num_rows=-1)
    row("two_count_sources", fn, "sources", last_id=WORD)
    row("unknown_rule", fn, "unknown Adam rule" if fn in ADAMS else "unknown update rule", rule=7)
    row("bad_element_code", fn, "unsupported type code", elem=3)
    row("bad_index_code", fn, "unsupported type code", idx=7)
    row("count_above_capacity", fn, "num_rows", num_rows=1)
for fn in SINGLE:
    row("pieces_without_counts", fn, "pieces", pieces=2)
    row("no_pieces", fn, "pieces", pieces=0)
    row("negative_capacity", fn, "piece_rows", piece_rows=-1, num_rows=-1, last_id=WORD)
    row("work_without_buffers", fn, "table", **WORK)
for fn in GROUPED:
    row("negative_capacity", fn, "total_entries", total_entries=-1)
    row("host_count_zero", fn, None, total_entries=8)
    row("no_tables", fn, "num_tables", num_tables=0)
    row("too_many_tables", fn, "num_tables", num_tables=1024)
    row("null_tables_host", fn, "tables_host", tables_host=None)
    row("null_tables_device", fn, "tables_device", tables_device=None)
    row("null_row_base", fn, "row_base", row_base=None)
    row("work_without_ids", fn, "ids", **dict(GROUPED_WORK, ids=None))
    row("work_with_a_null_table", fn, "tables_host", **dict(GROUPED_WORK, tables_host=[0]))
for fn in STOCHASTIC:
    row("float_table", fn, "unsupported type code", elem=F32)

# update, plain and placed (state_ids == NULL forwards) and stochastic: the state check precedes the work check
for fn in ("update", "update_placed", "update_stochastic"):
    for work, extra in (("", {}), ("_with_work", WORK)):
        row("sgd_with_state" + work, fn, "state", state=STATE, **extra)
        row("adagrad_without_state" + work, fn, "state", rule=ADAGRAD, **extra)
        row("rowwise_adagrad_without_state" + work, fn, "state", rule=ROWWISE_ADAGRAD, **extra)
    row("adagrad_nothing_to_do", fn, None, rule=ADAGRAD, state=STATE)
row("state_ids_with_sgd", "update_placed", "kSgd", state_ids=IDS1)
row("state_ids_without_state", "update_placed", "state", rule=ADAGRAD, state_ids=IDS1)
row("state_ids_nothing_to_do", "update_placed", None, rule=ADAGRAD, state=STATE, state_ids=IDS1)
row("state_ids_work_without_buffers", "update_placed", "table", rule=ADAGRAD, state=STATE, state_ids=IDS1, **WORK)

row("null_row_names", "update_placed_stochastic", "row_names", row_names=None)
row("sgd_with_state_ids", "update_placed_stochastic", "state_ids", state_ids=IDS1)
row("sgd_with_state", "update_placed_stochastic", "state", state=STATE)
row("adagrad_without_state_ids", "update_placed_stochastic", "state_ids", rule=ADAGRAD, state=STATE)
row("adagrad_without_state", "update_placed_stochastic", "state", rule=ADAGRAD, state_ids=IDS1)
row("adagrad_nothing_to_do", "update_placed_stochastic", None, rule=ADAGRAD, state=STATE, state_ids=IDS1)

# what UpdateLaneBytes refuses, past `table != nullptr`
for fn in ("update", "update_stochastic", "adam"):
    moments = dict(exp_avg=STATE, exp_avg_sq=STATE2) if fn in ADAMS else {}
    row("row_of_2_bytes", fn, "row_bytes", **dict(BUFFERS, width=1, **moments))
    row("no_width", fn, "embed_width", **dict(BUFFERS, width=0, **moments))
    row("table_at_4k_plus_2", fn, "table", **dict(BUFFERS, table=TABLE + 2, **moments))
row("state_at_8k_plus_4", "update", "state", **dict(BUFFERS, rule=ADAGRAD, state=STATE + 4))
row("exp_avg_at_8k_plus_4", "adam", "state", **dict(BUFFERS, exp_avg=STATE + 4, exp_avg_sq=STATE2))

# Adam: hyper-parameters first, the moments only where there is work
for fn in ADAMS:
    placed = PLACED_MOMENTS if fn == "adam_placed" else {}
    row("beta1_is_1", fn, "beta1", beta1=1.0, **placed)
    row("negative_beta2", fn, "beta2", beta2=-0.125, **placed)
    row("negative_eps", fn, "eps", eps=-1e-8, **placed)
    row("negative_weight_decay", fn, "weight_decay", weight_decay=-0.125, **placed)
    if fn == "adam_placed":
        row("placed_nothing_to_do", fn, None, **placed)
    if fn in SINGLE:
        row("work_without_exp_avg", fn, "exp_avg", **dict(BUFFERS, exp_avg_sq=STATE2, **placed))
        row("work_without_exp_avg_sq", fn, "exp_avg_sq", **dict(BUFFERS, exp_avg=STATE, **placed))
        row("exp_avg_sq_at_4k_plus_2", fn, "exp_avg_sq", **dict(BUFFERS, exp_avg=STATE, exp_avg_sq=STATE2 + 2, **placed))
row("exp_avg_ids_alone", "adam_placed", "exp_avg_sq_ids", exp_avg_ids=IDS1)
row("exp_avg_sq_ids_alone", "adam_placed", "exp_avg_ids", exp_avg_sq_ids=IDS2)
row("null_row_names", "adam_placed_stochastic", "row_names", row_names=None)
row("without_exp_avg_ids", "adam_placed_stochastic", "exp_avg_ids", exp_avg_ids=None)
row("without_exp_avg_sq_ids", "adam_placed_stochastic", "exp_avg_sq_ids", exp_avg_sq_ids=None)

# grouped: the state is refused even with zero entries; the host copies only where they are read
for fn in ("update_grouped", "update_grouped_stochastic"):
    row("sgd_with_state", fn, "state_device", state_device=STATE)
    row("adagrad_without_state", fn, "state_device", rule=ADAGRAD)
    row("adagrad_nothing_to_do", fn, None, rule=ADAGRAD, state_device=STATE)
    row("adagrad_without_host_state", fn, "state_host", **dict(GROUPED_WORK, rule=ADAGRAD, state_device=STATE))
for fn in ("adam_grouped", "adam_grouped_stochastic"):
    row("without_exp_avg", fn, "exp_avg_device", exp_avg_device=None)
    row("without_exp_avg_sq", fn, "exp_avg_sq_device", exp_avg_sq_device=None)
    row("without_host_exp_avg", fn, "state_host", **GROUPED_WORK)
for fn in ("update_grouped_stochastic", "adam_grouped_stochastic"):
    row("without_seeds", fn, "seeds", seeds=None)

CHILD = """
import ctypes, sys
KINDS = dict(p=ctypes.c_void_p, h=ctypes.c_void_p, i=ctypes.c_int, l=ctypes.c_int64, f=ctypes.c_float, u=ctypes.c_uint64)
lib, name, kinds, values = %r, %r, %r, %r
call = getattr(ctypes.CDLL(lib), name)
call.restype = None
call.argtypes = [KINDS[k] for k in kinds]
arrays = [None if v is None else (ctypes.c_void_p * len(v))(*v) for k, v in zip(kinds, values) if k == "h"]
held = iter(arrays)
args = []
for k, v in zip(kinds, values):
    if k == "h":
        a = next(held)
        v = None if a is None else ctypes.cast(a, ctypes.c_void_p)
    args.append(v)
call(*args)
"""


def run_row(entry):
    _, fn, overrides, _ = entry
    fields = [f.split(":") for f in SIGNATURES[fn].split()]
    values = dict(defaults(fn))
    unknown = set(overrides) - {n for n, _ in fields}
    assert not unknown, (fn, unknown)
    values.update(overrides)
    kinds = [k for _, k in fields]
    args = [values.get(n, None if k in "ph" else 0) for n, k in fields]
    code = CHILD % (LIB, "cuembed_sparse_row_" + fn, kinds, args)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    return subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env)


@pytest.fixture(scope="module")
def outcomes():
    """Every row's child, run once, several at a time."""
    with ThreadPoolExecutor(max_workers=8) as pool:
        return dict(zip([e[0] for e in ROWS_OF_TABLE], pool.map(run_row, ROWS_OF_TABLE)))


def test_the_table_names_every_entry_point_once():
    assert len({e[0] for e in ROWS_OF_TABLE}) == len(ROWS_OF_TABLE)
    assert {e[1] for e in ROWS_OF_TABLE} == set(ALL) and len(ALL) == 12


@pytest.mark.parametrize("entry", ROWS_OF_TABLE, ids=[e[0] for e in ROWS_OF_TABLE])
def test_optimizer_entry_point_refuses_or_returns(outcomes, entry):
    name, _, _, keyword = entry
    r = outcomes[name]
    if keyword is None:
        assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr)
        return
    assert r.returncode != 0 and "Check failed: " in r.stderr, (r.returncode, r.stderr)
    condition = r.stderr.split("Check failed: ", 1)[1].rsplit(" at ", 1)[0]    # (without the file name and line)
    assert keyword in condition, (keyword, condition)
