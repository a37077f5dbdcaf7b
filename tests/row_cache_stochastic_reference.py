"""The data of the test that shows, without the library's other path, that stochastic rounding through the row cache
names its bits by the TABLE ROW (tests/test_gpu_row_cache_stochastic.py, test 3), and what a wrong naming would give
(numpy, no GPU; not a test module).  tests/test_row_cache_stochastic_host.py shows on the CPU that this data tells right
from wrong.

A 300-row table of width 136 behind a cache of one set.  A forward on READ, ten rows that are never updated, occupies
ways 0 to 9; the update's ids then miss and take the ways from 10 on in ascending row order (DynamicRowCache's
contract), so the slot of the id of rank k is 10 + k -- slots().  The ids are drawn from [100, 290): no updated row sits
in the slot of its own number, and a walk that drew the bits of the slot (or of a translated id) instead of the table
row would draw another row's."""
import numpy as np

import stochastic_rounding_reference as S

ROWS, WIDTH, ENTRIES, STEPS = 300, 136, 37, 3
LR, SEED = 0.0371, 0xC0FFEE1234567
READ = np.arange(290, 300)


def problem(kind):
    """(table patterns [ROWS, WIDTH], ids [ENTRIES] distinct and in no order, gradient patterns per step
    [STEPS, ENTRIES, WIDTH]): standard normal values rounded to the type, so that no update is representable."""
    rng = np.random.default_rng(136 + (kind == "bf16"))
    table = S.nearest(rng.standard_normal((ROWS, WIDTH)).astype(np.float32), kind)
    ids = (100 + rng.permutation(190)[:ENTRIES]).astype(np.int64)
    grads = S.nearest(rng.standard_normal((STEPS, ENTRIES, WIDTH)).astype(np.float32), kind)
    return table, ids, grads


def slots(ids):
    """The way each id takes in the one set once READ holds ways 0 to 9: 10 + its rank among the ids."""
    return 10 + np.argsort(np.argsort(ids))


def trained(kind, seed=SEED, names=None):
    """The table after the STEPS SGD steps: stochastic with the fields of (seed, step, names[k], column) -- names=None:
    the ids themselves, which is the specification -- or, seed=None, to nearest."""
    table, ids, grads = problem(kind)
    for step in range(STEPS):
        if seed is None or names is None:
            table = S.sgd(table, ids, grads[step], LR, kind, seed=seed, step=step)
        else:
            x = S.sgd_value(table[ids], grads[step], LR, kind)
            table = table.copy()
            table[ids] = S.stochastic(x, S.fields(seed, step, names, WIDTH), kind)
    return table
