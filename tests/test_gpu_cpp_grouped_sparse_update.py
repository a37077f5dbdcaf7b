"""Runs the C++ program of the grouped optimizer step (tests/cpp/grouped_sparse_update_kat.hip), built against the
HEADER-ONLY API: cuembed::SparseRowUpdateGrouped / SparseRowAdamGrouped on a group of separate tables with 1, 5 and 70
rows against cuembed::SparseRowUpdate / SparseRowAdam per table inside the same program, bit for bit, for all five rules."""
import subprocess

import pytest

pytestmark = pytest.mark.gpu


def test_grouped_sparse_update_against_the_per_table_calls():
    from cuembed_amd import build
    exe = build.build_grouped_sparse_update_test()
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout
    assert "all grouped sparse update known-answer checks passed" in r.stdout
    assert r.stdout.count(": ok") == 20 and "MISMATCH" not in r.stdout
