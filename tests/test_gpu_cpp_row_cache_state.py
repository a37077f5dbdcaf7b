"""Runs the C++ known-answer program of the row cache's state plane (tests/cpp/row_cache_state_kat.hip), built against
the HEADER-ONLY API: one cuembed::RowCachePrefetch with a state plane, one cuembed::SparseRowUpdate with state_ids and
one cuembed::RowCacheFlush, for both Adagrad rules, against a host recomputation."""
import subprocess

import pytest

pytestmark = pytest.mark.gpu


def test_row_cache_state_known_answers():
    from cuembed_amd import build
    exe = build.build_row_cache_state_test()
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout
    assert "known-answer checks passed" in r.stdout
