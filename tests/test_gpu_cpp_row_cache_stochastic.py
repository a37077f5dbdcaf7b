"""Runs the C++ known-answer program of stochastic rounding through the row cache (tests/cpp/row_cache_stochastic_kat.hip),
built against the HEADER-ONLY API: one cuembed::RowCachePrefetch, one cuembed::TranslateIndicesForRowCachePlanes, one
cuembed::SparseRowUpdate / cuembed::SparseRowAdam with row_names and one cuembed::RowCacheFlush, for row-wise Adagrad (one
state plane) and lazy Adam (two) on __half and __hip_bfloat16, against a host recomputation that rounds with
stochastic_rounding.hpp's own host functions and the table row as the name."""
import subprocess

import pytest

pytestmark = pytest.mark.gpu


def test_row_cache_stochastic_known_answers():
    from cuembed_amd import build
    exe = build.build_row_cache_stochastic_test()
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout
    assert "known-answer checks passed" in r.stdout
