"""Runs the C++ known-answer program of the row cache's two state planes (tests/cpp/row_cache_adam_kat.hip), built
against the HEADER-ONLY API: one cuembed::RowCachePrefetch with two planes, one cuembed::TranslateIndicesForRowCachePlanes,
one cuembed::SparseRowAdam with placed moments and one cuembed::RowCacheFlush, for both Adam rules, against a host
recomputation."""
import subprocess

import pytest

pytestmark = pytest.mark.gpu


def test_row_cache_adam_known_answers():
    from cuembed_amd import build
    exe = build.build_row_cache_adam_test()
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout
    assert "known-answer checks passed" in r.stdout
