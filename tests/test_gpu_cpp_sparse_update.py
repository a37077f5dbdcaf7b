"""Runs the C++ known-answer program of the sparse optimizer step (tests/cpp/sparse_update_kat.hip), built against the
HEADER-ONLY API: cuembed::SparseRowUpdate for every rule, element and index type and every source of the entry count."""
import subprocess

import pytest

pytestmark = pytest.mark.gpu


def test_sparse_update_known_answers():
    from cuembed_amd import build
    exe = build.build_sparse_update_test()
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout
    assert "known-answer checks passed" in r.stdout
