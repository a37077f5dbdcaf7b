"""Runs the C++ known-answer program of the sparse Adam step (tests/cpp/sparse_adam_kat.hip), built against the
HEADER-ONLY API: cuembed::SparseRowAdam for both rules, every element and index type and every source of the entry
count, and cuembed::AdamClockAdvance."""
import subprocess

import pytest

pytestmark = pytest.mark.gpu


def test_sparse_adam_known_answers():
    from cuembed_amd import build
    exe = build.build_sparse_adam_test()
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout
    assert "known-answer checks passed" in r.stdout
