"""Runs the C++ known-answer program of stochastic rounding in the sparse optimizer step
(tests/cpp/stochastic_rounding_kat.hip), built against the HEADER-ONLY API: cuembed::SparseRowUpdate with
options.stochastic_rounding for both 16-bit table types, both index types, every lane width and body."""
import subprocess

import pytest

pytestmark = pytest.mark.gpu


def test_stochastic_rounding_known_answers():
    from cuembed_amd import build
    exe = build.build_stochastic_rounding_test()
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout
    assert "known-answer checks passed" in r.stdout
