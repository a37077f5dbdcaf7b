"""Runs the C++ known-answer program of stochastic rounding in the grouped optimizer step
(tests/cpp/grouped_stochastic_rounding_kat.hip), built against the HEADER-ONLY API: cuembed::SparseRowUpdateGrouped (SGD,
the step as an immediate) and cuembed::SparseRowAdamGrouped (row-wise Adam, the step in a device word) with one seed per
table on a group of three separate tables, fp16 and bf16, against a host recomputation with stochastic_rounding.hpp's own
host functions called with (seeds[t], step, row inside table t, column)."""
import subprocess

import pytest

pytestmark = pytest.mark.gpu


def test_grouped_stochastic_rounding_against_the_host_functions():
    from cuembed_amd import build
    exe = build.build_grouped_stochastic_rounding_test()
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout
    assert "grouped stochastic rounding: all 44 known-answer checks passed" in r.stdout
    assert r.stdout.count(": done") == 4 and "FAILED" not in r.stdout
