"""Runs the C++ known-answer program of the mixed-width grouped forward (tests/cpp/mixed_group_kat.hip), built against
the HEADER-ONLY API: cuembed::EmbeddingForwardMixedGroup on a hand-written three-table group of widths 4, 8 and 2 (CSR
with an empty bag, sum and weighted mean; then fixed hotness), against answers written in the source."""
import subprocess

import pytest

pytestmark = pytest.mark.gpu


def test_mixed_group_known_answers():
    from cuembed_amd import build
    exe = build.build_mixed_group_test()
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout
    assert "known-answer checks passed" in r.stdout
