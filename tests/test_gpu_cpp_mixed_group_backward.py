"""Runs the C++ known-answer program of the mixed-width grouped backward (tests/cpp/mixed_group_backward_kat.hip), built
against the HEADER-ONLY API: cuembed::GroupedBackwardKeys, cuembed::Transpose, cuembed::EmbeddingBackwardMixedGroup and
cuembed::MixedGroupMeanScale on a hand-written three-table group of widths 4, 8 and 2, against answers written in the
source; sentinel-filled outputs (rows past the count untouched) and the capacity check (nothing written, word raised)."""
import subprocess

import pytest

pytestmark = pytest.mark.gpu


def test_mixed_group_backward_known_answers():
    from cuembed_amd import build
    exe = build.build_mixed_group_backward_test()
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout
    assert "known-answer checks passed" in r.stdout
