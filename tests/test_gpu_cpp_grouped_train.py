"""Runs the C++ known-answer program of a group's weight gradient and mean scale (tests/cpp/grouped_train_kat.hip), built
against the HEADER-ONLY API: cuembed::EmbeddingWeightGradGrouped and cuembed::GroupedMeanScale on a three-table group,
CSR and fixed hotness, fp32 and fp16, against a host recomputation on exact data."""
import subprocess

import pytest

pytestmark = pytest.mark.gpu


def test_grouped_train_known_answers():
    from cuembed_amd import build
    exe = build.build_grouped_train_test()
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout
    assert "known-answer checks passed" in r.stdout
