"""Runs the C++ known-answer program of the device-side index check (tests/cpp/index_check_kat.hip), built against the
HEADER-ONLY API: cuembed::CheckIndices on a hand-written three-table CSR batch (out of place, then the repaired batch
in place) and a fixed-hotness table, against answers written in the source."""
import subprocess

import pytest

pytestmark = pytest.mark.gpu


def test_index_check_known_answers():
    from cuembed_amd import build
    exe = build.build_index_check_test()
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout
    assert "known-answer checks passed" in r.stdout
