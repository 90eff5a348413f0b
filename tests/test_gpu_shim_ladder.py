"""GPU (-m gpu): the C++ drop-in's AlignLadders -- one device job that climbs computeAlignment's corridor retry ladder -- against
SingleAlign called rung by rung on host-built corridors (tests/cpp/ladder_shim_test.cpp)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "ngmlr_amd", "ladder_shim_test")


@pytest.mark.gpu
def test_align_ladders_equals_single_align_rung_by_rung(built):
    assert os.path.exists(EXE), "ngmlr_amd/ladder_shim_test not built (make -C ngmlr_amd/csrc shim_test)"
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ladder_shim_test: ok" in r.stdout
