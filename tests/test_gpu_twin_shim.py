"""GPU (-m gpu): the C++ drop-ins in scalar-twin mode (tests/cpp/twin_shim_test.cpp): Convex::ConvexAlignHip and
Convex::SharedAligner constructed in twin mode leave Align::svType and Align::cigarOpCount exactly as the caller passed them;
in default mode they are 0 and the op count."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "ngmlr_amd", "twin_shim_test")


@pytest.mark.parametrize("mode", ["twin", "default"])
def test_drop_ins_leave_sv_type_and_op_count_alone_in_twin_mode(built, mode):
    assert os.path.exists(EXE), "make -C ngmlr_amd/csrc shim_test builds it"
    r = subprocess.run([EXE, mode], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "twin_shim_test: ok" in r.stdout
    assert "svType 1234 cigarOpCount 77" in r.stdout
