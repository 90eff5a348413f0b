"""GPU (-m gpu): the C++ drop-ins answering a request in Align::nmPerPosition with a note of the job's regions
(tests/cpp/regions_shim_test.cpp): Convex::ConvexAlignHip::AlignTiles with marked and unmarked buffers in one launch -- the
note's regions equal cvx_nm_regions_host over the profile the same shim writes for the same tile, a buffer too small for its
note is regrown, without the flag a request ends as the full profile -- and the same through Convex::SharedAligner on one and
two logical devices, with the binding announced and with CVX_DEVICE_REGIONS=0."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "ngmlr_amd", "regions_shim_test")


@pytest.mark.parametrize("devices,switch", [(1, None), (2, None), (1, "0")], ids=["one_device", "two_devices", "switched_off"])
def test_drop_ins_answer_a_request_with_a_note(built, devices, switch):
    assert os.path.exists(EXE), "make -C ngmlr_amd/csrc shim_test builds it"
    env = dict(os.environ)
    env.pop("CVX_DEVICE_REGIONS", None)
    env.pop("CVX_ALIAS_DEVICES", None)
    if devices > 1:
        env["CVX_ALIAS_DEVICES"] = str(devices)
    if switch is not None:
        env["CVX_DEVICE_REGIONS"] = switch
    r = subprocess.run([EXE, str(devices)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "regions_shim_test: ok (%s)" % ("profile" if switch == "0" else "regions") in r.stdout
    assert "SharedAligner on %d logical device(s)" % devices in r.stdout
