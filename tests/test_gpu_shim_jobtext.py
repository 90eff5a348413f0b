"""GPU (-m gpu): the C++ drop-ins taking a tile's CIGAR and MD from the launch's device-made text (tests/cpp/jobtext_shim_test.cpp):
Convex::ConvexAlignHip::AlignTiles with requests and plain buffers in one launch on an aligner with CVX_CREATE_JOB_TEXT -- every
Align field, both strings, the note and the profile equal the run whose Finish formats every tile on the host, with external
clips, a pBuffer2 too small (regrown) and a CIGAR beyond maxBufferLength (the tile's hard error) -- and the same through
Convex::SharedAligner on one and two logical devices with CVX_JOB_TEXT=1, =0 and the constructor's argument."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "ngmlr_amd", "jobtext_shim_test")


@pytest.mark.parametrize("devices,switch,ctor", [(1, "1", 0), (2, "1", 0), (1, "0", 0), (2, None, 0), (1, None, 1)],
                         ids=["one_device", "two_devices", "switched_off", "default_is_off", "constructor_argument"])
def test_drop_ins_take_their_text_from_the_device(built, devices, switch, ctor):
    assert os.path.exists(EXE), "make -C ngmlr_amd/csrc shim_test builds it"
    env = dict(os.environ)
    for k in ("CVX_DEVICE_REGIONS", "CVX_ALIAS_DEVICES", "CVX_JOB_TEXT", "CVX_DEVICE_TEXT"):
        env.pop(k, None)
    if devices > 1:
        env["CVX_ALIAS_DEVICES"] = str(devices)
    if switch is not None:
        env["CVX_JOB_TEXT"] = switch
    r = subprocess.run([EXE, str(devices), str(ctor)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    on = switch == "1" or ctor
    assert "jobtext_shim_test: ok (%s)" % ("device text" if on else "host form") in r.stdout
    assert "SharedAligner on %d logical device(s)" % devices in r.stdout
    line = [ln for ln in r.stderr.splitlines() if "took their CIGAR and MD from the device" in ln]
    assert len(line) == 1, r.stderr
    # the exit line counts the whole process: the AlignTiles run with the constructor's flag came first
    n_dev = int(line[0].split("SharedAligner: ")[1].split()[0])
    before = int(re.search(r"AlignTiles \(job text\): (\d+) from the device", r.stdout).group(1))
    assert before > 0 and ((n_dev > before) if on else (n_dev == before)), (before, line[0])
