"""GPU (-m gpu): the C++ drop-in with queries noted as segments of reads (Convex::DeviceReads) against the same tiles with
host-built strings (tests/cpp/segments_shim_test.cpp): a noted launch through cvx_submit_segments, a mixed launch that is
materialised on the host and counted, DeviceReads::Materialise -- on one logical device and on two (CVX_ALIAS_DEVICES=2)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "ngmlr_amd", "segments_shim_test")


@pytest.mark.gpu
@pytest.mark.parametrize("alias", [1, 2])
def test_noted_queries_equal_host_built_strings(built, alias):
    assert os.path.exists(EXE), "ngmlr_amd/segments_shim_test not built (make -C ngmlr_amd/csrc shim_test)"
    env = dict(os.environ)
    env.pop("CVX_ALIAS_DEVICES", None)
    env.pop("CVX_DEVICE_READS", None)
    if alias > 1:
        env["CVX_ALIAS_DEVICES"] = str(alias)
    r = subprocess.run([EXE], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "segments_shim_test: ok" in r.stdout
    assert r.stdout.count(" tiles over ") == alias and "device %d of %d" % (alias - 1, alias) in r.stdout
