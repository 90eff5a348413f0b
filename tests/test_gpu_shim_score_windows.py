"""GPU (-m gpu): StrippedSWHip::BatchScoreWindows, the C++ drop-in's extension for pairs given as windows of the resident genome,
against its own BatchScore on host-built strings (tests/cpp/score_windows_shim_test.cpp) -- on one logical device and on two
(CVX_ALIAS_DEVICES=2: one genome upload per logical device, freed with the device's last scorer)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "ngmlr_amd", "score_windows_shim_test")


@pytest.mark.gpu
@pytest.mark.parametrize("alias", [1, 2])
def test_batch_score_windows_equals_batch_score(built, alias):
    assert os.path.exists(EXE), "ngmlr_amd/score_windows_shim_test not built (make -C ngmlr_amd/csrc shim_test)"
    env = dict(os.environ)
    env.pop("CVX_ALIAS_DEVICES", None)
    if alias > 1:
        env["CVX_ALIAS_DEVICES"] = str(alias)
    r = subprocess.run([EXE], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "score_windows_shim_test: ok" in r.stdout
    assert r.stdout.count(" failed decodes") == alias and "device %d of %d" % (alias - 1, alias) in r.stdout
    # the exit line: one window call per device, three pairs each through the string path
    assert r.stderr.count(" window calls") == alias and "3 through the string path" in r.stderr
