"""GPU (-m gpu): CandidateSearchHip::SearchAndScore, the C++ drop-in's search and score in one device call, against its own Search
followed by StrippedSWHip::BatchScoreWindows on pairs built from the lists (tests/cpp/search_score_shim_test.cpp) -- on one logical
device and on two (CVX_ALIAS_DEVICES=2).  The searcher and the scorers of a device share one resident genome: uploaded once per
logical device, counted by the shared holder (Convex::DeviceGenome::Uploads)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "ngmlr_amd", "search_score_shim_test")


@pytest.mark.gpu
@pytest.mark.parametrize("alias", [1, 2])
def test_search_and_score_equals_search_then_score_windows(built, alias):
    assert os.path.exists(EXE), "ngmlr_amd/search_score_shim_test not built (make -C ngmlr_amd/csrc shim_test)"
    env = dict(os.environ)
    env.pop("CVX_ALIAS_DEVICES", None)
    if alias > 1:
        env["CVX_ALIAS_DEVICES"] = str(alias)
    r = subprocess.run([EXE], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "search_score_shim_test: ok" in r.stdout
    assert r.stdout.count(", 1 genome uploads") == alias and "device %d: " % (alias - 1) in r.stdout
    # the exit lines: every device's searcher scored in its search call, every device's scorer made its one window call
    assert "%d of the search calls scored their candidates in the same call" % alias in r.stderr
    assert r.stderr.count(" window calls") == alias
