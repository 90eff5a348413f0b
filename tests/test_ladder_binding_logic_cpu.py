"""CPU: the rules ladder_binding.inc keeps when it hands computeAlignment's retry loop over as one request
(ngmlr_amd/csrc/ladder_binding_logic.h) as a program of its own -- its own main, host code only, never loaded into Python -- built
with plain g++ and again under -fsanitize=address,undefined: cvx_ladder's left / right bit for bit against a restatement of
getCorridorEndpointsWithAnchors' loop with every operation rounded once (no anchor, one on the line, far left and far right,
reverse strand, refLen != qryLen, a random sweep), acceptance and the counters against the reference's loop for attempts 1 .. 5 x
{last valid, last failed, an alignment of another length} (tests/cpp/ladder_binding_logic_test.cpp)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_ladder_binding_logic(tmp_path, sanitize):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "ladder_binding_logic_test"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else []
    subprocess.run([gxx, "-O1", "-g", "-std=c++11", "-ffp-contract=off", "-Wall", "-Werror"] + flags +
                   ["-I" + os.path.join(ROOT, "ngmlr_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "ladder_binding_logic_test.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ladder_binding_logic_test: ok" in r.stdout
