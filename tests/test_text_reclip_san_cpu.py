"""CPU: cvx_text_reclip's helper (cvx::text_reclip, ngmlr_amd/csrc/cvx_job_text_logic.h) as a program of its own -- its own main, host code
only, never loaded into Python -- built with plain g++ and again under -fsanitize=address,undefined: hand-written records with own
clips of 0 to 100 000 and external clips up to 2 000 000 000, default and scalar-twin op counts, and every output capacity from 0
over the exact length to beyond it, each buffer allocated at exactly that capacity (tests/cpp/text_reclip_test.cpp)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_text_reclip(tmp_path, sanitize):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "text_reclip_test"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else []
    subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror"] + flags +
                   ["-I" + os.path.join(ROOT, "ngmlr_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "text_reclip_test.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "text_reclip_test: ok" in r.stdout
