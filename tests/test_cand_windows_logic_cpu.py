"""CPU: plan_candidate_windows_kernel's source (ngmlr_amd/csrc/cvx_score_cands.hip) compiled for the host over tests/cpp/hip_host_stub
and run thread by thread under -fsanitize=address,undefined against score_windows_plan on the pairs the two-call path builds
(tests/cpp/cand_windows_logic_test.cpp).  The program has its own main and is never loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_kernel_thread_by_thread(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "cand_windows_logic_test"
    subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I" + os.path.join(ROOT, "tests", "cpp", "hip_host_stub"), "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "ngmlr_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "cand_windows_logic_test.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cand_windows_logic_test: ok" in r.stdout
