"""CPU: the host half of scoring against the resident genome (ngmlr_amd/csrc/cvx_score_windows.h: closed-form string lengths,
classes, slot order, arena offsets, the host-built strings) through tests/cpp/score_windows_logic_test.cpp, built with plain g++ and
nothing of HIP -- once as it is and once with -fsanitize=address,undefined.  The program has its own main and runs on the host only."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan-ubsan"])
def test_score_windows_logic(tmp_path, sanitize):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "score_windows_logic_test"
    flags = ["-O1", "-g", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "ngmlr_amd", "csrc")]      # no HIP
    if sanitize:
        flags += ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
        if os.path.exists(os.path.join(ROCM, "include", "hip", "hip_runtime.h")):
            # this build also holds the class rule's rows against score_wave_rows of cvx_score_wave.h, which includes the HIP runtime's header
            flags += ["-DCVX_WITH_SCORE_WAVE_H", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include")]
    subprocess.run([gxx] + flags + [os.path.join(ROOT, "tests", "cpp", "score_windows_logic_test.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "score_windows_logic_test: ok" in r.stdout
