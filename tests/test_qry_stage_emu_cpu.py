"""CPU: stage_segments_kernel's source compiled for the host (tests/cpp/hip_host_stub stands in for the HIP headers, v_perm_b32
emulated) and run lane by lane under -fsanitize=address,undefined against the host-built strings
(tests/cpp/qry_stage_emu_test.cpp).  The program has its own main and is never loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_segments_kernel_lane_by_lane(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "qry_stage_emu_test"
    subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I" + os.path.join(ROOT, "tests", "cpp", "hip_host_stub"), "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "ngmlr_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "qry_stage_emu_test.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "qry_stage_emu_test: ok" in r.stdout
