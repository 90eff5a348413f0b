"""CPU: the runtime's owning buffer (ngmlr_amd/csrc/cvx_buf.h), instantiated over a counting fake memory in tests/cpp/buf_test.cpp:
the capacity every growth reaches against the rule as DevBuf::ensure and PinBuf::ensure stated it (old capacity x request x
high-water mark, both slack constants), the one drain-and-retry when the generous size does not fit, the failure that neither
drains nor retries, and ownership -- growth parks the old block, scope exit and move assignment free exactly once, allocations
equal frees plus parked blocks.  Built with plain g++ under -fsanitize=address,undefined; the program has its own main and is
never loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_buf(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "buf_test"
    subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "ngmlr_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "buf_test.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "buf_test: ok" in r.stdout
