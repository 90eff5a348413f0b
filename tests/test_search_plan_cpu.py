"""CPU: the host half of the candidate search (ngmlr_amd/csrc/cvx_search_plan.h) -- the knobs of a call, its staging and read
layouts, map sizes and candidate slots, the retry ladder, an attempt's launches by map size, the table budgets, the regions and
the dense offsets -- compiled with plain g++ over tests/cpp/hip_host_stub and run under -fsanitize=address,undefined against values
written out by hand (tests/cpp/search_plan_test.cpp).  The program has its own main and is never loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_search_plan_rules_at_their_edges(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "search_plan_test"
    subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I" + os.path.join(ROOT, "tests", "cpp", "hip_host_stub"), "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "ngmlr_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "search_plan_test.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "search_plan_test: ok" in r.stdout
