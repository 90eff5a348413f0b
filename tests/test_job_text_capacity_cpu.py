"""CPU: the host logic of a job that delivers its CIGAR / MD strings with its results (ngmlr_amd/csrc/cvx_job_text_logic.h): the first
capacity of the string arena (kJobTextBytesPerRow x read rows + 64 x tiles), the predicate text_bounded_kernel asks before a tile
writes -- against a byte map of the arena --, and CVX_TUNE_JOB_TEXT_CAP's parsing.  tests/cpp/job_text_capacity_test.cpp is a
program of its own: no device, no library."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_job_text_capacity(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "job_text_capacity_test"
    subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "ngmlr_amd", "csrc"),
                    "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "job_text_capacity_test.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "job_text_capacity_test: ok" in r.stdout
