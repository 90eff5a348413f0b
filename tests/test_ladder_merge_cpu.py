"""CPU: the rule by which cvx_wait merges the per-rung regions, checks and text of a ladder job (cvx::ladder_merge_plan /
ladder_merge_records, ngmlr_amd/csrc/cvx_ladder_merge.h) as a program of its own -- its own main, host code only, never loaded
into Python -- built with plain g++ and again under -fsanitize=address,undefined: ladders of one to five rungs, a tile reported
by each rung, tiles without regions or text, a failed last rung, an empty job, every arena allocated at exactly its size, the
merged offsets and arena against a straightforward per-tile rebuild (tests/cpp/ladder_merge_test.cpp)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_ladder_merge(tmp_path, sanitize):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "ladder_merge_test"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else []
    subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror"] + flags +
                   ["-I" + os.path.join(ROOT, "ngmlr_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "ladder_merge_test.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ladder_merge_test: ok" in r.stdout
