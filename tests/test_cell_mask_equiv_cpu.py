"""CPU: the lane-mask network of the FAST ring fill's cell update (cvx_fill_ring.inc, phase2 / phase3) and the two ways a lane's row
activity can enter it -- a select and two `& act` on the masks, or the maximum and the equalities written under EXEC = act into
registers that hold zero -- restated for one lane in tests/cpp/cell_mask_equiv_test.cpp: all 64 mask combinations, and one slot with
the slot above it over random histories (rows that start and end, +0 / -0 scores, three-way ties, a positive neighbour beside a
lane outside its row).  Built with plain g++ under -fsanitize=address,undefined; the program has its own main and is never loaded
into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cell_mask_equiv(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "cell_mask_equiv_test"
    subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "ngmlr_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "cell_mask_equiv_test.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cell_mask_equiv_test: ok" in r.stdout
