"""CPU: the cell update of the FAST ring fill in its two domains -- unscaled with max(max3, 0) and the offer max(S + pen, S * -2^100),
and scaled by 2^-64 with the clamp of v_max3_f32 and the offer max(S + pen, -S) (cvx_fill_ring.inc) -- restated for whole tiles of
at most 64 x 64 cells in tests/cpp/cell_scale_equiv_test.cpp: identical masks per cell and scores bit-equal after scaling back,
with both signs of zero fed in and returned by the clamp; and the host's condition for the scaled form, score_scale_exact()
(cvx_host_logic.h).  Built with plain g++ under -fsanitize=address,undefined; the program has its own main and is never loaded
into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cell_scale_equiv(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "cell_scale_equiv_test"
    subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-pthread",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "ngmlr_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "cell_scale_equiv_test.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cell_scale_equiv_test: ok" in r.stdout
