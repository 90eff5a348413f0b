"""CPU: the request / note a caller and the aligner exchange in Align::nmPerPosition (ngmlr_amd/csrc/nm_regions_note.h).
tests/cpp/nm_note_test.cpp is a program of its own (its own main, never loaded into Python), built with plain g++ and again
under -fsanitize=address,undefined: round trips with 0, 1, 16, 17 and 1 000 regions, the growth of a buffer too small for its
note, profiles never taken for a request or a note -- a zeroed buffer, random rows and the first entry of every profile
recorded in tests/golden/ref_test_3.npz --, and a request that ends as a full profile where there are no regions, in a
buffer no shorter than the alignmentLength rows the profile's reader scans.  (That a request survives an invalid result is
ConvexAlignHip::Finish's doing and is checked where it runs, tests/test_gpu_shim_regions.py.)"""
import os
import shutil
import subprocess

import pytest

from tests import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def first_entries(tmp_path_factory):
    path = tmp_path_factory.mktemp("nm_note") / "first_entries.txt"
    rows = [exp["nm_per_position"].reshape(-1, 3)[0] for _t, exp in util.load_golden("ref_test_3.npz")
            if exp["ret"] >= 0 and len(exp["nm_per_position"])]
    assert len(rows) >= 30
    path.write_text("".join("%d %d %d\n" % tuple(int(v) for v in r) for r in rows))
    return str(path), len(rows)


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_nm_note(tmp_path, first_entries, sanitize):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "nm_note_test"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else []
    subprocess.run([gxx, "-O1", "-g", "-std=c++11", "-Wall", "-Werror"] + flags +
                   ["-I" + os.path.join(ROOT, "ngmlr_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "nm_note_test.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, timeout=300)
    path, n = first_entries
    r = subprocess.run([str(exe), path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "nm_note_test: ok" in r.stdout and "nm_note_test: %d recorded first entries" % n in r.stdout
