"""CPU: the inversion-check binding without a GPU.

tests/cpp/inv_note_test.cpp (a program of its own, no device; built here plain and under ASan / UBSan, and by the Makefile's
shim_test target): the checks form of the note
(nm_regions_note.h) -- round trips, the regrow from the allocation binding's buffer, stale notes, neither form taken for the
other or for a profile, zeros or a request -- and the outcomes of inv_checks_binding_logic.h against hand-written expectations.
The same program is held to the unmodified reference: for each of the 1 013 checkForSV calls recorded on test_3
(tests/golden/inv_checks_test_3.npz) the logic's class from (mid_read, read_len, inv_len) must be the recorded outcome.

oracle/_ref/ngmlr_invchecks_cpu (tools/build_ngmlr_hip.sh): both insertion sites inside the reference's own binary, the records
filled in at the finder site from the host rule (tests/cpp/inv_checks_cpu_source.h).  The SAM must equal the unmodified
reference's with the binding on, with CVX_DEVICE_INV_CHECKS=0 and under CVX_INV_CHECKS_VERIFY=1; the exit line must show the
checks taken, none through checkForSV's own scoring for a missing window or an inconsistent record, and under verify every taken
check verified without a disagreement."""
import gzip
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
E2E = os.path.join(GOLDEN, "e2e")
NOTE_TEST = os.path.join(ROOT, "ngmlr_amd", "inv_note_test")
BINARY = os.path.join(ROOT, "oracle", "_ref", "ngmlr_invchecks_cpu")
REF = os.path.join(ROOT, "oracle", "_ref", "ngmlr_ref")
SV_READS = 4
LINE = re.compile(r"DeviceInvChecks: (\d+) checks taken from the job \((\d+) scored, (\d+) without a read part\), (\d+) through checkForSV's own scoring "
                  r"\((\d+) no window, (\d+) inconsistent record, (\d+) note without checks\), (\d+) verified, (\d+) disagreements")
SWITCHES = ("CVX_DEVICE_INV_CHECKS", "CVX_INV_CHECKS_VERIFY", "CVX_DEVICE_REGIONS")

needs_binary = pytest.mark.skipif(not (os.path.exists(BINARY) and os.path.exists(REF)),
                                  reason="oracle/_ref/ngmlr_invchecks_cpu not built (tools/build_ngmlr_hip.sh needs /root/reference)")


def exit_line(err):
    """-> dict of the one DeviceInvChecks line: N, S, R, F, a, b, c, V, D"""
    lines = LINE.findall(err)
    assert len(lines) == 1, err[-2000:]
    return dict(zip("NSRFabcVD", (int(x) for x in lines[0])))


@pytest.fixture(scope="module", params=[False, True], ids=["plain", "asan_ubsan"])
def note_test(request, tmp_path_factory):
    """tests/cpp/inv_note_test.cpp as a program of its own (its own main, never loaded into Python), built with plain g++ and again
    under -fsanitize=address,undefined; the Makefile's shim_test target builds the plain form too (ngmlr_amd/inv_note_test)"""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = tmp_path_factory.mktemp("inv_note") / "inv_note_test"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if request.param else []
    subprocess.run([gxx, "-O1", "-g", "-std=c++11", "-Wall", "-Werror"] + flags +
                   ["-I" + os.path.join(ROOT, "ngmlr_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "inv_note_test.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, timeout=300)
    return str(exe)


def test_note_and_logic(note_test):
    r = subprocess.run([note_test], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "inv_note_test: ok" in r.stdout


def test_makefile_builds_the_note_test(built):
    assert os.path.exists(NOTE_TEST), "make -C ngmlr_amd/csrc shim_test builds it"
    r = subprocess.run([NOTE_TEST], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "inv_note_test: ok" in r.stdout, r.stdout + r.stderr


def test_logic_classes_equal_the_reference_recording(note_test, tmp_path):
    """(inv_len, mid_read, read_len) of every recorded call through the program's `classes` mode: one class per line"""
    z = np.load(os.path.join(GOLDEN, "inv_checks_test_3.npz"))
    n = int(z["n"])
    assert n == 1013
    calls = tmp_path / "calls.txt"
    with open(calls, "w") as f:
        for k in range(n):
            f.write("%d %d %d\n" % (int(z["inv_len"][k]), int(z["mid_read"][k]), int(z["read_len"][k])))
    r = subprocess.run([note_test, "classes", str(calls)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.array([int(l) for l in r.stdout.split()], dtype=np.int32)
    assert got.shape == (n,)
    want = z["outcome"].astype(np.int32)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]
    # CVX_CHECK_SCORED / _TOO_SHORT / _NO_READ
    assert [int((got == c).sum()) for c in (0, 1, 2)] == [497, 512, 4]


def _records(text):
    return [l.rstrip("\n") for l in text.splitlines() if l.strip() and not l.startswith("@")]


def _run(cwd, binary, args, extra_env=None):
    env = dict(os.environ)
    for k in SWITCHES:
        env.pop(k, None)
    env.update(extra_env or {})
    res = subprocess.run([binary, "--skip-write"] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                         timeout=900, cwd=str(cwd), env=env)
    assert res.returncode == 0, res.stderr[-2000:]
    return _records(res.stdout), res.stderr


def _three_ways(cwd, args, want, min_scored):
    got, err = _run(cwd, BINARY, args)
    assert sorted(got) == want, "binding on"
    on = exit_line(err)
    print("on:", on)
    assert on["S"] >= min_scored and on["N"] == on["S"] + on["R"]
    assert on["a"] == 0 and on["b"] == 0
    assert on["V"] == 0 and on["D"] == 0

    got, err = _run(cwd, BINARY, args, {"CVX_INV_CHECKS_VERIFY": "1"})
    assert sorted(got) == want, "CVX_INV_CHECKS_VERIFY=1"
    ver = exit_line(err)
    print("verify:", ver)
    assert ver["S"] >= min_scored and ver["a"] == 0 and ver["b"] == 0
    assert ver["D"] == 0 and ver["V"] == ver["N"]

    got, err = _run(cwd, BINARY, args, {"CVX_DEVICE_INV_CHECKS": "0"})
    assert sorted(got) == want, "CVX_DEVICE_INV_CHECKS=0"
    off = exit_line(err)
    print("off:", off)
    assert off["N"] == 0 and off["V"] == 0


@needs_binary
def test_test_3_sam_identical_on_off_and_verified(tmp_path):
    fq = os.path.join(str(tmp_path), "test_3.fq")
    with gzip.open(os.path.join(E2E, "test_3_reads.fq.gz"), "rb") as f, open(fq, "wb") as o:
        o.write(f.read())
    args = ["-x", "pacbio", "-t", "4", "-R", "0.01", "--no-progress", "-r", os.path.join(E2E, "test_3_reference.fasta.gz"), "-q", fq]
    with gzip.open(os.path.join(GOLDEN, "test_3.sorted.sam.gz"), "rt") as f:
        want = [l.rstrip("\n") for l in f if l.strip() and not l.startswith("@")]
    assert len(want) > 200
    ref, _ = _run(tmp_path, REF, args)
    assert sorted(ref) == want
    # the reference's recording holds 497 distinct scored calls and no NO_WINDOW
    _three_ways(tmp_path, args, want, 497)


@needs_binary
def test_split_reads_sam_identical_on_off_and_verified(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import e2e_rates
    fa, fq = str(tmp_path / "sv_ref.fa"), str(tmp_path / "sv_reads.fq")
    e2e_rates.write_sv_workload(fa, fq, SV_READS, seed=78, L=1_000_000)
    args = ["-x", "ont", "-t", "8", "-R", "0.01", "--no-progress", "-r", fa, "-q", fq]
    want, _ = _run(tmp_path, REF, args)
    assert len(want) >= SV_READS
    _three_ways(tmp_path, args, sorted(want), 1)
