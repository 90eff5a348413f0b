"""GPU (-m gpu): ngmlr_hip_readseg end to end -- ngmlr_hip_all plus the query of every alignment tile taken as a segment of the
launch's read block and written on the device (read_segments_binding.inc at the top of the Interval overload of extractReadSeq,
Convex::DeviceReads::CopyOut in checkForSV; tools/build_ngmlr_hip.sh).  Every SAM record must equal the unmodified reference's on
test_3 and on the split-read workload with the binding on -- the exit line then counts noted launches -- and with
CVX_DEVICE_READS=0 (the reference's strings inside the same binary)."""
import gzip
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN_ALL = os.path.join(ROOT, "oracle", "_ref", "ngmlr_hip_all")
BIN = os.path.join(ROOT, "oracle", "_ref", "ngmlr_hip_readseg")
REF_BIN = os.path.join(ROOT, "oracle", "_ref", "ngmlr_ref")
E2E = os.path.join(ROOT, "tests", "golden", "e2e")
LINE = re.compile(r"SharedAligner: (\d+) tiles in (\d+) launches took their query as a segment of the launch's read block .*?, (\d+) mixed launches")


def _binary():
    if not os.path.exists(BIN):
        if os.path.exists(BIN_ALL):
            pytest.fail("oracle/_ref/ngmlr_hip_all was built but ngmlr_hip_readseg was not (tools/build_ngmlr_hip.sh)")
        pytest.skip("oracle/_ref/ngmlr_hip_readseg not built (tools/build_ngmlr_hip.sh needs /root/reference)")
    return BIN


def _records(text):
    return [l for l in text.splitlines() if l and not l.startswith("@")]


def _run(args, cwd, on, env=None, binary=None):
    res = subprocess.run([binary or _binary(), "--skip-write"] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900, cwd=str(cwd),
                         env=dict(os.environ, CVX_DEVICE_READS="1" if on else "0", **(env or {})))
    assert res.returncode == 0, res.stderr[-3000:]
    if binary is None:
        noted = [tuple(int(x) for x in m) for m in LINE.findall(res.stderr)]
        if on:
            assert noted and noted[0][0] >= noted[0][1] > 0, res.stderr[-3000:]      # noted launches > 0
        else:
            assert not noted, noted
    return _records(res.stdout), res.stderr


@pytest.mark.parametrize("on", [True, False], ids=["segments", "strings"])
def test_test_3(built, tmp_path, on):
    fq = str(tmp_path / "test_3.fq")
    with gzip.open(os.path.join(E2E, "test_3_reads.fq.gz"), "rb") as f, open(fq, "wb") as o:
        o.write(f.read())
    with gzip.open(os.path.join(ROOT, "tests", "golden", "test_3.sorted.sam.gz"), "rt") as f:
        want = [l.rstrip("\n") for l in f if l.strip()]
    got, err = _run(["-x", "pacbio", "-t", "8", "-R", "0.01", "--no-progress", "-r", os.path.join(E2E, "test_3_reference.fasta.gz"), "-q", fq], tmp_path, on,
                    env={"CVX_POOL_CONTEXTS": "256"})
    assert sorted(got) == want
    assert re.search(r"SharedAligner: 985 alignments", err), err[-1500:]


@pytest.mark.parametrize("on", [True, False], ids=["segments", "strings"])
def test_split_reads(built, tmp_path, on):
    """the split-read workload of tests/test_gpu_e2e.py (several intervals per read, reverse-strand segments, realignment) against
    the unmodified reference run in this very test"""
    if not os.path.exists(REF_BIN):
        pytest.skip("oracle/_ref/ngmlr_ref not built")
    _binary()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import e2e_rates
    fa, fq = str(tmp_path / "sv_ref.fa"), str(tmp_path / "sv_reads.fq")
    e2e_rates.write_sv_workload(fa, fq, 160, seed=77)
    args = ["-x", "ont", "-R", "0.01", "--no-progress", "-r", fa, "-q", fq]
    want, _ = _run(["-t", "16"] + args, tmp_path, on, binary=REF_BIN)
    got, _ = _run(["-t", "8"] + args, tmp_path, on, env={"CVX_POOL_CONTEXTS": "128"})
    assert sorted(got) == sorted(want)
    flags = [int(l.split("\t")[1]) for l in want]
    assert sum(1 for f in flags if f & 2048) >= 20 and any(f & 16 for f in flags), "the workload must exercise split and reverse-strand records"
