"""GPU (-m gpu): CIGAR and MD taken from the device inside ngmlr, end to end (oracle/_ref/ngmlr_hip_regions with CVX_JOB_TEXT=1:
SharedAligner's handles carry CVX_CREATE_NM_REGIONS | CVX_CREATE_JOB_TEXT, and Finish copies the launch's device-made text for
every alignment whose request it answers with a note).  Every SAM record must equal the unmodified reference's with the switch
on and with CVX_JOB_TEXT=0 inside the same binary, and the exit line must say where the text came from."""
import gzip
import os
import re

import pytest

from tests.test_gpu_e2e_regions import BINARY, E2E, GOLDEN, REF, ROOT, _run

pytestmark = pytest.mark.gpu
LINE = re.compile(r"SharedAligner: (\d+) alignments took their CIGAR and MD from the device, (\d+) were formatted on the host \(CVX_JOB_TEXT=0 turns that off\)")


def _check(tmp_path, args, want):
    for switch in ("1", "0"):
        got, err = _run(tmp_path, BINARY, args, extra_env={"CVX_JOB_TEXT": switch})
        assert sorted(got) == want, "CVX_JOB_TEXT=" + switch
        m = LINE.search(err)
        assert m, err[-2000:]
        dev, host = int(m.group(1)), int(m.group(2))
        print("CVX_JOB_TEXT=%s: %d alignments from the device, %d formatted on the host" % (switch, dev, host))
        if switch == "1":
            assert dev > 0
        else:
            assert dev == 0 and host > 0


def test_test_3_sam_identical_with_the_devices_text(built, tmp_path):
    fq = os.path.join(str(tmp_path), "test_3.fq")
    with gzip.open(os.path.join(E2E, "test_3_reads.fq.gz"), "rb") as f, open(fq, "wb") as o:
        o.write(f.read())
    args = ["-x", "pacbio", "-t", "8", "-R", "0.01", "--no-progress", "-r", os.path.join(E2E, "test_3_reference.fasta.gz"), "-q", fq]
    with gzip.open(os.path.join(GOLDEN, "test_3.sorted.sam.gz"), "rt") as f:
        want = [l.rstrip("\n") for l in f if l.strip() and not l.startswith("@")]
    assert len(want) > 200
    _check(tmp_path, args, want)


def test_split_reads_sam_identical_with_the_devices_text(built, tmp_path):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import e2e_rates
    fa, fq = str(tmp_path / "sv_ref.fa"), str(tmp_path / "sv_reads.fq")
    e2e_rates.write_sv_workload(fa, fq, 12, seed=78, L=1_000_000)
    args = ["-x", "ont", "-t", "8", "-R", "0.01", "--no-progress", "-r", fa, "-q", fq]
    want, _ = _run(tmp_path, REF, args)
    assert len(want) >= 12 and any(int(l.split("\t")[1]) & 2048 for l in want)          # split reads among them
    _check(tmp_path, args, sorted(want))
