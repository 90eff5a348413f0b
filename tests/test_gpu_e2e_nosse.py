"""GPU (-m gpu): ngmlr --nosse end to end.  The --nosse branch of the reference's ngmlr (src/AlignmentBuffer.h:345-353) is bound to
the same drop-in class as the default branch, constructed in scalar-twin mode (tools/build_ngmlr_hip.sh): Convex::ConvexAlign's
semantics on the MI355X.  The SAM records must equal those of the unmodified reference run with --nosse
(tests/golden/test_*.nosse*.sam*, tools/make_golden_twin.sh) -- which differ from the default run's in the SV:i tag of nearly
every record: the twin leaves the read's id in Align::svType, so the test also shows that the bindings number reads as the
reference's reader does -- and the alignments must have gone through device launches, as many as the reference made calls."""
import gzip
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
E2E = os.path.join(GOLDEN, "e2e")
BINARIES = {"ngmlr_hip": 1, "ngmlr_hip_batched": 16, "ngmlr_hip_all": 16}      # binary -> -t


def _calls():
    out = {}
    for line in open(os.path.join(GOLDEN, "nosse_calls.txt")):
        if not line.startswith("#"):
            name, n, nx = line.split()
            out[name] = (int(n), int(nx))
    return out


def _want(name):
    path = os.path.join(GOLDEN, "test_3.nosse.sorted.sam.gz" if name == "test_3" else "%s.nosse.sam" % name)
    with (gzip.open(path, "rt") if path.endswith(".gz") else open(path)) as f:
        return [l.rstrip("\n") for l in f if l.strip() and not l.startswith("@")]


def _args(name, threads, tmp_path):
    if name == "test_2":
        return ["-t", str(threads), "-r", os.path.join(E2E, "ref_chr21_20kb.fa"), "-q", os.path.join(E2E, "reads_100_2200bp.fa")]
    if name == "test_4":
        return ["-x", "pacbio", "-t", str(threads), "-r", os.path.join(E2E, "test_4_reference.fasta.gz"), "-q", os.path.join(E2E, "test_4_read.fa.gz")]
    fq = os.path.join(str(tmp_path), "test_3.fq")          # FASTQ: FASTA + a reverse-strand hit crashes the reference
    with gzip.open(os.path.join(E2E, "test_3_reads.fq.gz"), "rb") as f, open(fq, "wb") as o:
        o.write(f.read())
    return ["-x", "pacbio", "-t", str(threads), "-R", "0.01", "--no-progress", "-r", os.path.join(E2E, "test_3_reference.fasta.gz"), "-q", fq]


def test_the_nosse_fixtures_are_not_the_default_run():
    """Every difference to the default run's records is the SV:i tag (the read's id instead of the N-clip flags)."""
    default = [l for l in open(os.path.join(GOLDEN, "test_2.sam")).read().splitlines() if l and not l.startswith("@")]
    nosse = _want("test_2")
    strip = lambda recs: sorted(re.sub(r"\tSV:i:-?\d+", "", r) for r in recs)      # noqa: E731
    assert len(nosse) == 12 and strip(nosse) == strip(default) and sorted(nosse) != sorted(default)
    assert len(_want("test_3")) == 202 and len(_want("test_4")) == 1
    assert _calls()["test_3"] == (985, 93)


@pytest.mark.parametrize("name", ["test_2", "test_4", "test_3"])
@pytest.mark.parametrize("binary", sorted(BINARIES))
def test_nosse_sam_identical_to_the_reference(built, tmp_path, binary, name):
    exe = os.path.join(ROOT, "oracle", "_ref", binary)
    if not os.path.exists(exe):
        pytest.skip("%s not built (tools/build_ngmlr_hip.sh needs the reference tree)" % binary)
    res = subprocess.run([exe, "--skip-write", "--nosse"] + _args(name, BINARIES[binary], tmp_path), stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, text=True, timeout=600, cwd=str(tmp_path))
    assert res.returncode == 0, res.stderr[-3000:]
    got = sorted(l for l in res.stdout.splitlines() if l and not l.startswith("@"))
    want = sorted(_want(name))
    assert len(got) == len(want)
    bad = [(g, w) for g, w in zip(got, want) if g != w]
    assert not bad, (len(bad), bad[0])
    if binary != "ngmlr_hip":
        # the LAST summary: SharedAligner prints its running totals whenever its last user leaves, and with 16 workers on one
        # read the early workers may all have left before the read's worker joins (then a first line says 0 alignments)
        ms = re.findall(r"SharedAligner: (\d+) alignments in (\d+) device launches", res.stderr)
        assert ms, res.stderr[-2000:]
        assert int(ms[-1][0]) == _calls()[name][0] and int(ms[-1][1]) >= 1      # every call of the reference's run, on the device
    else:
        syms = subprocess.run(["nm", "-C", exe], stdout=subprocess.PIPE, text=True).stdout
        assert "Convex::ConvexAlignHip::ScalarTwin" in syms or "ConvexAlignHip::ConvexAlignHip" in syms
