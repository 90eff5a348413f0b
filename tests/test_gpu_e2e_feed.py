"""GPU (-m gpu): ngmlr_hip_feed end to end -- ngmlr_hip_scorewin plus a CS batch of sub-reads searched AND scored in one device call
(cs_feed_binding.inc inside cs_search_binding.inc: CandidateSearchHip::SearchAndScore, ScoreBuffer::addScoredRead over the
reference's own completion block; tools/build_ngmlr_hip.sh).  Every SAM record must equal the unmodified reference's with the
binding on -- the exit line then counts batches that really went through the fused call -- and with CVX_CS_FEED=0 (the two calls
inside the same binary), on the reference's test_3 reads and on a split-read workload (inversions, deletions, foreign insertions)."""
import gzip
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_BIN = os.path.join(ROOT, "oracle", "_ref", "ngmlr_ref")
BIN_ALL = os.path.join(ROOT, "oracle", "_ref", "ngmlr_hip_all")
BIN = os.path.join(ROOT, "oracle", "_ref", "ngmlr_hip_feed")
E2E = os.path.join(ROOT, "tests", "golden", "e2e")
LINE = re.compile(r"CandidateSearchHip: feed: (\d+) batches fused, (\d+) through the two calls \((\d+) CVX_CS_FEED=0, (\d+) no genome announced, "
                  r"(\d+) scorer is not a StrippedSWHip, (\d+) with a short read")


def _binary():
    if not os.path.exists(BIN):
        if os.path.exists(BIN_ALL):
            pytest.fail("oracle/_ref/ngmlr_hip_all was built but ngmlr_hip_feed was not (tools/build_ngmlr_hip.sh)")
        pytest.skip("oracle/_ref/ngmlr_hip_feed not built (tools/build_ngmlr_hip.sh needs /root/reference)")
    return BIN


def _records(text):
    return [l for l in text.splitlines() if l and not l.startswith("@")]


def _run(args, cwd, on, env=None, binary=None):
    res = subprocess.run([binary or _binary(), "--skip-write"] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900, cwd=str(cwd),
                         env=dict(os.environ, CVX_CS_FEED="1" if on else "0", **(env or {})))
    assert res.returncode == 0, res.stderr[-3000:]
    if binary is None:
        m = LINE.search(res.stderr)
        assert m, res.stderr[-3000:]
        fused, two, off, no_genome, scorer, shape = (int(x) for x in m.groups())
        print("feed: %d batches fused, %d through the two calls (%d off, %d no genome, %d scorer, %d shape)" % (fused, two, off, no_genome, scorer, shape))
        if on:
            assert fused > 0 and off == 0 and no_genome == 0 and scorer == 0, m.group(0)
        else:
            assert fused == 0 and two > 0 and off == two, m.group(0)
    return _records(res.stdout)


@pytest.mark.parametrize("on", [True, False], ids=["fused", "two_calls"])
def test_test_3(built, tmp_path, on):
    fq = str(tmp_path / "test_3.fq")
    with gzip.open(os.path.join(E2E, "test_3_reads.fq.gz"), "rb") as f, open(fq, "wb") as o:
        o.write(f.read())
    with gzip.open(os.path.join(ROOT, "tests", "golden", "test_3.sorted.sam.gz"), "rt") as f:
        want = [l.rstrip("\n") for l in f if l.strip()]
    got = _run(["-x", "pacbio", "-t", "8", "-R", "0.01", "--no-progress", "-r", os.path.join(E2E, "test_3_reference.fasta.gz"), "-q", fq], tmp_path, on,
               env={"CVX_POOL_CONTEXTS": "256"})
    assert sorted(got) == want


@pytest.fixture(scope="module")
def sv_workload(tmp_path_factory):
    """e2e_rates.write_sv_workload: ONT-like reads of 8-30 kb, a third with an inversion, a deletion or a foreign insertion -- and
    what the unmodified reference writes for them (one run for the module)"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import e2e_rates
    _binary()
    if not os.path.exists(REF_BIN):
        pytest.fail("oracle/_ref/ngmlr_ref missing next to ngmlr_hip_feed")
    d = tmp_path_factory.mktemp("sv_feed")
    fa, fq = str(d / "sv_ref.fa"), str(d / "sv_reads.fq")
    e2e_rates.write_sv_workload(fa, fq, 120, seed=93)
    args = ["-x", "ont", "-R", "0.01", "--no-progress", "-r", fa, "-q", fq]
    want = _run(["-t", "16"] + args, d, True, binary=REF_BIN)
    return d, args, sorted(want)


@pytest.mark.parametrize("on", [True, False], ids=["fused", "two_calls"])
def test_split_read_workload(built, sv_workload, on):
    d, args, want = sv_workload
    got = _run(["-t", "8"] + args, d, on, env={"CVX_POOL_CONTEXTS": "128"})
    assert len(want) > 100 and sorted(got) == want
