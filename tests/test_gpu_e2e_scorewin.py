"""GPU (-m gpu): ngmlr_hip_scorewin end to end -- ngmlr_hip_all plus the scoring calls of ScoreBuffer::DoRun and scoreShortRead as
windows of the resident genome (score_windows_binding.inc, StrippedSWHip::BatchScoreWindows; tools/build_ngmlr_hip.sh).  Every SAM
record must equal the unmodified reference's with the binding on -- the exit line then counts its calls, none of whose pairs went
through the string path on these inputs -- and with CVX_SCORE_WINDOWS=0 (the string path inside the same binary)."""
import gzip
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN_ALL = os.path.join(ROOT, "oracle", "_ref", "ngmlr_hip_all")
BIN = os.path.join(ROOT, "oracle", "_ref", "ngmlr_hip_scorewin")
E2E = os.path.join(ROOT, "tests", "golden", "e2e")
LINE = re.compile(r"StrippedSWHip: (\d+) window calls(?: on device \d+ \(physical \d+\))?, (\d+) pairs, (\d+) through the string path")


def _binary():
    if not os.path.exists(BIN):
        if os.path.exists(BIN_ALL):
            pytest.fail("oracle/_ref/ngmlr_hip_all was built but ngmlr_hip_scorewin was not (tools/build_ngmlr_hip.sh)")
        pytest.skip("oracle/_ref/ngmlr_hip_scorewin not built (tools/build_ngmlr_hip.sh needs /root/reference)")
    return BIN


def _records(text):
    return [l for l in text.splitlines() if l and not l.startswith("@")]


def _run(args, cwd, on, env=None):
    res = subprocess.run([_binary(), "--skip-write"] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900, cwd=str(cwd),
                         env=dict(os.environ, CVX_SCORE_WINDOWS="1" if on else "0", **(env or {})))
    assert res.returncode == 0, res.stderr[-3000:]
    calls = [tuple(int(x) for x in m) for m in LINE.findall(res.stderr)]
    assert calls, res.stderr[-3000:]
    n_calls, n_pairs, n_strings = (sum(c[k] for c in calls) for k in range(3))
    if on:
        assert n_calls > 0 and n_pairs >= n_calls and n_strings == 0, calls
    else:
        assert n_calls == 0 and n_pairs == 0, calls
    return _records(res.stdout)


@pytest.mark.parametrize("on", [True, False], ids=["windows", "strings"])
def test_test_2_and_test_4(built, tmp_path, on):
    got = _run(["-t", "1", "-r", os.path.join(E2E, "ref_chr21_20kb.fa"), "-q", os.path.join(E2E, "reads_100_2200bp.fa")], tmp_path, on)
    assert sorted(got) == sorted(_records(open(os.path.join(ROOT, "tests", "golden", "test_2.sam")).read()))     # (the pool's record order)
    got = _run(["-x", "pacbio", "-t", "1", "-r", os.path.join(E2E, "test_4_reference.fasta.gz"), "-q", os.path.join(E2E, "test_4_read.fa.gz")], tmp_path, on)
    assert sorted(got) == sorted(_records(open(os.path.join(ROOT, "tests", "golden", "test_4.sam")).read()))


@pytest.mark.parametrize("on", [True, False], ids=["windows", "strings"])
def test_test_3(built, tmp_path, on):
    fq = str(tmp_path / "test_3.fq")
    with gzip.open(os.path.join(E2E, "test_3_reads.fq.gz"), "rb") as f, open(fq, "wb") as o:
        o.write(f.read())
    with gzip.open(os.path.join(ROOT, "tests", "golden", "test_3.sorted.sam.gz"), "rt") as f:
        want = [l.rstrip("\n") for l in f if l.strip()]
    got = _run(["-x", "pacbio", "-t", "8", "-R", "0.01", "--no-progress", "-r", os.path.join(E2E, "test_3_reference.fasta.gz"), "-q", fq], tmp_path, on,
               env={"CVX_POOL_CONTEXTS": "256"})
    assert sorted(got) == want
