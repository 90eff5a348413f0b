"""GPU (-m gpu): ngmlr_hip_checks end to end -- ngmlr_hip_all plus the interval check (AlignmentBuffer::scoreInterval, reference
src/AlignmentBuffer.cpp:2515-2548) and the inversion check (checkForSV, :1158-1235) scored on the device through
Convex::SharedScorer / BatchingScorer (tools/build_ngmlr_hip.sh).  Every SAM record must equal the unmodified reference's, with
the checks on the device (the exit line counts them) and with CVX_CHECK_SCORER=0 (the reference's StrippedSW inside the same
binary), on one and on two logical devices."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_BIN = os.path.join(ROOT, "oracle", "_ref", "ngmlr_ref")
BIN_ALL = os.path.join(ROOT, "oracle", "_ref", "ngmlr_hip_all")
BIN_CHECKS = os.path.join(ROOT, "oracle", "_ref", "ngmlr_hip_checks")
E2E = os.path.join(ROOT, "tests", "golden", "e2e")
LINE = re.compile(r"BatchingScorer: device (\d+): (\d+) interval checks, (\d+) inversion checks, (\d+) launches, ([\d.]+) pairs per launch, ([\d.]+) ms of kernels")


def _binary():
    if not os.path.exists(BIN_CHECKS):
        if os.path.exists(BIN_ALL):
            pytest.fail("oracle/_ref/ngmlr_hip_all was built but ngmlr_hip_checks was not (tools/build_ngmlr_hip.sh)")
        pytest.skip("oracle/_ref/ngmlr_hip_checks not built (tools/build_ngmlr_hip.sh needs /root/reference)")
    return BIN_CHECKS


def _records(text):
    return [l for l in text.splitlines() if l and not l.startswith("@")]


def _run(args, cwd, binary, env=None):
    res = subprocess.run([binary, "--skip-write"] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         text=True, timeout=900, cwd=str(cwd), env=dict(os.environ, **(env or {})))
    assert res.returncode == 0, res.stderr[-3000:]
    return _records(res.stdout), res.stderr


def _checks(err):
    """{device: (interval checks, inversion checks, launches)} from the exit lines"""
    return {int(m[0]): (int(m[1]), int(m[2]), int(m[3])) for m in LINE.findall(err)}


def test_test_2_and_test_4(built, tmp_path):
    b = _binary()
    got, err = _run(["-t", "1", "-r", os.path.join(E2E, "ref_chr21_20kb.fa"), "-q", os.path.join(E2E, "reads_100_2200bp.fa")], tmp_path, b)
    assert sorted(got) == sorted(_records(open(os.path.join(ROOT, "tests", "golden", "test_2.sam")).read()))     # (the pool's record order)
    got, err = _run(["-x", "pacbio", "-t", "1", "-r", os.path.join(E2E, "test_4_reference.fasta.gz"),
                     "-q", os.path.join(E2E, "test_4_read.fa.gz")], tmp_path, b)
    assert sorted(got) == sorted(_records(open(os.path.join(ROOT, "tests", "golden", "test_4.sam")).read()))


def test_test_3(built, tmp_path):
    import gzip
    b = _binary()
    fq = str(tmp_path / "test_3.fq")
    with gzip.open(os.path.join(E2E, "test_3_reads.fq.gz"), "rb") as f, open(fq, "wb") as o:
        o.write(f.read())
    with gzip.open(os.path.join(ROOT, "tests", "golden", "test_3.sorted.sam.gz"), "rt") as f:
        want = [l.rstrip("\n") for l in f if l.strip()]
    got, err = _run(["-x", "pacbio", "-t", "8", "-R", "0.01", "--no-progress", "-r", os.path.join(E2E, "test_3_reference.fasta.gz"), "-q", fq],
                    tmp_path, b, env={"CVX_POOL_CONTEXTS": "256"})
    assert sorted(got) == want


def _append_short_events(fa, fq, n_reads, seed):
    """Reads of 8-20 kb on the same reference with a SHORT event inside: a 450-900 base piece inverted, or copied in from
    100 kb or more away.  The read's gap between the flanking intervals is then shorter than 1 000 bases and overlapped by
    the piece's own interval, which is what makes gapOverlapsWithInterval score both (src/AlignmentBuffer.cpp:2685-2724);
    write_sv_workload's events (inversions of 1-3 kb, foreign insertions) never reach that check."""
    import numpy as np
    from ngmlr_amd import synth
    ref = np.frombuffer("".join(l.strip() for l in open(fa) if not l.startswith(">")).encode(), dtype=np.uint8)
    rng = np.random.default_rng(seed)
    with open(fq, "a") as f:
        for i in range(n_reads):
            n = int(rng.integers(8000, 20000))
            a = int(rng.integers(200000, len(ref) - n - 200000))
            w = ref[a:a + n].copy()
            m = int(rng.integers(450, 900))
            p0 = int(rng.integers(3000, n - m - 3000))
            if i % 2:
                w = np.concatenate([w[:p0], synth.revcomp(w[p0:p0 + m]), w[p0 + m:]])
            else:
                b = int(rng.integers(0, a - 100000 - m)) if rng.random() < 0.5 else int(rng.integers(a + n + 100000, len(ref) - m))
                w = np.concatenate([w[:p0], ref[b:b + m], w[p0 + m:]])
            q = synth.mutate(rng, w, 0.08, (4, 4, 2))
            if rng.random() < 0.5:
                q = synth.revcomp(q)
            f.write("@short%d_%d\n%s\n+\n%s\n" % (i, a, q.tobytes().decode(), "I" * len(q)))


@pytest.fixture(scope="module")
def sv_workload(tmp_path_factory):
    """e2e_rates.write_sv_workload (ONT-like reads of 8-30 kb, a third with an inversion, a deletion or a foreign insertion) plus
    reads with short events on the same reference (_append_short_events)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import e2e_rates
    d = tmp_path_factory.mktemp("sv_checks")
    fa, fq = str(d / "sv_ref.fa"), str(d / "sv_reads.fq")
    e2e_rates.write_sv_workload(fa, fq, 240, seed=91)
    _append_short_events(fa, fq, 160, seed=92)
    return d, fa, fq


_want_cache = {}


def _sv(sv_workload, extra, env=None, threads="8"):
    b = _binary()
    d, fa, fq = sv_workload
    if not os.path.exists(REF_BIN):
        pytest.fail("oracle/_ref/ngmlr_ref missing next to ngmlr_hip_checks")
    args = ["-x", "ont", "-R", "0.01", "--no-progress"] + extra + ["-r", fa, "-q", fq]
    key = tuple(extra)
    if key not in _want_cache:
        _want_cache[key] = _run(["-t", "16"] + args, d, REF_BIN)[0]
    got, err = _run(["-t", threads] + args, d, b, env=dict({"CVX_POOL_CONTEXTS": "128"}, **(env or {})))
    return sorted(got), sorted(_want_cache[key]), err


@pytest.mark.parametrize("extra", [[], ["--subread-corridor", "80"]])
def test_sv_workload_checks_on_the_device(built, sv_workload, extra):
    got, want, err = _sv(sv_workload, extra)
    assert got == want
    c = _checks(err)
    assert set(c) == {0}, err[-2000:]
    interval, inversion, launches = c[0]
    assert interval > 0 and inversion > 0 and launches > 0, err[-2000:]


def test_sv_workload_reference_scorer_in_the_same_binary(built, sv_workload):
    """CVX_CHECK_SCORER=0: the proxies hand every check to the reference's StrippedSW; no device scorer is created."""
    got, want, err = _sv(sv_workload, [], env={"CVX_CHECK_SCORER": "0"})
    assert got == want
    assert _checks(err) == {}, err[-2000:]


def test_sv_workload_two_logical_devices(built, sv_workload):
    """CVX_ALIAS_DEVICES=2: the proxies are dealt over both logical devices, each with its own scorer and handle."""
    got, want, err = _sv(sv_workload, [], env={"CVX_ALIAS_DEVICES": "2", "CVX_POOL_CONTEXTS": "256"})
    assert got == want
    c = _checks(err)
    assert set(c) == {0, 1}, err[-2000:]
    assert all(v[0] + v[1] > 0 for v in c.values()), c
    assert sum(v[0] for v in c.values()) > 0 and sum(v[1] for v in c.values()) > 0, c
