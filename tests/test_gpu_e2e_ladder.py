"""GPU (-m gpu): computeAlignment's retry loop as one request, end to end (oracle/_ref/ngmlr_hip_ladder = ngmlr_hip_regions +
ladder_binding.inc, tools/build_ngmlr_hip.sh): the binding fills a cvx_ladder, SharedAligner's dispatcher gathers ladder launches
from the parked contexts and the device climbs.  In this one binary the ladder meets the regions note, job text
(CVX_JOB_TEXT=1), window placeholders, the profile (CVX_DEVICE_REGIONS=0), plain reference strings (CVX_DEVICE_DECODE=0) and the
scalar twin (--nosse); CVX_DEVICE_LADDER=0 and CVX_DEVICE_TEXT=1 leave the reference's loop running.  Every SAM record must equal
the unmodified reference's every time, and the device's exit line must show the ladders taken -- at least the 12 calls with two
attempts or more that the reference's recording holds on test_3 (tests/golden/ladder_test_3.npz) -- or none."""
import gzip
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
E2E = os.path.join(GOLDEN, "e2e")
BINARY = os.path.join(ROOT, "oracle", "_ref", "ngmlr_hip_ladder")
REF = os.path.join(ROOT, "oracle", "_ref", "ngmlr_ref")
LINE = re.compile(r"SharedAligner: device (\d+): (\d+) ladder requests, (\d+) with attempts >= 2, (\d+) reported a failed last rung, (\d+) ladder launches")
# switch -> does the binding take the ladders
SWITCHES = [("default", {}, True), ("CVX_DEVICE_LADDER=0", {"CVX_DEVICE_LADDER": "0"}, False), ("CVX_DEVICE_REGIONS=0", {"CVX_DEVICE_REGIONS": "0"}, True),
            ("CVX_JOB_TEXT=1", {"CVX_JOB_TEXT": "1"}, True), ("CVX_DEVICE_DECODE=0", {"CVX_DEVICE_DECODE": "0"}, True), ("CVX_DEVICE_TEXT=1", {"CVX_DEVICE_TEXT": "1"}, False)]


def _records(text):
    return [l.rstrip("\n") for l in text.splitlines() if l.strip() and not l.startswith("@")]


def _run(cwd, binary, args, extra_env=None):
    if not os.path.exists(binary):
        pytest.skip("%s not built (tools/build_ngmlr_hip.sh needs /root/reference)" % os.path.relpath(binary, ROOT))
    env = dict(os.environ, CVX_POOL_CONTEXTS="128")
    for k in ("CVX_DEVICE_LADDER", "CVX_DEVICE_REGIONS", "CVX_JOB_TEXT", "CVX_DEVICE_DECODE", "CVX_DEVICE_TEXT"):
        env.pop(k, None)
    env.update(extra_env or {})
    res = subprocess.run([binary, "--skip-write"] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                         timeout=600, cwd=str(cwd), env=env)
    assert res.returncode == 0, res.stderr[-3000:]
    return _records(res.stdout), res.stderr


def _ladders(err):
    """-> (ladder requests, with attempts >= 2, with a failed last rung, ladder launches) summed over the devices' exit lines"""
    lines = LINE.findall(err)
    assert lines, err[-2000:]
    return tuple(sum(int(l[k]) for l in lines) for k in range(1, 5))


@pytest.fixture(scope="module")
def test_3(built, tmp_path_factory):
    d = tmp_path_factory.mktemp("ladder_test_3")
    fq = os.path.join(str(d), "test_3.fq")
    with gzip.open(os.path.join(E2E, "test_3_reads.fq.gz"), "rb") as f, open(fq, "wb") as o:
        o.write(f.read())
    args = ["-x", "pacbio", "-t", "8", "-R", "0.01", "--no-progress", "-r", os.path.join(E2E, "test_3_reference.fasta.gz"), "-q", fq]
    with gzip.open(os.path.join(GOLDEN, "test_3.sorted.sam.gz"), "rt") as f:
        want = [l.rstrip("\n") for l in f if l.strip() and not l.startswith("@")]
    assert len(want) > 200
    return d, args, want


@pytest.fixture(scope="module")
def split_reads(built, tmp_path_factory):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import e2e_rates
    d = tmp_path_factory.mktemp("ladder_split")
    fa, fq = str(d / "sv_ref.fa"), str(d / "sv_reads.fq")
    e2e_rates.write_sv_workload(fa, fq, 12, seed=78, L=1_000_000)
    args = ["-x", "ont", "-t", "8", "-R", "0.01", "--no-progress", "-r", fa, "-q", fq]
    want, _ = _run(d, REF, args)
    assert len(want) >= 12 and any(int(l.split("\t")[1]) & 2048 for l in want)          # split reads among them
    return d, args, sorted(want)


@pytest.mark.parametrize("name,env,taken", SWITCHES, ids=[s[0] for s in SWITCHES])
def test_test_3_sam_identical_with_ladders(test_3, name, env, taken):
    d, args, want = test_3
    got, err = _run(d, BINARY, args, env)
    assert sorted(got) == want, name
    requests, climbed, unresolved, launches = _ladders(err)
    print("%s: %d ladder requests, %d with attempts >= 2, %d with a failed last rung, %d ladder launches" % (name, requests, climbed, unresolved, launches))
    if taken:
        assert requests > 0 and climbed >= 12 and 0 < launches <= requests
    else:
        assert (requests, climbed, unresolved, launches) == (0, 0, 0, 0)


@pytest.mark.parametrize("name,env,taken", SWITCHES, ids=[s[0] for s in SWITCHES])
def test_split_reads_sam_identical_with_ladders(split_reads, name, env, taken):
    d, args, want = split_reads
    got, err = _run(d, BINARY, args, env)
    assert sorted(got) == want, name
    requests, climbed, unresolved, launches = _ladders(err)
    print("%s: %d ladder requests, %d with attempts >= 2, %d with a failed last rung, %d ladder launches" % (name, requests, climbed, unresolved, launches))
    assert (requests > 0) == taken


def test_nosse_ladders_on_the_scalar_twin(built, tmp_path):
    args = ["-x", "pacbio", "-t", "1", "--nosse", "-r", os.path.join(E2E, "test_4_reference.fasta.gz"), "-q", os.path.join(E2E, "test_4_read.fa.gz")]
    want, _ = _run(tmp_path, REF, args)
    got, err = _run(tmp_path, BINARY, args)
    assert len(want) == 1 and got == want
    assert _ladders(err)[0] > 0
