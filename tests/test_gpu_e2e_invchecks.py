"""GPU (-m gpu): checkForSV on the scores its job brought, end to end (oracle/_ref/ngmlr_hip_invchecks = ngmlr_hip_regions + the
two insertions of inv_checks_binding.inc and nm_regions_finder_binding.inc, tools/build_ngmlr_hip.sh): SharedAligner's handles
carry CVX_CREATE_INV_CHECKS, Finish writes the checks form of the note, the finder's walk offers region k's record to the
checkForSV call of region k.  Every SAM record must equal the unmodified reference's under every switch that bears on it, and the
binding's exit line must show what was taken: at least the 497 scored calls the reference's recording holds on test_3
(tests/golden/inv_checks_test_3.npz), nothing through checkForSV's own scoring for a missing window or an inconsistent record,
every taken check verified without a disagreement under CVX_INV_CHECKS_VERIFY=1, none taken where the binding is off, where the
windows are decoded on the host (CVX_DEVICE_DECODE=0: notes without checks, counted) and under --stdout 4, whose FASTA records only
the reference's scoring path prints."""
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
BINARY = os.path.join(ROOT, "oracle", "_ref", "ngmlr_hip_invchecks")
REF = os.path.join(ROOT, "oracle", "_ref", "ngmlr_ref")
LINE = re.compile(r"DeviceInvChecks: (\d+) checks taken from the job \((\d+) scored, (\d+) without a read part\), (\d+) through checkForSV's own scoring "
                  r"\((\d+) no window, (\d+) inconsistent record, (\d+) note without checks\), (\d+) verified, (\d+) disagreements")
KNOBS = ("CVX_DEVICE_INV_CHECKS", "CVX_INV_CHECKS_VERIFY", "CVX_JOB_TEXT", "CVX_DEVICE_DECODE", "CVX_DEVICE_REGIONS", "CVX_DEVICE_TEXT")
SWITCHES = [("default", {}), ("CVX_DEVICE_INV_CHECKS=0", {"CVX_DEVICE_INV_CHECKS": "0"}), ("CVX_INV_CHECKS_VERIFY=1", {"CVX_INV_CHECKS_VERIFY": "1"}),
            ("CVX_JOB_TEXT=1", {"CVX_JOB_TEXT": "1"}), ("CVX_DEVICE_DECODE=0", {"CVX_DEVICE_DECODE": "0"}), ("CVX_DEVICE_REGIONS=0", {"CVX_DEVICE_REGIONS": "0"})]


def _records(text):
    return [l.rstrip("\n") for l in text.splitlines() if l.strip() and not l.startswith("@")]


def _run_raw(cwd, binary, args, extra_env=None):
    if not os.path.exists(binary):
        pytest.skip("%s not built (tools/build_ngmlr_hip.sh needs /root/reference)" % os.path.relpath(binary, ROOT))
    env = dict(os.environ, CVX_POOL_CONTEXTS="128")
    for k in KNOBS:
        env.pop(k, None)
    env.update(extra_env or {})
    res = subprocess.run([binary, "--skip-write"] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                         timeout=600, cwd=str(cwd), env=env)
    assert res.returncode == 0, res.stderr[-3000:]
    return res.stdout, res.stderr


def _run(cwd, binary, args, extra_env=None):
    out, err = _run_raw(cwd, binary, args, extra_env)
    return _records(out), err


def _exit_line(err):
    lines = LINE.findall(err)
    assert len(lines) == 1, err[-2000:]
    return dict(zip("NSRFabcVD", (int(x) for x in lines[0])))


def _check_line(name, c, min_scored):
    print("%s: %s" % (name, c))
    assert c["N"] == c["S"] + c["R"] and c["F"] == c["a"] + c["b"] + c["c"]
    if name in ("default", "CVX_JOB_TEXT=1"):
        assert c["S"] >= min_scored and c["a"] == 0 and c["b"] == 0 and c["V"] == 0 and c["D"] == 0
    elif name == "CVX_INV_CHECKS_VERIFY=1":
        assert c["S"] >= min_scored and c["a"] == 0 and c["b"] == 0 and c["D"] == 0 and c["V"] == c["N"]
    elif name == "CVX_DEVICE_DECODE=0":
        assert c["N"] == 0 and c["c"] > 0 and c["a"] == 0 and c["b"] == 0
    else:
        assert c["N"] == 0 and c["F"] == 0 and c["V"] == 0


@pytest.fixture(scope="module")
def test_3(built, tmp_path_factory):
    d = tmp_path_factory.mktemp("invchecks_test_3")
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
    d = tmp_path_factory.mktemp("invchecks_split")
    fa, fq = str(d / "sv_ref.fa"), str(d / "sv_reads.fq")
    e2e_rates.write_sv_workload(fa, fq, 12, seed=78, L=1_000_000)
    args = ["-x", "ont", "-t", "8", "-R", "0.01", "--no-progress", "-r", fa, "-q", fq]
    want, _ = _run(d, REF, args)
    assert len(want) >= 12 and any(int(l.split("\t")[1]) & 2048 for l in want)          # split reads among them
    return d, args, sorted(want)


@pytest.mark.parametrize("name,env", SWITCHES, ids=[s[0] for s in SWITCHES])
def test_test_3_sam_identical_with_checks_from_the_job(test_3, name, env):
    d, args, want = test_3
    got, err = _run(d, BINARY, args, env)
    assert sorted(got) == want, name
    # the reference's recording holds 497 distinct scored calls and no NO_WINDOW
    _check_line(name, _exit_line(err), 497)


@pytest.mark.parametrize("name,env", SWITCHES, ids=[s[0] for s in SWITCHES])
def test_split_reads_sam_identical_with_checks_from_the_job(split_reads, name, env):
    d, args, want = split_reads
    got, err = _run(d, BINARY, args, env)
    assert sorted(got) == want, name
    _check_line(name, _exit_line(err), 1)


def _fasta_records(out):
    """stdout under --stdout 4 with the SAM in a file: nothing but the two-line FASTA records checkForSV prints"""
    lines = out.splitlines()
    assert len(lines) % 2 == 0 and all(l.startswith(">") for l in lines[0::2]) and not any(l.startswith(">") for l in lines[1::2])
    return sorted(zip(lines[0::2], lines[1::2]))


def test_stdout_4_prints_the_references_candidates(test_3):
    """The SAM goes to a file (-o) on either side: the reference writes its SAM buffer with fwrite_unlocked (src/PlainFileWriter.h:44)
    while checkForSV's printf takes the stream's lock, so with both on stdout and several threads its own output can lose or tear
    records from run to run.  Each FASTA record is one printf, so stdout alone is whole records in some order."""
    d, args, want = test_3
    want_out, _ = _run_raw(d, REF, ["--stdout", "4", "-o", "ref_stdout4.sam"] + args)
    got_out, err = _run_raw(d, BINARY, ["--stdout", "4", "-o", "got_stdout4.sam"] + args)
    want_fa, got_fa = _fasta_records(want_out), _fasta_records(got_out)
    assert len(want_fa) == 2 * 497      # /1 the window, /2 the reversed read part of each of the recording's scored calls
    assert got_fa == want_fa
    for name in ("ref_stdout4.sam", "got_stdout4.sam"):
        with open(os.path.join(str(d), name)) as f:
            assert sorted(_records(f.read())) == want, name
    c = _exit_line(err)
    print("--stdout 4: %s" % c)
    assert c["N"] == 0 and c["F"] == 0
