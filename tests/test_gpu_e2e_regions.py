"""GPU (-m gpu): detectMisalignment on the regions the device found, end to end (oracle/_ref/ngmlr_hip_regions =
ngmlr_hip_all + nm_regions_alloc_binding.inc + nm_regions_finder_binding.inc, tools/build_ngmlr_hip.sh): SharedAligner's
handles carry CVX_CREATE_NM_REGIONS, computeAlignment writes a request instead of allocating the nmPerPosition profile, Finish
answers it with the job's regions and the peak finder walks them.  Every SAM record must equal the unmodified reference's, with
the binding on and with CVX_DEVICE_REGIONS=0 inside the same binary."""
import gzip
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
E2E = os.path.join(GOLDEN, "e2e")
BINARY = os.path.join(ROOT, "oracle", "_ref", "ngmlr_hip_regions")
REF = os.path.join(ROOT, "oracle", "_ref", "ngmlr_ref")
LINE = re.compile(r"SharedAligner: (\d+) alignments handed detectMisalignment (\d+) regions from the device, (\d+) their profile \(CVX_DEVICE_REGIONS=0 turns that off\)")


def _records(text):
    return [l.rstrip("\n") for l in text.splitlines() if l.strip() and not l.startswith("@")]


def _run(tmp_path, binary, args, switch=None, extra_env=None):
    if not os.path.exists(binary):
        pytest.skip("%s not built (tools/build_ngmlr_hip.sh needs /root/reference)" % os.path.relpath(binary, ROOT))
    env = dict(os.environ, CVX_POOL_CONTEXTS="128")
    env.pop("CVX_DEVICE_REGIONS", None)
    if switch is not None:
        env["CVX_DEVICE_REGIONS"] = switch
    env.update(extra_env or {})
    res = subprocess.run([binary, "--skip-write"] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                         timeout=600, cwd=str(tmp_path), env=env)
    assert res.returncode == 0, res.stderr[-3000:]
    return _records(res.stdout), res.stderr


def _check(tmp_path, args, want):
    got, err = _run(tmp_path, BINARY, args)
    assert sorted(got) == want, "binding on"
    m = LINE.search(err)
    assert m, err[-2000:]
    n, r, profiles = (int(x) for x in m.groups())
    print("on: %d alignments handed %d regions, %d their profile" % (n, r, profiles))
    assert n > 0 and r >= 10 and profiles == 0
    got, err = _run(tmp_path, BINARY, args, switch="0")
    assert sorted(got) == want, "CVX_DEVICE_REGIONS=0"
    m = LINE.search(err)
    assert m is None or (int(m.group(1)) == 0 and int(m.group(2)) == 0), err[-2000:]
    # the device text stage has no regions: every request ends as a full profile, in a buffer as long as the rows the finder's
    # loop scans (it was a few dozen rows when the request was written), and the reference's loop runs over it
    got, err = _run(tmp_path, BINARY, args, extra_env={"CVX_DEVICE_TEXT": "1"})
    assert sorted(got) == want, "CVX_DEVICE_TEXT=1"
    m = LINE.search(err)
    assert m and int(m.group(1)) == 0 and int(m.group(3)) == n, err[-2000:]
    assert "text stage on the device" in err


def test_test_3_sam_identical_on_the_devices_regions(built, tmp_path):
    fq = os.path.join(str(tmp_path), "test_3.fq")
    with gzip.open(os.path.join(E2E, "test_3_reads.fq.gz"), "rb") as f, open(fq, "wb") as o:
        o.write(f.read())
    args = ["-x", "pacbio", "-t", "8", "-R", "0.01", "--no-progress", "-r", os.path.join(E2E, "test_3_reference.fasta.gz"), "-q", fq]
    with gzip.open(os.path.join(GOLDEN, "test_3.sorted.sam.gz"), "rt") as f:
        want = [l.rstrip("\n") for l in f if l.strip() and not l.startswith("@")]
    assert len(want) > 200
    _check(tmp_path, args, want)


def test_split_reads_sam_identical_on_the_devices_regions(built, tmp_path):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import e2e_rates
    fa, fq = str(tmp_path / "sv_ref.fa"), str(tmp_path / "sv_reads.fq")
    e2e_rates.write_sv_workload(fa, fq, 12, seed=78, L=1_000_000)
    args = ["-x", "ont", "-t", "8", "-R", "0.01", "--no-progress", "-r", fa, "-q", fq]
    want, _ = _run(tmp_path, REF, args)
    assert len(want) >= 12 and any(int(l.split("\t")[1]) & 2048 for l in want)          # split reads among them
    _check(tmp_path, args, sorted(want))
