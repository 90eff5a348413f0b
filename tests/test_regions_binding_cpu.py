"""CPU: detectMisalignment on the regions the aligner found, inside the reference's own binary, without a GPU
(oracle/_ref/ngmlr_regions_cpu, tools/build_ngmlr_hip.sh): computeAlignment writes a request instead of allocating the
nmPerPosition profile (nm_regions_alloc_binding.inc), the reference's CPU aligner behind tests/cpp/regions_cpu_aligner.h answers
it with a note (nm_regions_note.h), and the peak finder's loop walks the note (nm_regions_finder_binding.inc).  Every SAM record
must equal the unmodified reference's, with the binding on and with CVX_DEVICE_REGIONS=0; with it on the exit lines show the
regions walked and no violation of what the device finder assumes about the profile's rows past its entries."""
import gzip
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
E2E = os.path.join(GOLDEN, "e2e")
BINARY = os.path.join(ROOT, "oracle", "_ref", "ngmlr_regions_cpu")
REF = os.path.join(ROOT, "oracle", "_ref", "ngmlr_ref")
SV_READS = 4       # split-read workload (seed 78): small, and its alignments still walk far more than ten regions

needs_binary = pytest.mark.skipif(not os.path.exists(BINARY), reason="oracle/_ref/ngmlr_regions_cpu not built (tools/build_ngmlr_hip.sh needs /root/reference)")


def _records(text):
    return [l.rstrip("\n") for l in text.splitlines() if l.strip() and not l.startswith("@")]


def _run(tmp_path, binary, args, switch=None):
    env = dict(os.environ)
    env.pop("CVX_DEVICE_REGIONS", None)
    if switch is not None:
        env["CVX_DEVICE_REGIONS"] = switch
    res = subprocess.run([binary, "--skip-write"] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                         timeout=900, cwd=str(tmp_path), env=env)
    assert res.returncode == 0, res.stderr[-2000:]
    return _records(res.stdout), res.stderr


def _exit_lines(err):
    """-> (notes, regions in them, calls answered with a profile, (violations), alignments walked as notes, regions walked, scanned as profiles)"""
    m = re.search(r"RegionsCpuAligner: (\d+) calls answered with a note \((\d+) regions\), (\d+) with their profile; violations: (\d+) profiles with a "
                  r"row past their entries that is not zero, (\d+) buffers written twice, (\d+) alignments longer than their buffer", err)
    w = re.search(r"RegionsCpuAligner: (\d+) alignments handed detectMisalignment (\d+) regions from their note, (\d+) their profile", err)
    assert m and w, err[-1500:]
    g = [int(x) for x in m.groups()]
    return g[0], g[1], g[2], tuple(g[3:]), int(w.group(1)), int(w.group(2)), int(w.group(3))


def _check(got_on, err_on, got_off, err_off, want):
    assert sorted(got_on) == want, "binding on"
    assert sorted(got_off) == want, "CVX_DEVICE_REGIONS=0"
    notes, regions, profiles, violations, walked, walked_regions, scanned = _exit_lines(err_on)
    print("on: %d notes of %d regions, %d profile calls, violations %s; finder: %d notes with %d regions, %d profiles" % (
        notes, regions, profiles, violations, walked, walked_regions, scanned))
    assert violations == (0, 0, 0)
    assert notes > 0 and profiles == 0 and walked > 0 and scanned == 0
    assert walked_regions >= 10
    notes, regions, profiles, violations, walked, walked_regions, scanned = _exit_lines(err_off)
    assert notes == 0 and profiles > 0 and walked == 0 and walked_regions == 0 and scanned > 0


@needs_binary
def test_test_3_sam_identical_with_notes_and_with_profiles(tmp_path):
    fq = os.path.join(str(tmp_path), "test_3.fq")
    with gzip.open(os.path.join(E2E, "test_3_reads.fq.gz"), "rb") as f, open(fq, "wb") as o:
        o.write(f.read())
    args = ["-x", "pacbio", "-t", "4", "-R", "0.01", "--no-progress", "-r", os.path.join(E2E, "test_3_reference.fasta.gz"), "-q", fq]
    with gzip.open(os.path.join(GOLDEN, "test_3.sorted.sam.gz"), "rt") as f:
        want = [l.rstrip("\n") for l in f if l.strip() and not l.startswith("@")]
    assert len(want) > 200
    on = _run(tmp_path, BINARY, args)
    off = _run(tmp_path, BINARY, args, switch="0")
    _check(on[0], on[1], off[0], off[1], want)


@needs_binary
@pytest.mark.skipif(not os.path.exists(REF), reason="oracle/_ref/ngmlr_ref not built (tools/build_ngmlr_hip.sh needs /root/reference)")
def test_split_reads_sam_identical_with_notes_and_with_profiles(tmp_path):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import e2e_rates
    fa, fq = str(tmp_path / "sv_ref.fa"), str(tmp_path / "sv_reads.fq")
    e2e_rates.write_sv_workload(fa, fq, SV_READS, seed=78, L=1_000_000)
    args = ["-x", "ont", "-t", "8", "-R", "0.01", "--no-progress", "-r", fa, "-q", fq]
    want, _ = _run(tmp_path, REF, args)
    assert len(want) >= SV_READS
    on = _run(tmp_path, BINARY, args)
    off = _run(tmp_path, BINARY, args, switch="0")
    _check(on[0], on[1], off[0], off[1], sorted(want))


@needs_binary
@pytest.mark.skipif(not os.path.exists(REF), reason="oracle/_ref/ngmlr_ref not built (tools/build_ngmlr_hip.sh needs /root/reference)")
def test_nosse_keeps_the_profile(tmp_path):
    """--nosse constructs the reference's scalar aligner, which the wrapper does not stand in front of and which knows no request:
    the binding is not announced, the reference's allocation and loop run, no note is written or walked."""
    args = ["-x", "pacbio", "-t", "1", "--nosse", "-r", os.path.join(E2E, "test_4_reference.fasta.gz"), "-q", os.path.join(E2E, "test_4_read.fa.gz")]
    want, _ = _run(tmp_path, REF, args)
    got, err = _run(tmp_path, BINARY, args)
    assert len(want) == 1 and got == want
    assert "RegionsCpuAligner:" not in err      # the wrapper was never constructed, so it has no exit lines
