"""CPU: computeAlignment's retry loop handed over as one request, inside the reference's own binary, without a GPU
(oracle/_ref/ngmlr_ladder_cpu, tools/build_ngmlr_hip.sh): ladder_binding.inc in front of the loop fills a cvx_ladder
(ladder_binding_logic.h), finds Convex::LadderAligner with dynamic_cast and the reference's CPU aligner behind
tests/cpp/ladder_cpu_aligner.h climbs with cvx_ladder_rung's rule.  Every SAM record must equal the unmodified reference's, with
the binding on and with CVX_DEVICE_LADDER=0; and the calls the binding makes (CVX_LADDER_DUMP) -- corridor before the clamp,
lengths, the four flags, fullReadLength, the bits of left / right where the anchors builder runs, the attempts -- must be the
set of distinct calls recorded from the unmodified reference (tests/golden/ladder_*.npz, tools/make_golden_ladder.sh)."""
import gzip
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
E2E = os.path.join(GOLDEN, "e2e")
BINARY = os.path.join(ROOT, "oracle", "_ref", "ngmlr_ladder_cpu")
REF = os.path.join(ROOT, "oracle", "_ref", "ngmlr_ref")
SV_READS = 4       # split-read workload (seed 78), as tests/test_regions_binding_cpu.py

needs_binary = pytest.mark.skipif(not os.path.exists(BINARY), reason="oracle/_ref/ngmlr_ladder_cpu not built (tools/build_ngmlr_hip.sh needs /root/reference)")
needs_ref = pytest.mark.skipif(not os.path.exists(REF), reason="oracle/_ref/ngmlr_ref not built (tools/build_ngmlr_hip.sh needs /root/reference)")
LINE = re.compile(r"LadderCpuAligner: (\d+) ladder requests, (\d+) with attempts >= 2, (\d+) reported a failed last rung")
ANCHORS, REALIGN, SHORT, FULL = 1, 2, 4, 8


def _records(text):
    return [l.rstrip("\n") for l in text.splitlines() if l.strip() and not l.startswith("@")]


def _run(tmp_path, binary, args, switch=None, dump=None):
    env = dict(os.environ)
    env.pop("CVX_DEVICE_LADDER", None)
    env.pop("CVX_LADDER_DUMP", None)
    if switch is not None:
        env["CVX_DEVICE_LADDER"] = switch
    if dump is not None:
        env["CVX_LADDER_DUMP"] = dump
    res = subprocess.run([binary, "--skip-write"] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                         timeout=900, cwd=str(tmp_path), env=env)
    assert res.returncode == 0, res.stderr[-2000:]
    return _records(res.stdout), res.stderr


def _requests(err):
    m = LINE.search(err)
    assert m, err[-1500:]
    return tuple(int(x) for x in m.groups())


def _test_3(tmp_path, threads):
    fq = os.path.join(str(tmp_path), "test_3.fq")
    with gzip.open(os.path.join(E2E, "test_3_reads.fq.gz"), "rb") as f, open(fq, "wb") as o:
        o.write(f.read())
    return ["-x", "pacbio", "-t", str(threads), "-R", "0.01", "--no-progress", "-r", os.path.join(E2E, "test_3_reference.fasta.gz"), "-q", fq]


def _bits(x):
    return struct.unpack("<I", struct.pack("<f", float(x)))[0]


def _recorded(name):
    """the fixture's distinct calls, projected: (corridor, read_length, ref_len, anchors, realign, short, full, full_read_length,
    n_attempts, have_lr, left bits, right bits) -- the floats only where the reference's builder computed them"""
    calls = np.load(os.path.join(GOLDEN, name))["calls"]
    out = set()
    for c in calls:
        lr = bool(c["have_lr"])
        out.add((int(c["corridor"]), int(c["read_length"]), int(c["ref_len"]), int(c["anchor_length"] > 0), int(c["realign"]), int(c["short_read"]), int(c["full"]),
                 int(c["full_read_length"]), int(c["n_attempts"]), int(lr), _bits(c["left"]) if lr else 0, _bits(c["right"]) if lr else 0))
    return calls, out


def _dumped(path):
    """the binding's calls as ladder_cpu_aligner.h dumps them, projected the same way (ref_len there is the string's length: the
    recorder's refSeqLen is one more)"""
    out = set()
    with open(path) as f:
        for line in f:
            corridor, flags, lb, rb, ref_len, qry_len, full_read_length, attempts = line.split()
            flags = int(flags)
            lr = bool(flags & ANCHORS) and not flags & (REALIGN | SHORT | FULL)      # the one case in which the loop calls the anchors builder
            out.add((int(corridor), int(qry_len), int(ref_len) + 1, int(bool(flags & ANCHORS)), int(bool(flags & REALIGN)), int(bool(flags & SHORT)), int(bool(flags & FULL)),
                     int(full_read_length), int(attempts), int(lr), int(lb, 16) if lr else 0, int(rb, 16) if lr else 0))
    return out


@needs_binary
def test_test_3_sam_identical_with_the_ladder_and_with_the_loop(tmp_path):
    args = _test_3(tmp_path, 4)
    with gzip.open(os.path.join(GOLDEN, "test_3.sorted.sam.gz"), "rt") as f:
        want = [l.rstrip("\n") for l in f if l.strip() and not l.startswith("@")]
    assert len(want) > 200
    got, err = _run(tmp_path, BINARY, args)
    assert sorted(got) == want, "binding on"
    requests, climbed, unresolved = _requests(err)
    print("on: %d ladder requests, %d climbed, %d unresolved" % (requests, climbed, unresolved))
    assert requests >= 826 and climbed >= 12
    got, err = _run(tmp_path, BINARY, args, switch="0")
    assert sorted(got) == want, "CVX_DEVICE_LADDER=0"
    assert _requests(err) == (0, 0, 0)


@needs_binary
@needs_ref
def test_split_reads_sam_identical_with_the_ladder_and_with_the_loop(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import e2e_rates
    fa, fq = str(tmp_path / "sv_ref.fa"), str(tmp_path / "sv_reads.fq")
    e2e_rates.write_sv_workload(fa, fq, SV_READS, seed=78, L=1_000_000)
    args = ["-x", "ont", "-t", "8", "-R", "0.01", "--no-progress", "-r", fa, "-q", fq]
    want, _ = _run(tmp_path, REF, args)
    assert len(want) >= SV_READS
    got, err = _run(tmp_path, BINARY, args)
    assert sorted(got) == sorted(want), "binding on"
    assert _requests(err)[0] > 0
    got, err = _run(tmp_path, BINARY, args, switch="0")
    assert sorted(got) == sorted(want), "CVX_DEVICE_LADDER=0"
    assert _requests(err) == (0, 0, 0)


@needs_binary
def test_test_3_calls_are_the_recorded_ones(tmp_path):
    """-t 1 and the recorder's arguments: what the binding puts into cvx_ladder, float bits included, is what the unmodified
    reference's loop and builder held"""
    calls, want = _recorded("ladder_test_3.npz")
    assert len(calls) == 826 and int((calls["n_attempts"] >= 2).sum()) == 12
    dump = str(tmp_path / "calls.txt")
    _run(tmp_path, BINARY, _test_3(tmp_path, 1), dump=dump)
    got = _dumped(dump)
    print("test_3: %d distinct calls dumped, %d recorded, %d only dumped, %d only recorded" % (len(got), len(want), len(got - want), len(want - got)))
    assert got == want, (sorted(got - want)[:5], sorted(want - got)[:5])
    assert sum(1 for c in got if c[8] >= 2) == 12 and any(c[9] for c in got)


@needs_binary
def test_split_read_calls_are_the_recorded_ones(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import e2e_rates
    calls, want = _recorded("ladder_split.npz")
    fa, fq = str(tmp_path / "sv_ref.fa"), str(tmp_path / "sv_reads.fq")
    e2e_rates.write_sv_workload(fa, fq, 160, seed=77, L=3_000_000)      # tools/make_golden_ladder.sh
    dump = str(tmp_path / "calls.txt")
    _run(tmp_path, BINARY, ["-x", "ont", "-t", "1", "-R", "0.01", "--no-progress", "-r", fa, "-q", fq], dump=dump)
    got = _dumped(dump)
    print("split reads: %d distinct calls dumped, %d recorded, %d only dumped, %d only recorded" % (len(got), len(want), len(got - want), len(want - got)))
    assert got == want, (sorted(got - want)[:5], sorted(want - got)[:5])
    assert any(c[9] for c in got)
