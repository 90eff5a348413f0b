"""GPU (-m gpu): the low-identity regions of the NM profile found on the device (cvx_job_nm_regions, cvx_nm_regions_ops:
nm_regions_kernel) against the loop at the top of detectMisalignment written out literally (tests/nm_region_cases.literal_scan)
over the profile -- the reference aligner's own, the recorded reference output, and the device's own nm_profile padded with
zeros to alignmentLength -- region by region and with the state the loop ends in."""
import numpy as np
import pytest

from tests import nm_region_cases as cases
from tests import util

pytestmark = pytest.mark.gpu


def _job(al, tiles):
    job = al.submit(tiles)
    job.wait()
    eqs = np.array([t.ext_qstart for t in tiles], dtype=np.int32)
    eqe = np.array([t.ext_qend for t in tiles], dtype=np.int32)
    return job, job.text(eqs, eqe)


def _device_regions(job, n, ranges):
    """-> per tile (regions int32[r, 4], open record) from cvx_job_nm_regions over `ranges`"""
    out = [None] * n
    for first, count in ranges:
        off, reg, opn, ms = job.nm_regions(first, count)
        assert ms >= 0.0 and off[0] == 0 and int(off[count]) == len(reg) and len(opn) == count
        assert (np.diff(off.astype(np.int64)) >= 0).all()
        for i in range(count):
            out[first + i] = (reg[int(off[i]):int(off[i + 1])], opn[i])
    assert all(o is not None for o in out)
    return out


def _check(tiles, dev, got, profile_of):
    """got[i] against the literal scan over profile_of(i) -> (triples, alignment_length) or None for "no valid alignment";
    -> (valid tiles, regions, open runs)"""
    valid = regions = opens = 0
    for i, t in enumerate(tiles):
        p = profile_of(i)
        reg, opn = got[i]
        if p is None:
            assert dev[i]["ret"] < 0 and len(reg) == 0 and cases.same(([], (0, 20, (-1, -1, -1, -1))), reg, opn) is None, t.tag
            continue
        tri, al = p
        assert dev[i]["ret"] >= 0 and dev[i]["alignment_length"] == al, t.tag
        want = cases.literal_scan(cases.padded(tri, al), al)
        diff = cases.same(want, reg, opn)
        assert diff is None, (t.tag, diff)
        valid += 1
        regions += len(want[0])
        opens += want[1][0]
    return valid, regions, opens


_CACHE = {}


def _zoo():
    from tests.test_gpu_parity import _sv_tile
    rng = np.random.default_rng(77)
    tiles = util.tile_zoo(seed=67, n=70, max_w=2000) + util.edge_tiles()
    tiles.append(_sv_tile(rng, 900, [70, 130], [65, 200], "full"))
    tiles.append(_sv_tile(rng, 700, [1, 2, 3, 33], [1, 2, 64], "endpoints"))
    tiles.append(_sv_tile(rng, 600, [31, 32, 33], [31, 32, 33], "full"))
    return tiles + cases.stretch_tiles(30) + cases.clean_tiles(4) + cases.tail_tiles(20)


@pytest.mark.parametrize("split", ["whole", "ranges"])
def test_job_regions_equal_the_literal_scan(hip_aligner, ref_oracle, split):
    """A whole job at once, and in tile ranges, against the scan over (a) the reference aligner's own profile (oracle/_ref)
    and (b) the device's nm_profile of the same job padded with zeros to alignment_length."""
    tiles = _zoo()
    n = len(tiles)
    ranges = [(0, n)] if split == "whole" else [(0, 7), (7, n - 20), (n - 13, 13)]
    job, dev = _job(hip_aligner, tiles)
    got = _device_regions(job, n, ranges)
    off, tri, _ = job.nm_profile(0, n)
    # asking again for a range gives the same answer (the buffers are the job's, the call has no memory)
    again = _device_regions(job, n, ranges)
    assert all(np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes() for a, b in zip(got, again))
    job.release()
    if "want" not in _CACHE:      # (the same tiles for both splits: one pass of the CPU aligner)
        _CACHE["want"] = [ref_oracle.align(t) for t in tiles]
    want = _CACHE["want"]
    a = _check(tiles, dev, got, lambda i: None if want[i]["ret"] < 0 else (want[i]["nm_per_position"], want[i]["alignment_length"]))
    b = _check(tiles, dev, got, lambda i: None if dev[i]["ret"] < 0 else (tri[int(off[i]):int(off[i + 1])], dev[i]["alignment_length"]))
    assert a == b
    valid, regions, opens = a
    assert valid >= 40 and regions >= 100 and opens >= 5 and valid < n, (valid, regions, opens, n)


@pytest.mark.parametrize("name", ["ref_test_2.npz", "ref_test_4.npz", "ref_test_3.npz"])
def test_job_regions_on_recorded_reference_profiles(hip_aligner, name):
    """The scan over the nmPerPosition rows the unmodified reference wrote for its own SingleAlign calls."""
    pairs = util.load_golden(name)
    tiles = [t for t, _ in pairs]
    job, dev = _job(hip_aligner, tiles)
    got = _device_regions(job, len(tiles), [(0, len(tiles))])
    job.release()
    valid, regions, _ = _check(tiles, dev, got, lambda i: None if pairs[i][1]["ret"] < 0 else (pairs[i][1]["nm_per_position"], pairs[i][1]["alignment_length"]))
    assert valid > 0
    if name == "ref_test_3.npz":
        assert regions == 64


def test_regions_of_arbitrary_op_lists(hip_aligner):
    """cvx_nm_regions_ops on every engineered family against the scan over cvx_nm_profile_ops' triples of the same lists,
    and the answers of the entry to too little room, to a NULL buffer and to ops outside the arena."""
    lib = hip_aligner.lib
    cs = cases.engineered()
    res, arena = cases.pack_ops(cs)
    n = len(cs)
    eoff = np.zeros(n + 1, dtype=np.uint64)
    assert lib.cvx_nm_profile_ops(hip_aligner.h, n, res, arena.ctypes.data, len(arena), eoff.ctypes.data, None, 0) == 0
    tri = np.zeros((int(eoff[-1]), 3), dtype=np.int32)
    assert lib.cvx_nm_profile_ops(hip_aligner.h, n, res, arena.ctypes.data, len(arena), eoff.ctypes.data, tri.ctypes.data, len(tri)) == 0
    off, reg, opn = hip_aligner.nm_regions_ops(res, arena)
    assert off[0] == 0 and int(off[n]) == len(reg)
    regions = opens = none = 0
    for i, c in enumerate(cs):
        al = sum(ln for ln, _ in c["ops"]) if c["status"] == 0 else 0
        rows = cases.padded(tri[int(eoff[i]):int(eoff[i + 1])], al)
        want = cases.literal_scan(rows, al)
        cases.check_expectations(c, rows, want)
        diff = cases.same(want, reg[int(off[i]):int(off[i + 1])], opn[i])
        assert diff is None, (c["tag"], diff)
        regions += len(want[0])
        opens += want[1][0]
        none += not want[0]
    assert regions > 300 and opens >= 5 and none >= 5, (regions, opens, none)
    # sizes only: the offsets and the end states, no regions asked for
    off2, none_, opn2 = hip_aligner.nm_regions_ops(res, arena, want_regions=False)
    assert none_ is None and np.array_equal(off, off2) and opn.tobytes() == opn2.tobytes()
    # too little room: CVX_ERR_CAPACITY, the offsets filled in, nothing written
    off3 = np.zeros(n + 1, dtype=np.uint64)
    small = np.full((2, 4), -7, dtype=np.int32)
    assert lib.cvx_nm_regions_ops(hip_aligner.h, n, res, arena.ctypes.data, len(arena), off3.ctypes.data, small.ctypes.data, 2, None) == -6
    assert np.array_equal(off, off3) and (small == -7).all()
    # ops outside the arena, NULL offsets
    assert lib.cvx_nm_regions_ops(hip_aligner.h, 1, res, arena.ctypes.data, 3, off3.ctypes.data, None, 0, None) == -3
    assert lib.cvx_nm_regions_ops(hip_aligner.h, n, res, arena.ctypes.data, len(arena), None, None, 0, None) == -3
    assert lib.cvx_nm_regions_ops(hip_aligner.h, 0, None, None, 0, None, None, 0, None) == 0


def test_job_regions_refuse_what_nm_profile_refuses(hip_aligner):
    import ctypes as C
    lib, h = hip_aligner.lib, hip_aligner.h
    tiles = cases.stretch_tiles(4, seed=9)
    job = hip_aligner.submit(tiles)
    off = np.zeros(5, dtype=np.uint64)
    ptr = C.c_void_p()
    assert lib.cvx_job_nm_regions(h, job.j, 0, 4, off.ctypes.data, C.byref(ptr), None, None) == -3      # not waited for
    job.wait()
    assert lib.cvx_job_nm_regions(h, job.j, 0, 4, off.ctypes.data, C.byref(ptr), None, None) == -3      # no text stage yet
    assert lib.cvx_job_nm_profile(h, job.j, 0, 4, off.ctypes.data, None, 0, None) == -3
    job.text()
    assert lib.cvx_job_nm_regions(h, job.j, 2, 3, off.ctypes.data, C.byref(ptr), None, None) == -3      # range past the job
    assert lib.cvx_job_nm_profile(h, job.j, 2, 3, off.ctypes.data, None, 0, None) == -3
    assert lib.cvx_job_nm_regions(h, job.j, -1, 2, off.ctypes.data, C.byref(ptr), None, None) == -3
    assert lib.cvx_job_nm_regions(h, job.j, 0, 4, None, C.byref(ptr), None, None) == -3
    assert lib.cvx_job_nm_regions(h, job.j, 0, 4, off.ctypes.data, None, None, None) == -3
    assert lib.cvx_job_nm_regions(h, None, 0, 4, off.ctypes.data, C.byref(ptr), None, None) == -3
    assert lib.cvx_job_nm_regions(h, job.j, 4, 0, None, C.byref(ptr), None, None) == 0                  # an empty range is fine
    # no open records, no timing asked for: still the regions
    assert lib.cvx_job_nm_regions(h, job.j, 0, 4, off.ctypes.data, C.byref(ptr), None, None) == 0
    off2, reg, _opn, _ms = job.nm_regions()
    assert np.array_equal(off, off2) and len(reg) == int(off[4]) > 0
    job.release()


def test_whole_job_of_2048_long_reads(hip_aligner):
    """One job of 2 048 PacBio 10 kb tiles asked for as a whole -- its profile would be some 250 MB of triples, which
    cvx_job_nm_profile takes in ranges only -- and 64 of its tiles against the scan over the profile path."""
    from ngmlr_amd import synth
    ts = synth.pacbio_tileset(2048, seed=12)
    job = hip_aligner.submit(ts)
    job.wait()
    dev, _off, _buf = job.text_raw()
    n = len(ts)
    off, reg, opn, ms = job.nm_regions()
    assert len(off) == n + 1 and int(off[n]) == len(reg) and ms > 0.0
    entries = sum(dev[i].nm_count for i in range(n) if dev[i].ret >= 0)
    assert 16 * len(reg) * 100 < 12 * entries                  # what comes back against what the triples would be
    checked = regions = 0
    for first in range(0, n, 256):
        poff, tri, _ = job.nm_profile(first, 8)
        for i in range(8):
            t = first + i
            if dev[t].ret < 0:
                assert off[t + 1] == off[t]
                continue
            al = dev[t].alignment_length
            want = cases.literal_scan(cases.padded(tri[int(poff[i]):int(poff[i + 1])], al), al)
            diff = cases.same(want, reg[int(off[t]):int(off[t + 1])], opn[t])
            assert diff is None, (t, diff)
            checked += 1
            regions += len(want[0])
    job.release()
    assert checked >= 60 and regions > 0
