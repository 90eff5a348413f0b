"""GPU (-m gpu): the low-identity regions of a job delivered with its results (CVX_CREATE_NM_REGIONS, cvx_job_regions:
nm_regions_kernel<true>, the offset scan and nm_regions_bounded_kernel queued behind the job's compaction) -- region by region
and end state by end state against the loop at the top of detectMisalignment written out literally over the reference aligner's
own profile, and against cvx_job_nm_regions of the same tiles on a plain handle; the second walk, the rewrite over a grown arena,
empty and invalid jobs, windows, segments, the scalar twin and a reused job slot."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import nm_region_cases as cases
from tests import util

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def burst_tile(rng, length=3000, period=110, run=24, tag="bursts"):
    """A read without indels whose every `period`-th base starts `run` substituted bases: the alignment stays on the diagonal
    (24 mismatches cost 120, the 86 matches between two runs earn 172, two gaps of 24 would cost more), every run marks some
    40 rows and the 60 clean rows behind them close the region -- one region per period, 26 in 3 000 bases."""
    from ngmlr_amd import synth
    ref = synth.random_ref(rng, length)
    qry = ref.copy()
    for a in range(60, length - 60 - run, period):
        qry[a:a + run] = synth._ACGT[(synth._CODE[qry[a:a + run]].astype(np.int64) + 1) % 4]
    off, ln = synth.corridor_anchors(len(qry), length, mult=2, scatter_left=20.0, scatter_right=20.0)
    return synth.Tile(ref=ref.tobytes(), qry=qry.tobytes(), row_offset=off, row_length=ln, tag=tag)


def invalid_tiles(n=6):
    """no base of the read matches the window: the best score is 0, no alignment"""
    from ngmlr_amd import synth
    return [synth.Tile(b"A" * (200 + 37 * i), b"C" * (150 + 41 * i), *synth.corridor_anchors(150 + 41 * i, 200 + 37 * i), tag="invalid%d" % i)
            for i in range(n)]


def family_tiles():
    rng = np.random.default_rng(5)
    return (cases.stretch_tiles(30) + cases.clean_tiles(4) + cases.tail_tiles(20) + util.edge_tiles() + invalid_tiles()
            + [burst_tile(rng, tag="bursts%d" % i) for i in range(2)])


@pytest.fixture(scope="module")
def handles(built):
    from ngmlr_amd.aligner import ConvexAlignHip
    hs = {"plain": ConvexAlignHip(device=0), "regions": ConvexAlignHip(device=0, nm_regions=True),
          "twin": ConvexAlignHip(device=0, scalar_twin=True), "twin_regions": ConvexAlignHip(device=0, scalar_twin=True, nm_regions=True)}
    yield hs
    for al in hs.values():
        al.close()


def _plain(job, tiles=None):
    """wait, the device text stage, cvx_job_nm_regions of the whole job -> (results bytes, ops bytes, text, off, reg, open)"""
    res, ops = job.wait()
    rb, ob = res.tobytes(), ops.tobytes()
    eqs = np.array([t.ext_qstart for t in tiles], dtype=np.int32) if tiles else None
    eqe = np.array([t.ext_qend for t in tiles], dtype=np.int32) if tiles else None
    dev = job.text(eqs, eqe)
    off, reg, opn, _ms = job.nm_regions()
    job.release()
    return rb, ob, dev, off, reg, opn


def _with_results(job):
    """wait, cvx_job_regions -> (results bytes, ops bytes, off, reg, open, info)"""
    res, ops = job.wait()
    rb, ob = res.tobytes(), ops.tobytes()
    off, reg, opn = job.regions()
    info = job.regions_info()
    job.release()
    assert off[0] == 0 and int(off[-1]) == len(reg) == info["total"] and len(opn) == len(off) - 1
    assert (np.diff(off.astype(np.int64)) >= 0).all()
    return rb, ob, off, reg, opn, info


def _same_as_plain(want, got):
    """results and ops byte for byte, regions and end states entry for entry"""
    assert got[0] == want[0] and got[1] == want[1]
    assert np.array_equal(got[2], want[3]), "offsets"
    assert np.array_equal(got[3], want[4]), "regions"
    assert got[4].tobytes() == want[5].tobytes(), "end states"


@pytest.fixture(scope="module")
def family_run(handles):
    """the family tiles once through both handles, shared by the tests below"""
    tiles = family_tiles()
    want = _plain(handles["plain"].submit(tiles), tiles)
    got = _with_results(handles["regions"].submit(tiles))
    return tiles, want, got


def test_flag_is_accepted_and_misuse_refused(handles):
    from ngmlr_amd import capi
    lib = handles["plain"].lib
    p = handles["plain"].params
    for flags in (capi.CREATE_NM_REGIONS, capi.CREATE_NM_REGIONS | capi.CREATE_SCALAR_TWIN):
        h = C.c_void_p()
        assert lib.cvx_create_ex(0, C.byref(p), 0, flags, C.byref(h)) == 0
        lib.cvx_destroy(h)
    h = C.c_void_p()
    assert lib.cvx_create_ex(0, C.byref(p), 0, capi.CREATE_NM_REGIONS | capi.CREATE_SERVICE, C.byref(h)) == -3
    assert b"SERVICE" in lib.cvx_last_error() and not h.value
    assert lib.cvx_create_ex(0, C.byref(p), 0, 8, C.byref(h)) == -3
    tiles = cases.stretch_tiles(3, seed=4)
    po, pr, pn = C.c_void_p(), C.c_void_p(), C.c_void_p()
    # a plain handle's finished job
    job = handles["plain"].submit(tiles)
    job.wait()
    assert lib.cvx_job_regions(handles["plain"].h, job.j, C.byref(po), C.byref(pr), C.byref(pn)) == -3
    assert b"CVX_CREATE_NM_REGIONS" in lib.cvx_last_error() and not po.value
    assert lib.cvx_job_regions_info(handles["plain"].h, job.j, None, None, None) == -3
    job.release()
    # a job nobody has waited for
    al = handles["regions"]
    job = al.submit(tiles)
    assert lib.cvx_job_regions(al.h, job.j, C.byref(po), C.byref(pr), C.byref(pn)) == -3
    assert b"cvx_wait" in lib.cvx_last_error()
    assert lib.cvx_job_regions(al.h, None, C.byref(po), C.byref(pr), C.byref(pn)) == -3
    job.wait()
    assert lib.cvx_job_regions(al.h, job.j, C.byref(po), None, None) == 0 and po.value      # any output may be left out
    assert lib.cvx_job_regions(al.h, job.j, None, None, None) == 0
    job.release()


def test_regions_equal_the_plain_handles_entry(family_run):
    """... and the job's results and ops are a plain handle's, byte for byte"""
    tiles, want, got = family_run
    _same_as_plain(want, got)
    dev, off = want[2], got[2]
    n_valid = sum(d["ret"] >= 0 for d in dev)
    assert 40 <= n_valid < len(tiles)
    assert all(off[i + 1] == off[i] for i, d in enumerate(dev) if d["ret"] < 0)      # no valid alignment, no region
    assert got[5]["rewrites"] == 0 and got[5]["total"] <= got[5]["first_capacity"]
    assert int(got[4]["open"].sum()) >= 3


def test_regions_equal_the_literal_scan_of_the_reference_profile(family_run, ref_oracle):
    tiles, want, got = family_run
    dev, off, reg, opn = want[2], got[2], got[3], got[4]
    regions = opens = valid = 0
    for i, t in enumerate(tiles):
        w = ref_oracle.align(t)
        mine = reg[int(off[i]):int(off[i + 1])]
        if w["ret"] < 0:
            assert dev[i]["ret"] < 0 and cases.same(([], (0, 20, (-1, -1, -1, -1))), mine, opn[i]) is None, t.tag
            continue
        al = w["alignment_length"]
        scan = cases.literal_scan(cases.padded(w["nm_per_position"], al), al)
        diff = cases.same(scan, mine, opn[i])
        assert diff is None, (t.tag, diff)
        valid += 1
        regions += len(scan[0])
        opens += scan[1][0]
    assert valid >= 40 and regions >= 60 and opens >= 3, (valid, regions, opens)


def test_recorded_reference_profiles(handles):
    """ref_test_3.npz: the rows the unmodified reference wrote for its own SingleAlign calls; 64 regions"""
    pairs = util.load_golden("ref_test_3.npz")
    tiles = [t for t, _ in pairs]
    _rb, _ob, off, reg, opn, info = _with_results(handles["regions"].submit(tiles))
    assert info["total"] == 64
    for i, (t, exp) in enumerate(pairs):
        mine = reg[int(off[i]):int(off[i + 1])]
        if exp["ret"] < 0:
            assert len(mine) == 0, t.tag
            continue
        scan = cases.literal_scan(cases.padded(exp["nm_per_position"], exp["alignment_length"]), exp["alignment_length"])
        diff = cases.same(scan, mine, opn[i])
        assert diff is None, (t.tag, diff)


def test_job_of_one_tile_with_more_regions_than_the_stage(handles):
    """more than kNmStage = 16 regions in one tile: the write walks the tile a second time"""
    tile = [burst_tile(np.random.default_rng(31))]
    want = _plain(handles["plain"].submit(tile), tile)
    got = _with_results(handles["regions"].submit(tile))
    _same_as_plain(want, got)
    assert got[5]["total"] > 16 and got[5]["rewrites"] == 0


def test_more_regions_than_the_arena_was_sized_for(built):
    """40 tiles of 26 regions each against an arena sized for eight per tile: the write runs again over a larger arena while
    the ops are downloaded, and the job's second run in the same slot (the arena is large now) does without"""
    from ngmlr_amd.aligner import ConvexAlignHip
    rng = np.random.default_rng(32)
    tiles = [burst_tile(rng, length=int(rng.integers(2400, 3001)), tag="bursts%d" % i) for i in range(40)] + invalid_tiles(2)
    plain, al = ConvexAlignHip(device=0), ConvexAlignHip(device=0, nm_regions=True)
    try:
        want = _plain(plain.submit(tiles), tiles)
        got = _with_results(al.submit(tiles))
        _same_as_plain(want, got)
        info = got[5]
        assert info["rewrites"] == 1 and info["total"] > info["first_capacity"] >= 8 * len(tiles), info
        again = _with_results(al.submit(tiles))
        _same_as_plain(want, again)
        assert again[5]["rewrites"] == 0 and again[5]["first_capacity"] >= info["total"]
    finally:
        plain.close()
        al.close()


def test_empty_and_all_invalid_jobs(handles):
    al = handles["regions"]
    rb, ob, off, reg, opn, info = _with_results(al.submit([]))
    assert len(off) == 1 and len(reg) == 0 and len(opn) == 0 and info["total"] == 0
    tiles = invalid_tiles()
    want = _plain(handles["plain"].submit(tiles))
    got = _with_results(al.submit(tiles))
    _same_as_plain(want, got)
    assert all(d["ret"] < 0 for d in want[2]) and got[5]["total"] == 0 and not got[2].any()
    assert not got[4]["open"].any() and (got[4]["distance"] == 20).all() and (got[4]["region"] == -1).all()


def _with_bursts(rng, q):
    q = np.frombuffer(q, dtype=np.uint8).copy()
    from ngmlr_amd import synth
    for a in range(80, len(q) - 120, 300):
        q[a:a + 40] = synth.random_ref(rng, 40)
    return q.tobytes()


@pytest.mark.parametrize("twin", [False, True], ids=["default", "twin"])
def test_windows_and_segments(handles, twin):
    """cvx_submit_windows and cvx_submit_segments (with and without the resident genome) go through the same stages"""
    from ngmlr_amd import synth
    from ngmlr_amd.aligner import Genome
    from oracle.pyoracle import DecodeOracle
    from tests.segment_cases import embed_queries
    plain, al = (handles["twin"], handles["twin_regions"]) if twin else (handles["plain"], handles["regions"])
    z = np.load(os.path.join(ROOT, "tests", "golden", "decode_test_3.npz"))
    starts = [int(x) for x in z["starts"]]
    orc = DecodeOracle()
    rng = np.random.default_rng(23)
    refs, positions = [], []
    for k in range(24):
        c = int(rng.integers(0, len(starts) - 1))
        W = int(rng.integers(600, 3000))
        p = int(rng.integers(starts[c], max(starts[c] + 1, starts[c + 1] - 1000 - W) + 1))
        refs.append(orc.window(z["binref"], z["starts"], p, W + 1)[:W])
        positions.append(p)
    queries = [_with_bursts(rng, synth.mutate(rng, np.frombuffer(r.replace(b"x", b"A"), dtype=np.uint8), 0.08).tobytes()) for r in refs]
    tiles = [synth.Tile(r, q, *synth.corridor_anchors(len(q), len(r)), tag="win%d" % k) for k, (r, q) in enumerate(zip(refs, queries))]
    reads, segs = embed_queries(rng, queries, [int(x) for x in rng.integers(0, 2, size=len(refs))])
    want = _plain(plain.submit(tiles))
    assert len(want[4]) >= 10
    gp, ga = Genome(plain, z["binref"], int(z["nibbles"]), z["starts"]), Genome(al, z["binref"], int(z["nibbles"]), z["starts"])
    try:
        _same_as_plain(want, _with_results(al.submit(tiles)))
        _same_as_plain(_plain(gp.submit(tiles, positions)), _with_results(ga.submit(tiles, positions)))
        _same_as_plain(want, _with_results(al.submit_segments(tiles, reads, segs)))
        _same_as_plain(want, _with_results(al.submit_segments(tiles, reads, segs, genome=ga, ref_positions=positions)))
    finally:
        gp.free()
        ga.free()


def test_align_batch_runs_the_same_stages(handles):
    """the synchronous form on a flagged handle: the finder runs inside it and its results stay a plain handle's"""
    tiles = cases.stretch_tiles(6, seed=12)
    arr, keep = handles["regions"]._pack(tiles)
    from ngmlr_amd import capi
    lib = handles["regions"].lib
    res = (capi.CvxResult * len(tiles))()
    ops = np.zeros(1 << 20, dtype=np.uint32)
    used = C.c_uint64()
    assert lib.cvx_align_batch(handles["regions"].h, len(tiles), arr, res, ops.ctypes.data, len(ops), C.byref(used)) == 0
    res2 = (capi.CvxResult * len(tiles))()
    ops2 = np.zeros(1 << 20, dtype=np.uint32)
    used2 = C.c_uint64()
    arr2, keep2 = handles["plain"]._pack(tiles)
    assert lib.cvx_align_batch(handles["plain"].h, len(tiles), arr2, res2, ops2.ctypes.data, len(ops2), C.byref(used2)) == 0
    assert bytes(res) == bytes(res2) and used.value == used2.value > 0 and np.array_equal(ops, ops2)


def test_a_smaller_job_in_the_slot_of_a_larger_one(handles):
    tiles = family_tiles()
    big = _with_results(handles["regions"].submit(tiles))      # released: its slot, offsets and arena go back to the handle's pool
    small = tiles[7:19]
    want = _plain(handles["plain"].submit(small), small)
    got = _with_results(handles["regions"].submit(small))
    _same_as_plain(want, got)
    assert 0 < got[5]["total"] < big[5]["total"]
