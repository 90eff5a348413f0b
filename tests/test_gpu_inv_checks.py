"""GPU (-m gpu): the inversion checks of low-identity regions scored on the device (inv_checks_kernel) -- the stand-alone form
(cvx_inv_checks) record for record against cvx_inv_checks_host on the engineered families of tests/inv_check_cases.py and on the
calls recorded from the unmodified reference, and the job form (CVX_CREATE_INV_CHECKS, cvx_job_checks) on windows and segments:
results, ops, regions and end states a CVX_CREATE_NM_REGIONS handle's byte for byte, the checks cvx_inv_checks_host's over the
job's own regions and results; the rewrite over a grown arena, jobs without a genome or a region, a reused slot, the twin and
job-text combinations, the flags."""
import ctypes as C

import numpy as np
import pytest

from tests import inv_check_cases as cases
from tests import nm_region_cases as region_cases

pytestmark = pytest.mark.gpu


def burst_tile(rng, length=3000, period=110, run=24, tag="bursts"):
    """(tests/test_gpu_job_regions.py's) A read without indels whose every `period`-th base starts `run` substituted bases: one
    region per period, 26 in 3 000 bases."""
    from ngmlr_amd import synth
    ref = synth.random_ref(rng, length)
    qry = ref.copy()
    for a in range(60, length - 60 - run, period):
        qry[a:a + run] = synth._ACGT[(synth._CODE[qry[a:a + run]].astype(np.int64) + 1) % 4]
    off, ln = synth.corridor_anchors(len(qry), length, mult=2, scatter_left=20.0, scatter_right=20.0)
    return synth.Tile(ref=ref.tobytes(), qry=qry.tobytes(), row_offset=off, row_length=ln, tag=tag)


def invalid_tiles(n=4):
    from ngmlr_amd import synth
    return [synth.Tile(b"A" * (200 + 37 * i), b"C" * (150 + 41 * i), *synth.corridor_anchors(150 + 41 * i, 200 + 37 * i), tag="invalid%d" % i)
            for i in range(n)]


def job_tiles():
    """stretch tiles, the burst tile and a tile with a planted 200-base inverted stretch (the last one)"""
    rng = np.random.default_rng(55)
    return region_cases.stretch_tiles(14) + [burst_tile(rng)] + [region_cases.stretch_tile(rng, 3000, 200, "inv", 0.05, tag="planted")]


def genome_of(lib, tiles):
    """one contig that holds every tile's reference window back to back between 1 500 random bases -> (encoded genome, ref_position per tile)"""
    from ngmlr_amd import aligner, synth
    rng = np.random.default_rng(56)
    parts, at, where = [synth.random_ref(rng, 1500).tobytes()], 1500, []
    for t in tiles:
        where.append(at)
        parts.append(t.ref)
        at += len(t.ref)
    parts.append(synth.random_ref(rng, 1500).tobytes())
    genome = aligner.encode_genome(lib, [b"".join(parts)])
    return genome, [int(genome[2][0]) + w for w in where]


@pytest.fixture(scope="module")
def handles(built):
    from ngmlr_amd.aligner import ConvexAlignHip
    hs = {"plain": ConvexAlignHip(device=0), "regions": ConvexAlignHip(device=0, nm_regions=True),
          "checks": ConvexAlignHip(device=0, nm_regions=True, inv_checks=True)}
    yield hs
    for al in hs.values():
        al.close()


@pytest.fixture(scope="module")
def lib(handles):
    return handles["plain"].lib


def _finish(job, want_checks=True):
    """wait -> (results, results bytes, ops bytes, off, reg, open, info, checks)"""
    res, ops = job.wait()
    out = (res.copy(), res.tobytes(), ops.tobytes()) + job.regions() + (job.regions_info(), job.checks() if want_checks else None)
    job.release()
    return out


def _host_checks(lib, genome, tiles, positions, run):
    from ngmlr_amd import aligner
    res, off, reg = run[0], run[3], run[4]
    return aligner.inv_checks_host(genome[0], genome[1], genome[2], [t.qry for t in tiles], positions, res["ref_position"], off, reg, lib=lib)


def _same_job(want, got):
    assert got[1] == want[1] and got[2] == want[2], "results / ops"
    assert np.array_equal(got[3], want[3]) and np.array_equal(got[4], want[4]) and got[5].tobytes() == want[5].tobytes(), "regions / end states"


def _records(a):
    return [tuple(x) for x in a.tolist()]


# --------------------------------------------------------------------------- the stand-alone form

@pytest.fixture(scope="module")
def small(handles, lib):
    from ngmlr_amd.aligner import Genome
    genome, calls = cases.engineered(lib)
    g = Genome(handles["plain"], *genome)
    yield genome, calls, g
    g.free()


def test_engineered_calls_equal_the_host_rule(handles, lib, small):
    from ngmlr_amd import aligner
    genome, calls, g = small
    args = cases.as_tiles(calls)
    want = aligner.inv_checks_host(*genome, *args, lib=lib)
    got, ms = handles["plain"].inv_checks(g, *args)
    assert _records(got) == _records(want) and got.tobytes() == want.tobytes()
    assert ms > 0
    assert {511, 2047, 2048, 2049, 6000} <= set(int(x) for x in got["window_chars"])
    assert set(int(x) for x in got["status"]) == {0, 1, 2, 3}
    # tiles without regions between the others: the kernel finds a region's tile by its offset
    got2, _ = handles["plain"].inv_checks(g, *cases.with_empty_tiles(args))
    assert got2.tobytes() == want.tobytes()


@pytest.mark.parametrize("n", [1, 3, 4, 5])
def test_regions_that_fill_and_do_not_fill_a_workgroup(handles, lib, small, n):
    from ngmlr_amd import aligner
    genome, calls, g = small
    scored = [c for c in calls if c.plan()[0] is None]
    for first in (0, 9, 20):
        args = cases.as_tiles(scored[first:first + n])
        got, _ = handles["plain"].inv_checks(g, *args)
        assert len(got) == n and got.tobytes() == aligner.inv_checks_host(*genome, *args, lib=lib).tobytes()


def test_windows_at_the_scorers_length_limit(handles, lib):
    from ngmlr_amd import aligner
    genome, calls = cases.long_genome(lib)
    g = aligner.Genome(handles["plain"], *genome)
    try:
        args = cases.as_tiles(calls)
        want = aligner.inv_checks_host(*genome, *args, lib=lib)
        got, _ = handles["plain"].inv_checks(g, *args)
    finally:
        g.free()
    assert _records(got) == _records(want)
    assert [int(x) for x in got["window_chars"]] == [99998, 99999, 99996] and got["score_fwd"][1] == -1.0 and got["score_fwd"][0] >= 60


@pytest.mark.parametrize("name", cases.RECORDED)
def test_recorded_reference_calls(handles, lib, name):
    from ngmlr_amd import aligner
    genome, calls, z = cases.recorded(lib, name)
    want = cases.recorded_records(z)
    g = aligner.Genome(handles["plain"], *genome)
    try:
        got, _ = handles["plain"].inv_checks(g, *cases.as_tiles(calls))
    finally:
        g.free()
    for f in ("status", "score_fwd", "score_rev"):
        assert got[f].tobytes() == want[f].tobytes(), f
    ran = z["outcome"] == 0
    assert np.array_equal(got["window_chars"][ran], z["ref_chars"][ran])


def test_stand_alone_arguments(handles, small):
    from ngmlr_amd import capi
    genome, calls, g = small
    lib = handles["plain"].lib
    assert lib.cvx_inv_checks(handles["plain"].h, None, 0, None, None, None, None, None, None, None, None) == -3
    assert lib.cvx_inv_checks(handles["plain"].h, g.g, 0, None, None, None, None, None, None, None, None) == 0
    off = np.array([1, 2], dtype=np.uint64)
    q = (C.c_char_p * 1)(b"ACGT")
    ql, pos, po = np.array([4], dtype=np.int32), np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.int32)
    assert lib.cvx_inv_checks(handles["plain"].h, g.g, 1, q, ql.ctypes.data, pos.ctypes.data, po.ctypes.data, off.ctypes.data, None, None, None) == -3
    assert capi.CHECK_NO_WINDOW == 3


# --------------------------------------------------------------------------- the job form

@pytest.fixture(scope="module")
def job_run(handles, lib):
    from ngmlr_amd.aligner import Genome
    tiles = job_tiles()
    genome, positions = genome_of(lib, tiles)
    gr, gc = Genome(handles["regions"], *genome), Genome(handles["checks"], *genome)
    want = _finish(gr.submit(tiles, positions), want_checks=False)
    got = _finish(gc.submit(tiles, positions))
    yield tiles, genome, positions, gr, gc, want, got
    gr.free()
    gc.free()


def test_job_on_windows(lib, job_run):
    tiles, genome, positions, _gr, _gc, want, got = job_run
    _same_job(want, got)
    off, chk = got[3], got[7]
    assert chk is not None and len(chk) == int(off[-1]) == got[6]["total"] >= 40
    assert _records(chk) == _records(_host_checks(lib, genome, tiles, positions, got))
    planted = chk[int(off[len(tiles) - 1]):int(off[len(tiles)])]
    assert len(planted) >= 1 and (planted["score_rev"] > planted["score_fwd"]).any()
    assert (chk["status"] == 0).sum() >= 20


@pytest.mark.parametrize("with_genome", [True, False])
def test_job_on_segments(handles, lib, job_run, with_genome):
    from tests.segment_cases import embed_queries
    tiles, genome, positions, _gr, gc, want, _got = job_run
    rng = np.random.default_rng(57)
    reads, segs = embed_queries(rng, [t.qry for t in tiles], [i % 2 for i in range(len(tiles))])      # both strands
    if with_genome:
        got = _finish(handles["checks"].submit_segments(tiles, reads, segs, genome=gc, ref_positions=positions))
        _same_job(want, got)
        assert _records(got[7]) == _records(_host_checks(lib, genome, tiles, positions, got))
    else:
        got = _finish(handles["checks"].submit_segments(tiles, reads, segs))      # no genome, no checks
        _same_job(want, got)
        assert got[6]["total"] > 0 and got[7] is None


def test_more_regions_than_the_arena_was_sized_for(built, lib):
    """20 burst tiles of 26 regions against an arena sized for eight per tile: the regions are written again over a larger arena,
    and the checks run again with them; the same job again in the slot (the arena is large now) gives the same records"""
    from ngmlr_amd.aligner import ConvexAlignHip, Genome
    rng = np.random.default_rng(58)
    tiles = [burst_tile(rng, length=int(rng.integers(2400, 3001)), tag="bursts%d" % i) for i in range(20)]
    genome, positions = genome_of(lib, tiles)
    al = ConvexAlignHip(device=0, nm_regions=True, inv_checks=True)
    g = Genome(al, *genome)
    try:
        got = _finish(g.submit(tiles, positions))
        assert got[6]["rewrites"] >= 1 and got[6]["total"] > got[6]["first_capacity"], got[6]
        want = _host_checks(lib, genome, tiles, positions, got)
        assert len(got[7]) == got[6]["total"] and _records(got[7]) == _records(want)
        again = _finish(g.submit(tiles, positions))
        assert again[6]["rewrites"] == 0 and again[7].tobytes() == got[7].tobytes() and again[1] == got[1]
    finally:
        g.free()
        al.close()


def test_jobs_without_a_genome_or_a_region(handles, lib, job_run):
    tiles, genome, positions, _gr, gc, want, _got = job_run
    al = handles["checks"]
    got = _finish(al.submit(tiles))                       # cvx_submit: no genome
    _same_job(want, got)
    assert got[6]["total"] > 0 and got[7] is None
    assert _finish(al.submit([]))[7] is None
    # tiles without a valid alignment, and clean tiles: no region
    for quiet in (invalid_tiles(), region_cases.clean_tiles(3)):
        from ngmlr_amd.aligner import Genome
        gq, pq = genome_of(lib, quiet)
        g = Genome(al, *gq)
        try:
            run = _finish(g.submit(quiet, pq))
        finally:
            g.free()
        assert run[6]["total"] == 0 and run[7] is None


def test_a_smaller_job_in_the_slot_of_a_larger_one(handles, lib, job_run):
    tiles, genome, positions, _gr, gc, _want, big = job_run
    small_tiles, small_pos = tiles[3:8], positions[3:8]
    got = _finish(gc.submit(small_tiles, small_pos))
    assert 0 < got[6]["total"] < big[6]["total"]
    assert _records(got[7]) == _records(_host_checks(lib, genome, small_tiles, small_pos, got))


@pytest.mark.parametrize("combo", [dict(scalar_twin=True), dict(job_text=True), dict(scalar_twin=True, job_text=True)],
                         ids=["twin", "job_text", "twin+job_text"])
def test_twin_and_job_text_combinations(lib, job_run, combo):
    from ngmlr_amd.aligner import ConvexAlignHip, Genome
    tiles, genome, positions = job_run[0][-6:], job_run[1], job_run[2][-6:]
    base, al = ConvexAlignHip(device=0, nm_regions=True, **combo), ConvexAlignHip(device=0, nm_regions=True, inv_checks=True, **combo)
    gb, ga = Genome(base, *genome), Genome(al, *genome)
    try:
        jb, ja = gb.submit(tiles, positions), ga.submit(tiles, positions)
        jb.wait()
        ja.wait()
        if combo.get("job_text"):
            tb, ta = jb.texts_raw(), ja.texts_raw()
            assert [bytes(x) for x in tb[0]] == [bytes(x) for x in ta[0]] and np.array_equal(tb[1], ta[1]) and tb[2] == ta[2]
        want, got = _finish(jb, want_checks=False), _finish(ja)
        _same_job(want, got)
        assert got[6]["total"] > 0 and _records(got[7]) == _records(_host_checks(lib, genome, tiles, positions, got))
    finally:
        gb.free()
        ga.free()
        base.close()
        al.close()


def test_flags(handles):
    from ngmlr_amd import capi
    lib, p = handles["plain"].lib, handles["plain"].params
    assert capi.CREATE_INV_CHECKS == 32
    for extra in (0, 2, 16, 2 | 16):
        h = C.c_void_p()
        assert lib.cvx_create_ex(0, C.byref(p), 0, 32 | 4 | extra, C.byref(h)) == 0, extra
        lib.cvx_destroy(h)
    h = C.c_void_p()
    assert lib.cvx_create_ex(0, C.byref(p), 0, 32, C.byref(h)) == -3 and b"CVX_CREATE_NM_REGIONS" in lib.cvx_last_error() and not h.value
    assert lib.cvx_create_ex(0, C.byref(p), 0, 32 | 4 | 1, C.byref(h)) == -3 and b"SERVICE" in lib.cvx_last_error() and not h.value
    assert lib.cvx_create_ex(0, C.byref(p), 0, 8, C.byref(h)) == -3
    assert lib.cvx_create_ex(0, C.byref(p), 0, 64, C.byref(h)) == -3
    assert lib.cvx_abi_version() == 9
    # a handle without the flag; a job nobody has waited for
    tiles = region_cases.stretch_tiles(3, seed=4)
    pc = C.c_void_p(1)
    job = handles["regions"].submit(tiles)
    job.wait()
    assert lib.cvx_job_checks(handles["regions"].h, job.j, C.byref(pc)) == -3
    assert b"CVX_CREATE_INV_CHECKS" in lib.cvx_last_error() and not pc.value
    job.release()
    job = handles["checks"].submit(tiles)
    assert lib.cvx_job_checks(handles["checks"].h, job.j, C.byref(pc)) == -3 and b"cvx_wait" in lib.cvx_last_error()
    job.wait()
    assert lib.cvx_job_checks(handles["checks"].h, job.j, C.byref(pc)) == 0 and not pc.value      # (cvx_submit: no genome)
    assert lib.cvx_job_checks(handles["checks"].h, job.j, None) == -3
    job.release()
