"""GPU (-m gpu): everything a handle owns is created, used and given back, three times over, and every round computes what the
first did and what the CPU oracles say.  A round walks every place where the runtime's buffers and events die: the pool (a job
waited for and released), the live list (jobs left to cvx_destroy), a failed job's batch, a ladder job's later rungs (released, and
left to cvx_destroy), the resident genome, the search and the scoring state of a handle, and the scope of each stand-alone entry.

cvx_submit_ladder refuses a handle with CVX_CREATE_NM_REGIONS, _INV_CHECKS or _JOB_TEXT (tests/test_gpu_ladder.py), so a round
has two handles: one with those three flags for the jobs with regions, checks and text, a plain one for the ladder jobs."""
import os

import numpy as np
import pytest

from tests import ladder_cases as lc
from tests import nm_region_cases as region_cases
from tests import util

pytestmark = pytest.mark.gpu

ROUNDS = 3
LADDER_TAGS = ("ep256-d0", "ep256-d60", "anchors-d20", "realign-d40")      # rungs 1, 2, 1, 1


def _flag_tiles():
    """four tiles of 500 to 700 bases: an inverted and an unrelated stretch, substitution bursts, a clean read -- 1, 1, 5 and 0 regions"""
    from tests.test_gpu_inv_checks import burst_tile
    rng = np.random.default_rng(71)
    return [region_cases.stretch_tile(rng, 700, 120, "inv", 0.05, tag="inv"), region_cases.stretch_tile(rng, 600, 90, "random", 0.1, tag="random"),
            burst_tile(rng, length=640), region_cases.clean_tiles(1, length=500)[0]]


@pytest.fixture(scope="module")
def fixture(built, port_oracle):
    """the tiles, their genomes and what the CPU oracles say, computed once and left alone"""
    from types import SimpleNamespace
    from ngmlr_amd import capi
    from oracle.pyoracle import SearchFixture
    from tests.test_gpu_inv_checks import genome_of
    lib = capi.load()
    tiles = _flag_tiles()
    genome, positions = genome_of(lib, tiles)
    want = [port_oracle.align(t) for t in tiles]
    scans = [region_cases.literal_scan(region_cases.padded(w["nm_per_position"], w["alignment_length"]), w["alignment_length"]) for w in want]
    assert all(w["ret"] >= 0 for w in want) and sum(len(s[0]) for s in scans) >= 3
    by_tag = {tag: (ref, qry, ladder) for tag, ref, qry, ladder in lc.engineered()}
    ladders = []
    for tag in LADDER_TAGS:
        ref, qry, ladder = by_tag[tag]
        rung, rungs = lc.climb(ref, qry, ladder, lambda t: port_oracle.align(t, want_nm=False)["ret"] >= 0)
        ladders.append(dict(tag=tag, ref=ref, qry=qry, ladder=ladder, rung=rung, tiles=rungs, live=True, port=port_oracle.align(rungs[-1])))
    assert sorted(e["rung"] for e in ladders) == [1, 1, 1, 2]
    from ngmlr_amd import synth
    lad_tiles = [synth.Tile(e["ref"], e["qry"], np.zeros(0, np.int32), np.zeros(0, np.int32), tag=e["tag"], desc=(2, 0.0, 0.0, 0.0, 0, 0)) for e in ladders]
    lad_genome, lad_positions = genome_of(lib, lad_tiles)
    search = SearchFixture(os.path.join(util.GOLDEN, "cs_test_3.npz"))
    return SimpleNamespace(lib=lib, tiles=tiles, genome=genome, positions=positions, want=want, scans=scans,
                           ladders=ladders, lad_tiles=lad_tiles, lad_genome=lad_genome, lad_positions=lad_positions, search=search)


@pytest.fixture(scope="module")
def kmer_table(fixture):
    """the k-mer table of the search fixture, uploaded once: a table belongs to no handle, the search state it is searched with does"""
    from ngmlr_amd.aligner import ConvexAlignHip, KmerIndex
    al = ConvexAlignHip(device=0)
    idx, locs = fixture.search.index_arrays()
    ix = KmerIndex(al, fixture.search.k, idx, locs, fixture.search.unit_offset)
    yield ix
    ix.free()
    al.close()


def _job_answer(job):
    """everything a finished job of the flag handle hands out, copied"""
    res, ops = job.wait()
    off, reg, opn = job.regions()
    recs, toff, raw = job.texts_raw()
    return dict(res=res.copy(), ops=ops.copy(), off=off, reg=reg, open=opn, checks=job.checks(), texts=job.texts(), text_off=toff, text_raw=raw)


def _flag_round(fx):
    """create, three jobs with a genome (released, left alone, failed), the six stand-alone entries at the jobs' size, destroy"""
    from ngmlr_amd import aligner, capi
    from ngmlr_amd.aligner import ConvexAlignHip, Genome
    import ctypes as C
    os.environ["CVX_TUNE_FAIL_COMPUTE"] = "3"
    try:
        al = ConvexAlignHip(device=0, nm_regions=True, inv_checks=True, job_text=True)
    finally:
        del os.environ["CVX_TUNE_FAIL_COMPUTE"]
    out = {}
    try:
        g = Genome(al, *fx.genome)
        jobs = [g.submit(fx.tiles, fx.positions) for _ in range(3)]
        out["released"] = _job_answer(jobs[0])
        jobs[0].release()
        out["kept"] = _job_answer(jobs[1])               # never released: cvx_destroy finds it on the handle's live list
        errors = []
        for _ in range(2):                               # the failed job answers with its own error, every time
            with pytest.raises(capi.CvxError) as e:
                jobs[2].wait()
            errors.append((e.value.code, "CVX_TUNE_FAIL_COMPUTE" in str(e.value)))
        out["errors"] = errors
        jobs[2].release()
        # the stand-alone entries, each once, over the same four tiles
        n = len(fx.tiles)
        out["decode"] = g.decode(fx.positions, [len(t.ref) + 1 for t in fx.tiles])
        reads = [t.qry for t in fx.tiles]
        segs = [(i, 3 * i, i % 2) for i in range(n)]     # both strands, a few bases into the read
        lens = [len(t.qry) - 3 * i - 7 for i, t in enumerate(fx.tiles)]
        out["segments"] = (al.stage_segments(reads, segs, lens), aligner.stage_segments_host(fx.lib, reads, segs, lens))
        out["rows"] = [tuple(a.copy() for a in al.corridor_rows(e["tiles"][0])) for e in fx.ladders]
        a = out["kept"]
        out["inv_checks"] = al.inv_checks(g, reads, fx.positions, a["res"]["ref_position"], a["off"], a["reg"])[0]
        res = (capi.CvxResult * n).from_buffer_copy(a["res"].tobytes())
        out["regions_ops"] = al.nm_regions_ops(res, a["ops"])
        arena = np.ascontiguousarray(a["ops"], dtype=np.uint32)
        eoff = np.zeros(n + 1, dtype=np.uint64)
        capi.check(fx.lib.cvx_nm_profile_ops(al.h, n, res, arena.ctypes.data, len(arena), eoff.ctypes.data, None, 0))
        tri = np.zeros((int(eoff[n]), 3), dtype=np.int32)
        capi.check(fx.lib.cvx_nm_profile_ops(al.h, n, res, arena.ctypes.data, len(arena), eoff.ctypes.data, tri.ctypes.data, len(tri)))
        out["profile_ops"] = (eoff, tri)
        g.free()
    finally:
        al.close()
    return out


def _ladder_round(fx, ix):
    """create, two ladder jobs with a genome (one released, one left to cvx_destroy), a search and a scoring call, destroy"""
    from ngmlr_amd.aligner import ConvexAlignHip, Genome, StrippedSWHip
    al = ConvexAlignHip(device=0)
    out = {}
    try:
        g = Genome(al, *fx.lad_genome)
        jobs = [al.submit_ladder(fx.lad_tiles, [e["ladder"] for e in fx.ladders], genome=g, ref_positions=fx.lad_positions) for _ in range(2)]
        for name, job in zip(("released", "kept"), jobs):
            res, ops = job.wait()
            out[name] = dict(res=res.copy(), ops=ops.copy(), lad=job.ladder(), info=job.ladder_info())
        jobs[0].release()
        # the handle's search state, over a table that outlives it
        owner, ix.al = ix.al, al
        try:
            out["search"] = ix.search(fx.search.seqs[:8])
        finally:
            ix.al = owner
        g.free()
    finally:
        al.close()
    sw = StrippedSWHip(device=0)
    try:
        out["scores"] = sw.batch_score([t.ref for t in fx.tiles], [t.qry for t in fx.tiles])
    finally:
        sw.close()
    return out


def _flat(x):
    """an answer as bytes and plain values, for comparing two rounds"""
    if isinstance(x, dict):
        return {k: _flat(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_flat(v) for v in x]
    if isinstance(x, np.ndarray):
        return (str(x.dtype), x.shape, x.tobytes())
    return x


@pytest.fixture(scope="module")
def rounds(fixture, kmer_table):
    return [(_flag_round(fixture), _ladder_round(fixture, kmer_table)) for _ in range(ROUNDS)]


def test_every_round_equals_the_first(rounds):
    first = _flat(rounds[0])
    for k in range(1, ROUNDS):
        got = _flat(rounds[k])
        for part in (0, 1):
            for name in first[part]:
                assert got[part][name] == first[part][name], (k, part, name)


def test_the_jobs_equal_the_oracles(fixture, rounds):
    from ngmlr_amd import aligner, capi
    from ngmlr_amd.aligner import format_alignment
    from oracle.pyoracle import same_alignment
    fx, (flag, _lad) = fixture, rounds[0]
    assert _flat(flag["released"]) == _flat(flag["kept"])
    a = flag["kept"]
    for i, t in enumerate(fx.tiles):
        got = format_alignment(fx.lib, capi.CvxResult.from_buffer_copy(a["res"][i].tobytes()), a["ops"], t)
        assert same_alignment(fx.want[i], got) is None, (t.tag, same_alignment(fx.want[i], got))
        mine = a["reg"][int(a["off"][i]):int(a["off"][i + 1])]
        assert region_cases.same(fx.scans[i], mine, a["open"][i]) is None, t.tag
        assert (a["texts"][i]["cigar"], a["texts"][i]["md"]) == (fx.want[i]["cigar"], fx.want[i]["md"]), t.tag
    assert a["checks"] is not None and len(a["checks"]) == int(a["off"][-1]) >= 3
    host = aligner.inv_checks_host(fx.genome[0], fx.genome[1], fx.genome[2], [t.qry for t in fx.tiles], fx.positions, a["res"]["ref_position"], a["off"], a["reg"], lib=fx.lib)
    assert a["checks"].tobytes() == host.tobytes()
    # the failed job returned its own error, twice (tests/test_gpu_abi.py: test_a_failed_job_keeps_its_own_error)
    assert flag["errors"] == [(-4, True), (-4, True)]


def test_the_ladder_jobs_equal_the_oracles(fixture, rounds, hip_aligner):
    from tests.test_gpu_ladder import _check_against_expectation
    lad = rounds[0][1]
    assert _flat(lad["released"]) == _flat(lad["kept"])
    a = lad["kept"]
    _check_against_expectation(hip_aligner, fixture.ladders, a["res"], a["ops"], a["lad"], a["info"], against=("port",))
    assert a["info"]["rungs_run"] == 2 and a["info"]["tiles"][:2] == [4, 1]


def test_the_stand_alone_entries_equal_the_oracles(fixture, rounds):
    from tests.test_gpu_search import _same
    fx, (flag, lad) = fixture, rounds[0]
    a = flag["kept"]
    assert flag["decode"] == [t.ref + b"\0" for t in fx.tiles]
    assert flag["segments"][0] == flag["segments"][1] and all(len(s) > 400 for s in flag["segments"][0])
    for e, (off, ln) in zip(fx.ladders, flag["rows"]):
        assert np.array_equal(off, e["tiles"][0].row_offset) and np.array_equal(ln, e["tiles"][0].row_length), e["tag"]
    assert flag["inv_checks"].tobytes() == a["checks"].tobytes()
    off, reg, opn = flag["regions_ops"]
    assert np.array_equal(off, a["off"]) and np.array_equal(reg, a["reg"]) and opn.tobytes() == a["open"].tobytes()
    eoff, tri = flag["profile_ops"]
    for i, w in enumerate(fx.want):
        mine = tri[int(eoff[i]):int(eoff[i + 1])]
        rows = np.asarray(w["nm_per_position"], dtype=np.int32).reshape(-1, 3)      # the entries, then zeros up to alignment_length
        assert len(mine) > 400 and np.array_equal(mine, rows[:len(mine)]) and not rows[len(mine):].any(), fx.tiles[i].tag
    assert all(_same(lad["search"][i], *fx.search.want[i]) for i in range(8))
    assert len(lad["scores"]) == len(fx.tiles) and (lad["scores"] > 0).all()
