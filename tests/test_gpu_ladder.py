"""GPU: cvx_submit_ladder -- the corridor retry ladder of computeAlignment climbed inside one device job -- against the Python
rule over the CPU oracles rung by rung (tests/ladder_cases.py), against the device's own sequential path (batch_align of the
reported rung's row-array tile), with other jobs in flight, with a resident genome, on a scalar-twin handle, and the refusals."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import ladder_cases as lc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _valid(oracle):
    return lambda t: oracle.align(t, want_nm=False)["ret"] >= 0


@pytest.fixture(scope="module")
def expectation(port_oracle, ref_oracle):
    """per engineered tile: the rung both oracles report, the rungs' row-array tiles, both oracles' alignment of the reported one"""
    out = []
    for tag, ref, qry, ladder in lc.engineered():
        n, tiles = lc.climb(ref, qry, ladder, _valid(port_oracle))
        n_ref, _ = lc.climb(ref, qry, ladder, _valid(ref_oracle))
        assert n == n_ref, (tag, n, n_ref)
        last = tiles[-1]
        live = lc.has_cells(last)
        out.append(dict(tag=tag, ref=ref, qry=qry, ladder=ladder, rung=n, tiles=tiles, live=live,
                        port=port_oracle.align(last) if live else None, reference=ref_oracle.align(last) if live else None))
    return out


def test_the_set_holds_every_ladder_the_issue_names(expectation):
    """from the CPU oracles alone: every ladder length 1 ... 5 among the resolved tiles, a tile no rung resolves, the switch from
    the anchors form to the endpoints form, a ladder the cap ends, REALIGN, FULL, SHORT, a 1-row tile and empty tiles"""
    resolved = {e["rung"] for e in expectation if e["live"] and e["port"]["ret"] >= 0}
    assert resolved == {1, 2, 3, 4, 5}
    assert any(e["rung"] == 5 and e["live"] and e["port"]["ret"] < 0 for e in expectation)
    assert any(e["ladder"][3] == lc.ANCHORS and e["rung"] >= 3 and e["port"]["ret"] >= 0 and e["tiles"][1].desc[3] != 0.0 and e["tiles"][2].desc[3] == 0.0 for e in expectation)
    assert any(e["rung"] == 1 and lc.ladder_length(len(e["ref"]), e["ladder"]) == 1 and not e["ladder"][3] & lc.FULL for e in expectation)
    assert any(e["ladder"][3] & lc.REALIGN and e["rung"] == 2 for e in expectation)
    assert any(e["ladder"][3] & lc.FULL for e in expectation) and any(e["ladder"][3] & lc.SHORT and e["rung"] == 2 for e in expectation)
    assert any(len(e["qry"]) == 1 and e["live"] and e["rung"] > 1 for e in expectation)      # (a 1-row tile is never valid: its best cell lies in read row 0)
    assert any(len(e["qry"]) == 0 for e in expectation) and any(len(e["ref"]) == 0 for e in expectation)


def _as_result(rec):
    from ngmlr_amd import capi
    return capi.CvxResult.from_buffer_copy(rec.tobytes())


def _run_ladder(al, cases, genome=None, positions=None):
    """-> (records copy, ops copy, ladder records, info, timing, launches) of one ladder job"""
    from ngmlr_amd import synth
    tiles = [synth.Tile(e["ref"], e["qry"], np.zeros(0, np.int32), np.zeros(0, np.int32), tag=e["tag"], desc=(2, 0.0, 0.0, 0.0, 0, 0)) for e in cases]
    job = al.submit_ladder(tiles, [e["ladder"] for e in cases], genome=genome, ref_positions=positions)
    res, ops = job.wait()
    out = (res.copy(), ops.copy(), job.ladder(), job.ladder_info(), job.timing(), job.launches())
    job.release()
    return out


def _check_against_expectation(al, cases, res, ops, lad, info, against=("port", "reference")):
    from ngmlr_amd.aligner import format_alignment
    from oracle.pyoracle import same_alignment
    used = 0
    for i, e in enumerate(cases):
        last = e["tiles"][-1]
        assert (int(lad[i]["rung"]), int(lad[i]["attempts"]), int(lad[i]["width"])) == (e["rung"], e["rung"], last.desc[5]), (e["tag"], lad[i], e["rung"], last.desc)
        assert int(res[i]["ops_begin"]) == used, e["tag"]      # the dense arena holds the ops of exactly the reported records, in tile order
        used += int(res[i]["n_ops"])
        if not e["live"]:
            assert int(res[i]["status"]) == 5 and int(res[i]["n_ops"]) == 0, (e["tag"], res[i])
            continue
        got = format_alignment(al.lib, _as_result(res[i]), ops, last)
        for name in against:
            assert same_alignment(e[name], got) is None, (e["tag"], name, same_alignment(e[name], got))
        assert (got["status"] == 0) == (e["port"]["ret"] >= 0) and got["status"] != -1, (e["tag"], got["status"])
    assert used == len(ops)
    want_tiles = [sum(1 for e in cases if e["rung"] >= r + 1) for r in range(5)]
    assert info["tiles"] == want_tiles and info["rungs_run"] == max([e["rung"] for e in cases] + [1]), (info, want_tiles)
    assert info["seq_bytes_after_submit"] == 0


def test_every_engineered_ladder_equals_the_rule_over_the_oracles(hip_aligner, expectation):
    res, ops, lad, info, timing, launches = _run_ladder(hip_aligner, expectation)
    _check_against_expectation(hip_aligner, expectation, res, ops, lad, info)
    # timing sums over the rungs, the launch list strings the rungs' launches together
    assert timing.n_fill_launches == len(launches) >= info["rungs_run"]
    assert sum(l["n_tiles"] for l in launches) <= sum(info["tiles"]) and timing.total_ms > 0.0


def test_the_reported_rung_equals_the_sequential_device_path(hip_aligner, expectation):
    """the same records against hip_aligner.batch_align of the reported rung's row-array tile"""
    from ngmlr_amd.aligner import format_alignment
    from oracle.pyoracle import same_alignment
    res, ops, lad, _, _, _ = _run_ladder(hip_aligner, expectation)
    want = hip_aligner.batch_align([e["tiles"][-1] for e in expectation])
    for i, e in enumerate(expectation):
        got = format_alignment(hip_aligner.lib, _as_result(res[i]), ops, e["tiles"][-1])
        assert same_alignment(want[i], got) is None, (e["tag"], same_alignment(want[i], got))
        assert all(want[i][k] == got[k] for k in ("status", "ret", "fwd_score_bits", "best_x", "best_y") if want[i]["status"] == 0), (e["tag"], want[i]["status"], got["status"])
        assert want[i]["status"] == got["status"], (e["tag"], want[i]["status"], got["status"])


def test_an_empty_ladder_job(hip_aligner):
    res, ops, lad, info, _, launches = _run_ladder(hip_aligner, [])
    assert len(res) == 0 and len(ops) == 0 and len(lad) == 0 and info["rungs_run"] == 1 and info["tiles"] == [0] * 5 and launches == []


def test_a_too_large_rung_climbs_like_any_invalid_one(built, port_oracle):
    """max_matrix_mb = 1: a rung of 1 000 000 cells or more is CVX_TILE_TOO_LARGE, the reference's -1"""
    from ngmlr_amd import synth
    from ngmlr_amd.aligner import ConvexAlignHip
    rng = np.random.default_rng(5)
    g = synth.random_ref(rng, 3000)
    cases = []
    # 2 400 rows: rung 1 (width 400, 960 000 cells) fits and fails on the 600-base deletion; every later rung is too large
    cases.append(("too-large-later", g.tobytes(), np.concatenate([g[:1200], g[1800:]]).tobytes(), (1600, 0.0, 0.0, 0)))
    ref = g[:2700]
    # rungs 1 and 2 too large at once (REALIGN keeps the whole corridor), and a plain tile beside them
    cases.append(("too-large-first", ref.tobytes(), np.concatenate([ref[:1200], ref[1500:]]).tobytes(), (2700, 0.0, 0.0, lc.REALIGN)))
    cases.append(("fits", g[:640].tobytes(), np.concatenate([g[:300], g[340:640]]).tobytes(), (256, 0.0, 0.0, 0)))
    exp = []
    for tag, r, q, ladder in cases:
        n, tiles = lc.climb(r, q, ladder, _valid(port_oracle), max_matrix_mb=1)
        exp.append(dict(tag=tag, ref=r, qry=q, ladder=ladder, rung=n, tiles=tiles))
    assert [e["rung"] for e in exp] == [3, 2, 1] and lc.too_large(2400, exp[0]["tiles"][-1].desc, 1) and not lc.too_large(2400, exp[0]["tiles"][0].desc, 1)
    al = ConvexAlignHip(device=0, max_matrix_mb=1)
    try:
        res, ops, lad, info, _, _ = _run_ladder(al, exp)
        assert [int(x) for x in lad["rung"]] == [e["rung"] for e in exp]
        assert [int(x) for x in res["status"][:2]] == [4, 4] and int(res["status"][2]) == 0
        assert info["tiles"] == [sum(1 for e in exp if e["rung"] >= r + 1) for r in range(5)]
    finally:
        al.close()


def _mixed_cases(port_oracle, n=200, seed=9):
    """n tiles of 600 read bases, about a quarter of them with a deletion their first rung cannot hold"""
    from ngmlr_amd import synth
    rng = np.random.default_rng(seed)
    genome = synth.random_ref(rng, 4000)
    out = []
    for i in range(n):
        d = int(rng.choice([80, 130, 200, 300])) if i % 4 == 1 else int(rng.integers(0, 40))
        at = int(rng.integers(0, 4000 - 600 - d))
        ref = genome[at:at + 600 + d]
        qry = synth.mutate(rng, np.concatenate([ref[:300], ref[300 + d:]]), 0.03)
        ladder = (256, 0.0, 0.0, 0) if i % 3 else (256, 184.32, 184.32, lc.ANCHORS | (lc.REALIGN if i % 2 else 0))
        r, q = ref.tobytes(), qry.tobytes()
        rung, tiles = lc.climb(r, q, ladder, _valid(port_oracle))
        out.append(dict(tag="mixed%d" % i, ref=r, qry=q, ladder=ladder, rung=rung, tiles=tiles, live=True, port=port_oracle.align(tiles[-1])))
    return out


def test_a_ladder_job_between_two_jobs_waited_for_out_of_order(hip_aligner, port_oracle):
    from ngmlr_amd import synth
    cases = _mixed_cases(port_oracle)
    climbing = sum(1 for e in cases if e["rung"] > 1)
    assert 30 <= climbing <= 90, climbing
    tiles_a = synth.workload_ont(24, seed=3, max_len=1500)
    tiles_c = synth.workload_pacbio(12, seed=4, read_len=1200)
    alone = []
    for tiles in (tiles_a, tiles_c):
        j = hip_aligner.submit(tiles)
        r, o = j.wait()
        alone.append((r.tobytes(), o.tobytes()))
        j.release()
    res0, ops0, lad0, info0, _, _ = _run_ladder(hip_aligner, cases)
    _check_against_expectation(hip_aligner, cases, res0, ops0, lad0, info0, against=("port",))
    lad_tiles = [synth.Tile(e["ref"], e["qry"], np.zeros(0, np.int32), np.zeros(0, np.int32), desc=(2, 0.0, 0.0, 0.0, 0, 0)) for e in cases]
    ja = hip_aligner.submit(tiles_a)
    jb = hip_aligner.submit_ladder(lad_tiles, [e["ladder"] for e in cases])
    jc = hip_aligner.submit(tiles_c)
    rc, oc = jc.wait()      # returns although nobody has polled the ladder job
    assert (rc.tobytes(), oc.tobytes()) == alone[1]
    ra, oa = ja.wait()
    assert (ra.tobytes(), oa.tobytes()) == alone[0]
    rb, ob = jb.wait()
    assert rb.tobytes() == res0.tobytes() and ob.tobytes() == ops0.tobytes() and jb.ladder().tobytes() == lad0.tobytes()
    assert jb.ladder_info() == info0
    # polled instead of waited for: the same answer
    jp = hip_aligner.submit_ladder(lad_tiles, [e["ladder"] for e in cases])
    done = C.c_int32(0)
    for _ in range(2000000):
        assert hip_aligner.lib.cvx_job_poll(hip_aligner.h, jp.j, C.byref(done)) == 0
        if done.value:
            break
    assert done.value == 1
    rp, op = jp.wait()
    assert rp.tobytes() == res0.tobytes() and op.tobytes() == ops0.tobytes()
    for j in (ja, jb, jc, jp):
        j.release()


def test_with_a_resident_genome_no_window_is_decoded_twice(hip_aligner, port_oracle):
    """references as windows of the resident genome: the answer of the host-reference ladder, the windows form's window_refs,
    and not a sequence byte moved after the submit call"""
    from ngmlr_amd.aligner import Genome
    from oracle.pyoracle import DecodeOracle
    z = np.load(os.path.join(ROOT, "tests", "golden", "decode_test_3.npz"))
    starts = [int(x) for x in z["starts"]]
    orc = DecodeOracle()
    rng = np.random.default_rng(23)
    cases, positions = [], []
    for k in range(24):
        c = int(rng.integers(0, len(starts) - 1))
        d = int(rng.choice([0, 20, 100, 200, 300]))
        W = 600 + d
        p = int(rng.integers(starts[c], max(starts[c] + 1, starts[c + 1] - 1000 - W)))
        ref = orc.window(z["binref"], z["starts"], p, W + 1)[:W]
        r = np.frombuffer(ref, dtype=np.uint8)
        qry = np.concatenate([r[:300], r[300 + d:]]).tobytes()
        ladder = (256, 0.0, 0.0, 0) if k % 2 else (300, 150.0, 150.0, lc.ANCHORS)
        rung, tiles = lc.climb(ref, qry, ladder, _valid(port_oracle))
        cases.append(dict(tag="win%d" % k, ref=ref, qry=qry, ladder=ladder, rung=rung, tiles=tiles, live=True, port=port_oracle.align(tiles[-1])))
        positions.append(p)
    assert max(e["rung"] for e in cases) >= 3
    g = Genome(hip_aligner, z["binref"], int(z["nibbles"]), z["starts"])
    try:
        host = _run_ladder(hip_aligner, cases)
        from ngmlr_amd import synth
        tiles = [synth.Tile(e["ref"], e["qry"], np.zeros(0, np.int32), np.zeros(0, np.int32), desc=(2, 0.0, 0.0, 0.0, 0, 0)) for e in cases]
        job = hip_aligner.submit_ladder(tiles, [e["ladder"] for e in cases], genome=g, ref_positions=positions)
        res, ops = job.wait()
        assert res.tobytes() == host[0].tobytes() and ops.tobytes() == host[1].tobytes() and job.ladder().tobytes() == host[2].tobytes()
        _check_against_expectation(hip_aligner, cases, res, ops, job.ladder(), job.ladder_info(), against=("port",))
        assert job.ladder_info()["seq_bytes_after_submit"] == 0 and job.ladder_info()["rungs_run"] >= 3
        ptrs = (C.c_void_p * len(tiles))()
        assert hip_aligner.lib.cvx_job_window_refs(hip_aligner.h, job.j, ptrs) == 0
        mine = [C.string_at(p, len(t.ref)) for t, p in zip(tiles, ptrs)]
        plain = g.submit([e["tiles"][0] for e in cases], positions)
        plain.wait()
        ptrs2 = (C.c_void_p * len(tiles))()
        assert hip_aligner.lib.cvx_job_window_refs(hip_aligner.h, plain.j, ptrs2) == 0
        assert mine == [C.string_at(p, len(t.ref)) for t, p in zip(tiles, ptrs2)] == [e["ref"] for e in cases]
        plain.release()
        job.release()
    finally:
        g.free()


def test_a_scalar_twin_handle_climbs_with_the_twin_semantics(built):
    """tiles of the scalar twin's 'x' fixture (tests/golden/twin_x.npz) under ladders: the twin handle's ladder job against the
    same handle's sequential path, rung by rung"""
    from ngmlr_amd.aligner import ConvexAlignHip, format_alignment
    from oracle.pyoracle import same_alignment
    from tests import twin_cases
    from oracle.pyoracle import DEFAULT_PARAMS
    picked = [t for fam, p, t, _, _ in twin_cases.load("twin_x.npz") if p == DEFAULT_PARAMS and 0 < len(t.qry) <= 3000 and len(t.ref) > 0][:40]
    assert len(picked) >= 10 and any(b"x" in t.ref for t in picked)
    al = ConvexAlignHip(device=0, scalar_twin=True)
    try:
        cases = []
        for i, t in enumerate(picked):
            ladder = (max(8, len(t.ref) // 12), 0.0, 0.0, 0) if i % 2 else (len(t.ref) // 3, 20.0, 24.5, lc.ANCHORS)
            rung, tiles = lc.climb(t.ref, t.qry, ladder, lambda rt: al.batch_align([rt], want_nm=False)[0]["status"] == 0)
            cases.append(dict(tag=t.tag, ref=t.ref, qry=t.qry, ladder=ladder, rung=rung, tiles=tiles))
        assert len({e["rung"] for e in cases}) >= 2
        res, ops, lad, info, _, _ = _run_ladder(al, cases)
        assert [int(x) for x in lad["rung"]] == [e["rung"] for e in cases]
        want = al.batch_align([e["tiles"][-1] for e in cases])
        for i, e in enumerate(cases):
            got = format_alignment(al.lib, _as_result(res[i]), ops, e["tiles"][-1], scalar_twin=True)
            assert want[i]["status"] == got["status"] and same_alignment(want[i], got) is None, (e["tag"], same_alignment(want[i], got))
        assert info["tiles"] == [sum(1 for e in cases if e["rung"] >= r + 1) for r in range(5)]
    finally:
        al.close()


@pytest.mark.parametrize("kw", [dict(nm_regions=True), dict(job_text=True), dict(nm_regions=True, inv_checks=True), dict(nm_regions=True, job_text=True, scalar_twin=True)],
                         ids=["nm_regions", "job_text", "inv_checks", "all_with_twin"])
def test_flag_handles_refuse_the_call(built, kw):
    from ngmlr_amd import capi, synth
    from ngmlr_amd.aligner import ConvexAlignHip
    al = ConvexAlignHip(device=0, **kw)
    try:
        t = synth.Tile(b"ACGTACGTAC" * 10, b"ACGTACGTAC" * 9, np.zeros(0, np.int32), np.zeros(0, np.int32), desc=(2, 0.0, 0.0, 0.0, 0, 0))
        with pytest.raises(capi.CvxError) as err:
            al.submit_ladder([t], [(64, 0.0, 0.0, 0)])
        assert err.value.code == -3
        j = al.submit([synth.Tile(t.ref, t.qry, *synth.corridor_full(len(t.qry), len(t.ref)))])      # the handle is as usable as before
        r, _ = j.wait()
        assert int(r["status"][0]) == 0
        j.release()
    finally:
        al.close()


def test_a_service_handle_and_bad_ladders_are_refused(hip_aligner):
    from ngmlr_amd import capi, synth
    lib = hip_aligner.lib
    h = C.c_void_p()
    capi.check(lib.cvx_create_ex(0, C.byref(hip_aligner.params), 10000, capi.CREATE_SERVICE, C.byref(h)))
    t = synth.Tile(b"ACGTACGTAC" * 10, b"ACGTACGTAC" * 9, np.zeros(0, np.int32), np.zeros(0, np.int32), desc=(2, 0.0, 0.0, 0.0, 0, 0))
    arr, keep = hip_aligner._pack([t], closed_form=True)
    lad = capi.CvxLadder(64, 0.0, 0.0, 0)
    j = C.c_void_p()
    assert lib.cvx_submit_ladder(h, None, 1, arr, None, C.byref(lad), C.byref(j)) == -3
    lib.cvx_destroy(h)
    for bad in ((-1, 0.0, 0.0, 0), (64, 0.0, 0.0, 32), (64, float("nan"), 1.0, lc.ANCHORS)):
        with pytest.raises(capi.CvxError) as err:
            hip_aligner.submit_ladder([t], [bad])
        assert err.value.code == -3
    assert lib.cvx_submit_ladder(hip_aligner.h, None, 1, arr, None, None, C.byref(j)) == -3
    # the text stages of finished jobs do not take a ladder job; cvx_job_ladder does not take a plain one
    job = hip_aligner.submit_ladder([t], [(64, 0.0, 0.0, 0)])
    job.wait()
    with pytest.raises(capi.CvxError):
        job.text()
    assert len(job.ladder()) == 1
    job.release()
    plain = hip_aligner.submit([synth.Tile(t.ref, t.qry, *synth.corridor_full(len(t.qry), len(t.ref)))])
    plain.wait()
    with pytest.raises(capi.CvxError):
        plain.ladder()
    plain.release()
