"""CPU: cvx_inv_checks_host, the rule of checkForSV (reference src/AlignmentBuffer.cpp:1158-1235) on the host -- against every
call the unmodified reference made on test_3 and on the split-read workload (tests/golden/inv_checks_*.npz, recorded by
tools/make_golden_inv_checks.sh: outcome and both score bit patterns), and on engineered calls against the rule restated in
tests/inv_check_cases.py over windows from cvx_stage_windows_host and scores from the score oracle."""
import numpy as np
import pytest

from tests import inv_check_cases as cases


@pytest.fixture(scope="module")
def lib(built):
    from ngmlr_amd import capi
    return capi.load()


@pytest.fixture(scope="module")
def oracle(built):
    from oracle.pyoracle import ScoreOracle, have_score_ref
    return ScoreOracle("reference" if have_score_ref() else "port")


def _host(lib, genome, calls, empty_tiles=False):
    from ngmlr_amd import aligner
    args = cases.as_tiles(calls)
    if empty_tiles:
        args = cases.with_empty_tiles(args)
    return aligner.inv_checks_host(genome[0], genome[1], genome[2], *args, lib=lib)


def _same(want, got, calls, fields=("status", "score_fwd", "score_rev", "window_chars")):
    bad = [(c.tag, tuple(w[f] for f in fields), tuple(g[f] for f in fields)) for c, w, g in zip(calls, want, got)
           if any(w[f].tobytes() != g[f].tobytes() for f in fields)]
    assert not bad, bad[:5]


@pytest.mark.parametrize("name", cases.RECORDED)
def test_recorded_reference_calls(lib, name):
    """outcome and both score bit patterns of every call; the window's length where the reference decoded one"""
    genome, calls, z = cases.recorded(lib, name)
    want = cases.recorded_records(z)
    got = _host(lib, genome, calls)
    assert len(got) == int(z["n"]) > 1000
    ran = z["outcome"] == 0
    # the reference cannot tell an empty window from one that did not decode: none of the recorded calls has one
    assert (z["ref_chars"][ran] > 0).all()
    _same(want, got, calls, ("status", "score_fwd", "score_rev"))
    assert np.array_equal(got["window_chars"][ran], z["ref_chars"][ran])
    assert (got["window_chars"][~ran] == 0).all()
    assert int((got["score_rev"] > got["score_fwd"]).sum()) >= 8


def test_engineered_calls(lib, oracle):
    genome, calls = cases.engineered(lib)
    want = cases.expected(lib, genome, calls, oracle)
    got = _host(lib, genome, calls)
    _same(want, got, calls)
    by = {c.tag: w for c, w in zip(calls, want)}
    # every family of the issue is there and means what its tag says
    assert by["invLen 10"]["status"] == cases.TOO_SHORT and by["invLen 11"]["status"] == cases.SCORED
    assert by["invLen 11, stop before start"]["status"] == cases.SCORED
    assert by["midRead 49"]["status"] == cases.NO_READ and by["midRead 50"]["status"] == cases.SCORED
    assert by["midRead + 50 == H"]["status"] == cases.NO_READ and by["midRead + 50 == H - 1"]["status"] == cases.SCORED
    assert by["midRead negative"]["status"] == cases.NO_READ
    assert {511, 2047, 2048, 2049, 6000} <= set(int(x) for x in want["window_chars"])
    assert by["planted inversion"]["score_rev"] > by["planted inversion"]["score_fwd"] and by["planted inversion"]["score_rev"] >= 60
    assert by["position at L -1"]["status"] == cases.SCORED and by["position at L +0"]["status"] == cases.NO_WINDOW
    assert by["position at L +1"]["status"] == cases.NO_WINDOW and by["below zero"]["status"] == cases.NO_WINDOW
    assert by["position zero"]["status"] == cases.SCORED and by["across the spacer"]["score_fwd"] >= 30
    assert by["into the spacer only"]["score_fwd"] == 0 and by["into the spacer only"]["window_chars"] > 500
    for w in want[want["status"] != cases.SCORED]:
        # whatever the reference's scorer gives ("", read) where the window does not decode, 0.0f where nothing is scored
        assert w["score_fwd"] == 0 and w["score_rev"] == 0 and w["window_chars"] == 0
    assert len({int(p[1]) & 1 for p in (c.plan() for c in calls) if p[0] is None}) == 2
    assert len({int(x) & 1 for x in want["window_chars"][want["status"] == cases.SCORED]}) == 2


def test_tiles_without_regions_between_the_others(lib):
    genome, calls = cases.engineered(lib)
    assert _host(lib, genome, calls).tobytes() == _host(lib, genome, calls, empty_tiles=True).tobytes()


def test_windows_at_the_scorers_length_limit(lib, oracle):
    """a window of 99 998 characters is scored, one of 99 999 (100 000 bytes with its NUL) gives -1.0f (src/StrippedSW.cpp:174)"""
    genome, calls = cases.long_genome(lib)
    want = cases.expected(lib, genome, calls, oracle)
    got = _host(lib, genome, calls)
    _same(want, got, calls)
    assert [int(x) for x in want["window_chars"]] == [99998, 99999, 99996]
    assert want["score_fwd"][0] >= 60 and want["score_fwd"][1] == -1.0 and want["score_rev"][1] == -1.0 and want["score_fwd"][2] >= 60


def test_arguments(lib):
    from ngmlr_amd import aligner, capi
    genome, calls = cases.engineered(lib)
    qrys, pos, po, off, reg = cases.as_tiles(calls[6:14])      # four regions of one tile, then tiles of two
    assert len(qrys) >= 3
    g = (genome[0], genome[1], genome[2])
    bad = off.copy()
    bad[0] = 1
    with pytest.raises(AssertionError):      # (the binding's own check of region_off[n] against the regions)
        aligner.inv_checks_host(*g, qrys, pos, po, off, reg[:-1], lib=lib)
    chk = np.zeros(len(reg), dtype=aligner.INV_CHECK_DTYPE)
    ql = np.array([len(q) for q in qrys], dtype=np.int32)
    import ctypes as C
    arr = (C.c_char_p * len(qrys))(*qrys)

    def call(off_, ql_=ql, bin_=genome[0].ctypes.data):
        return lib.cvx_inv_checks_host(bin_, genome[1], genome[2].ctypes.data, len(genome[2]), len(qrys), arr, ql_.ctypes.data, pos.ctypes.data,
                                       po.ctypes.data, off_.ctypes.data, reg.ctypes.data, chk.ctypes.data)
    assert call(off) == 0
    assert call(bad) == -3 and b"region_off" in lib.cvx_last_error()
    desc = off.copy()
    desc[1] = desc[2] + 1      # (the first tile's end behind the second's)
    assert call(desc) == -3
    neg = ql.copy()
    neg[0] = -1
    assert call(off, neg) == -3
    assert call(off, ql, None) == -3
    assert len(aligner.inv_checks_host(*g, [], [], [], [0], np.zeros((0, 4), dtype=np.int32), lib=lib)) == 0
