"""CPU: scoring against the resident genome, host half.  cvx_stage_windows_host -- DecodeRefSequence and computeReverseSeq restated
(reference src/SequenceProvider.cpp:567-625, src/MappedRead.cpp:35-73) -- against what the unmodified reference did in
ScoreBuffer::DoRun, in scoreShortRead and on a list of engineered windows (tests/golden/score_windows_*.npz, recorded by
tools/make_golden_score_windows.sh), and the fixtures themselves against the scoring oracles."""
import ctypes as C

import numpy as np
import pytest

from tests import score_windows_fixtures as fx


@pytest.fixture(scope="module")
def lib(built):
    from ngmlr_amd import capi
    return capi.load()


@pytest.mark.parametrize("name", fx.NAMES)
def test_host_strings_equal_the_recording(lib, name):
    from ngmlr_amd.aligner import stage_windows_host
    f = fx.load(name)
    win, qry, status = stage_windows_host(lib, f.binref, f.nibbles, f.starts, f.reads, f.pairs)
    assert np.array_equal(status, 1 - f.ret)
    bad = [i for i in range(len(f.pairs)) if win[i] != f.win[i] or qry[i] != f.qry[i]]
    assert not bad, "pairs %s differ from the recording" % bad[:10]


def test_what_the_recordings_cover():
    t3, t2, cases = fx.load("test_3"), fx.load("test_2"), fx.load("cases")
    assert len(t3.pairs) == 1600 and not (1 - t3.ret).any() and not (1 - t2.ret).any()
    assert int(t3.reverse.sum()) >= 300 and int((1 - t3.reverse).sum()) >= 300
    assert (t2.kind == 1).any() and (t2.buffer_len[t2.kind == 1] & 1).any()          # scoreShortRead, an odd buffer length
    # the decodes that fail are exactly the last cases: position L, L + 5 and the wrapped value; position L - 1 decodes
    assert np.flatnonzero(cases.ret == 0).tolist() == list(range(len(cases.pairs) - fx.CASE_FAILURES, len(cases.pairs)))
    L = cases.concat_len
    assert cases.position[-4:].tolist() == [L - 1, L, L + 5, (5 - 20) & 0xFFFFFFFFFFFFFFFF]
    for par in ((0, 0), (0, 1), (1, 0), (1, 1)):
        assert any((p & 1, bl & 1) == par for p, bl, _, _ in cases.pairs)
    assert {3, 4, 5, 17, 308, 600} <= set(cases.buffer_len.tolist()) and 0 in cases.position.tolist()
    assert any(b"x" in w for w in cases.win) and any(w.endswith(b"xx") for w in cases.win)


@pytest.mark.parametrize("kind", ["port", "reference"])
@pytest.mark.parametrize("name", fx.NAMES)
def test_fixture_scores_are_the_oracles(built, name, kind):
    """fixture honesty: the recorded scores are what the scoring oracles give for the recorded strings"""
    from oracle.pyoracle import ScoreOracle, have_score_ref
    if kind == "reference" and not have_score_ref():
        pytest.skip("oracle/_ref not built")
    f = fx.load(name)
    ok = np.flatnonzero(f.ret == 1)
    got = ScoreOracle(kind).scores([f.win[i] for i in ok], [f.qry[i] for i in ok])
    assert np.array_equal(got.view(np.uint32), f.score[ok].view(np.uint32))
    assert (f.score[f.ret == 0] == -1.0).all()


@pytest.mark.parametrize("name", fx.NAMES)
def test_concat_len(lib, name):
    from ngmlr_amd.aligner import genome_concat_len
    f = fx.load(name)
    assert genome_concat_len(lib, f.nibbles, f.starts) == f.concat_len


def test_argument_errors(lib):
    from ngmlr_amd import capi
    from ngmlr_amd.aligner import stage_windows_host
    f = fx.load("cases")
    ok = (int(f.starts[2]), 308, 0, 0)
    for pairs in ([(ok[0], 2, 0, 0)], [ok, (ok[0], 308, len(f.reads), 1)], [(ok[0], 308, -1, 0)]):
        with pytest.raises(capi.CvxError) as e:
            stage_windows_host(lib, f.binref, f.nibbles, f.starts, f.reads, pairs)
        assert e.value.code == -3
    # an arena that is too small: CVX_ERR_CAPACITY with the need
    from ngmlr_amd.aligner import KmerIndex, _window_pairs
    arena, offsets, _ = KmerIndex.make_arena(f.reads)
    tab = _window_pairs([ok, ok])
    out = np.zeros(16, dtype=np.uint8)
    ro, qo = np.zeros(2, dtype=np.uint64), np.zeros(2, dtype=np.uint64)
    used = C.c_uint64()
    b, st = np.ascontiguousarray(f.binref), np.ascontiguousarray(f.starts, dtype=np.uint64)
    rc = lib.cvx_stage_windows_host(b.ctypes.data, f.nibbles, st.ctypes.data, len(st), len(f.reads), arena.ctypes.data, offsets.ctypes.data,
                                    2, tab.ctypes.data, out.ctypes.data, 16, ro.ctypes.data, qo.ctypes.data, None, C.byref(used))
    assert rc == -6 and used.value == 2 * (306 + 1 + len(f.reads[0]) + 1) and not out.any()
