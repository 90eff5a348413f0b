"""GPU (-m gpu): scoring against the resident genome (cvx_score_windows*, stage_score_windows_kernel of cvx_score_stage.hip).  The
strings the device writes and the scores behind them against what the unmodified reference did in ScoreBuffer::DoRun, in
scoreShortRead and on a list of engineered windows (tests/golden/score_windows_*.npz), and against cvx_stage_windows_host +
the scoring oracle where the cases are made here."""
import numpy as np
import pytest

from tests import score_windows_fixtures as fx

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sw(built):
    from ngmlr_amd.aligner import StrippedSWHip
    s = StrippedSWHip(device=0)
    yield s
    s.close()


@pytest.fixture(scope="module")
def genomes(sw):
    from ngmlr_amd.aligner import Genome
    gs = {name: Genome(sw._al, fx.load(name).binref, fx.load(name).nibbles, fx.load(name).starts) for name in fx.NAMES}
    yield gs
    for g in gs.values():
        g.free()


@pytest.fixture(scope="module")
def port(built):
    from oracle.pyoracle import ScoreOracle
    return ScoreOracle("port")


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float32).view(np.uint32), np.asarray(b, dtype=np.float32).view(np.uint32))


def _expect(sw, port, f, reads, pairs):
    """cvx_stage_windows_host + ScoreOracle("port"): (windows, queries, status, scores)"""
    from ngmlr_amd.aligner import stage_windows_host
    win, qry, status = stage_windows_host(sw.lib, f.binref, f.nibbles, f.starts, reads, pairs)
    scores = np.full(len(pairs), -1.0, dtype=np.float32)
    ok = np.flatnonzero(status == 0)
    scores[ok] = port.scores([win[i] for i in ok], [qry[i] for i in ok])
    return win, qry, status, scores


@pytest.mark.parametrize("name", fx.NAMES)
def test_a_staged_strings_equal_the_recording(sw, genomes, name):
    f = fx.load(name)
    win, qry, status = sw.stage_windows(genomes[name], f.reads, f.pairs)
    assert np.array_equal(status, 1 - f.ret)
    bad = [i for i in range(len(f.pairs)) if win[i] != f.win[i] or qry[i] != f.qry[i]]
    assert not bad, "pairs %s differ from the recording" % bad[:10]


@pytest.mark.parametrize("name", fx.NAMES)
def test_b_scores_equal_the_recording(sw, genomes, name):
    f = fx.load(name)
    scores, status = sw.score_windows(genomes[name], f.reads, f.pairs)
    assert np.array_equal(status, 1 - f.ret)
    assert _same_bits(scores, f.score), np.flatnonzero(scores != f.score)[:10]
    assert sw.kernel_ms() > 0.0 and 0.0 < sw.stage_kernel_ms() <= sw.kernel_ms()


def test_c_one_call_both_strands_of_the_same_reads(sw, genomes, port):
    """reads of 1, 255, 256 and 257 bases, N and bytes outside ACGTN, both strands of every read in one call, and one pair beyond the
    diagonal kernel's shape (a read of 600 against buffer_len 900), so that a wave class runs behind the stage kernel"""
    f = fx.load("test_3")
    rng = np.random.default_rng(5)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    reads = [bytes(rng.choice(letters, size=n)) for n in (1, 255, 256, 257, 300, 600)]
    reads[4] = reads[4][:50] + b"NNNN" + reads[4][54:120] + b"acgtRY-*" + reads[4][128:]
    # read 5 begins with a piece of the genome, so that its long pair has a score worth comparing
    reads[5] = (f.win[0][20:20 + 290] + reads[5])[:600]
    pairs = []
    for r in range(len(reads)):
        for pos in (60000 + 977 * r, 60001 + 977 * r):
            pairs.append((pos, 308 + (r & 1), r, 0))
            pairs.append((pos, 308 + (r & 1), r, 1))
    pairs.append((f.pairs[0][0], 900, 5, 0))
    pairs.append((f.pairs[0][0] + 1, 901, 5, 1))
    win, qry, status, want = _expect(sw, port, f, reads, pairs)
    assert not status.any() and len(qry[-1]) == 600 and len(win[-2]) > 512
    assert sw.stage_windows(genomes["test_3"], reads, pairs)[:2] == (win, qry)
    scores, st = sw.score_windows(genomes["test_3"], reads, pairs)
    assert not st.any() and _same_bits(scores, want), (scores, want)
    assert want[-2] > 100.0      # (the long pair aligned: its score is no accident of an empty DP)


def test_d_two_jobs_in_flight(sw, genomes):
    a, b = fx.load("test_3"), fx.load("cases")
    pa = a.pairs[:300]
    want_a, _ = sw.score_windows(genomes["test_3"], a.reads, pa)
    want_b, _ = sw.score_windows(genomes["cases"], b.reads, b.pairs)
    ja = sw.submit_windows(genomes["test_3"], a.reads, pa)
    jb = sw.submit_windows(genomes["cases"], b.reads, b.pairs)
    got_b = jb.wait()
    got_a = ja.wait()
    assert _same_bits(got_a, want_a) and _same_bits(got_b, want_b)
    assert _same_bits(got_a, a.score[:300]) and _same_bits(got_b, b.score)      # (-1.0 where the decode fails)


def test_e_a_full_call_equals_the_string_path(sw, genomes):
    f = fx.load("test_3")
    idx = np.arange(576, 1600)      # 1 024 distinct recorded pairs (the call size of ScoreBuffer), both strands
    pairs = [f.pairs[i] for i in idx]
    scores, status = sw.score_windows(genomes["test_3"], f.reads, pairs)
    want = sw.batch_score([f.win[i] for i in idx], [f.qry[i] for i in idx])
    assert not status.any() and _same_bits(scores, want) and _same_bits(scores, f.score[idx])


def test_f_every_alignment_of_the_arena(sw, genomes, port):
    """strings that begin at all 16 offsets modulo 16 of the sequence arena: the kernel's byte-wise heads and tails around its
    16-byte pieces, windows and queries of both strands"""
    f = fx.load("test_3")
    reads = [f.reads[0][:37], f.reads[1][:64], f.reads[2]]
    pairs = [(70000 + 13 * k + (k & 1), 20 + (k * 7) % 47, k % 3, (k >> 1) & 1) for k in range(64)]
    win, qry, status, want = _expect(sw, port, f, reads, pairs)
    # one class (the diagonal kernel), so the slots lie in call order: string k begins where the ones before it end
    at, ref_at, qry_at = 0, set(), set()
    for w, q in zip(win, qry):
        ref_at.add(at % 16); at += len(w) + 1
        qry_at.add(at % 16); at += len(q) + 1
    assert ref_at == set(range(16)) and qry_at == set(range(16))
    assert sw.stage_windows(genomes["test_3"], reads, pairs)[:2] == (win, qry)
    scores, _ = sw.score_windows(genomes["test_3"], reads, pairs)
    assert _same_bits(scores, want)


def test_argument_errors(sw, genomes):
    from ngmlr_amd import capi
    f = fx.load("cases")
    ok = (int(f.starts[2]), 308, 0, 0)
    for pairs in ([(ok[0], 2, 0, 0)], [ok, (ok[0], 308, len(f.reads), 1)], [(ok[0], 308, -1, 0)]):
        with pytest.raises(capi.CvxError) as e:
            sw.score_windows(genomes["cases"], f.reads, pairs)
        assert e.value.code == -3
    scores, status = sw.score_windows(genomes["cases"], f.reads, [ok])      # (the handle still works)
    assert status[0] == 0 and scores[0] >= 0.0
