"""GPU (-m gpu): asynchronous sub-read scoring (cvx_score_submit / poll / wait) on the shapes of ngmlr's interval check
(reference src/AlignmentBuffer.cpp:2515-2548) and inversion check (:1158-1235), against the reference's own StrippedSW + ssw
(ScoreOracle("reference"), oracle/_ref) and the C restatement (ScoreOracle("port")).  Scores are integers: bit-exact."""
import os
import threading

import numpy as np
import pytest

from ngmlr_amd import synth

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _oracles():
    from oracle.pyoracle import SCORE_REF_SO, ScoreOracle
    out = [ScoreOracle("port")]
    if os.path.exists(SCORE_REF_SO):
        out.append(ScoreOracle("reference"))
    return out


def _check(got, refs, qrys):
    for orc in _oracles():
        want = orc.scores(refs, qrys)
        bad = np.nonzero(got != want)[0]
        assert len(bad) == 0, (orc.lib.score_oracle_kind(), bad[:10], got[bad[:10]], want[bad[:10]],
                               [(len(refs[i]), len(qrys[i])) for i in bad[:10]])


def inversion_pairs(seed=41, n=48):
    """100 read bases against inversionLength + 500 reference bases, forward and reverse-complemented (:1158-1235)."""
    rng = np.random.default_rng(seed)
    refs, qrys = [], []
    for i in range(n):
        span = int(rng.integers(500, 5501))
        ref = synth.random_ref(rng, span)
        a = int(rng.integers(0, span - 100))
        piece = synth.mutate(rng, ref[a:a + 100], float(rng.choice([0.0, 0.05, 0.15])))
        if i % 4 == 3:
            piece = synth.random_ref(rng, 100)
        refs.append(ref.tobytes())
        qrys.append((synth.revcomp(piece) if i % 2 else piece).tobytes())
    return refs, qrys


def interval_pairs(seed=43, n=64):
    """A read piece of 0-1 023 bases (<= 1 024 with its NUL) against an interval's ref span of 50-30 000, identity 0.6-1.0 with
    indels; some pairs with the read as the longer string."""
    rng = np.random.default_rng(seed)
    refs, qrys = [], []
    for i in range(n):
        short = int(rng.integers(0, 1024)) if i % 8 else int(rng.choice([0, 1, 63, 64, 127, 128, 255, 256, 511, 512, 1023]))
        span = int(rng.integers(max(50, short), 30001)) if i % 3 else int(rng.integers(50, 2000))
        ref = synth.random_ref(rng, span)
        a = int(rng.integers(0, max(1, span - short)))
        read = synth.mutate(rng, ref[a:a + short], float(rng.uniform(0.0, 0.4)), ratio=(4, 4, 2))[:1023]
        if i % 5 == 4:
            refs.append(read.tobytes()); qrys.append(ref.tobytes())        # the read side as the longer one
        else:
            refs.append(ref.tobytes()); qrys.append(read.tobytes())
    return refs, qrys


def gapped_pair():
    """Two 400-base matches around a one-base insertion: 800 - 255 = 545 beats the best ungapped run (400)."""
    rng = np.random.default_rng(47)
    a, b = synth.random_ref(rng, 400).tobytes(), synth.random_ref(rng, 400).tobytes()
    ref = synth.random_ref(rng, 300).tobytes() + a + b + synth.random_ref(rng, 300).tobytes()
    return ref, a + b"G" + b


def odd_pairs():
    """Lower case, N / IUPAC codes, empty strings, 99 998 / 99 999 characters (lengths 99 999 / 100 000 with the NUL)."""
    rng = np.random.default_rng(53)
    big = synth.random_ref(rng, 99999).tobytes()
    w = synth.random_ref(rng, 900).tobytes()
    iupac = bytes(rng.choice(np.frombuffer(b"ACGTNRYKMSWBDHVnx-", np.uint8), 700))
    return ([w.lower(), w, iupac, b"", b"", b"ACGT", big[:99998], big, big[:600], big[:99998], big[:2000]],
            [w[100:600], w[100:600].lower(), w[:500], b"", b"ACGT", b"", big[5000:5900], big[:700], big[:99998], big[:99998][::-1][:1500], big[:99999]])


def rows_pairs(seed=59, n=6):
    """Both sides longer than 1 024: score_kernel's class."""
    rng = np.random.default_rng(seed)
    refs, qrys = [], []
    for _ in range(n):
        ref = synth.random_ref(rng, int(rng.integers(1100, 4000)))
        qrys.append(synth.mutate(rng, ref[: int(rng.integers(1025, len(ref)))], 0.1).tobytes())
        refs.append(ref.tobytes())
    return refs, qrys


def all_pairs(seed=61):
    parts = [inversion_pairs(), interval_pairs(), ([gapped_pair()[0]], [gapped_pair()[1]]), odd_pairs(), rows_pairs()]
    refs = [r for p in parts for r in p[0]]
    qrys = [q for p in parts for q in p[1]]
    perm = np.random.default_rng(seed).permutation(len(refs))
    return [refs[i] for i in perm], [qrys[i] for i in perm]


@pytest.fixture(scope="module")
def scorer(built):
    from ngmlr_amd.aligner import StrippedSWHip
    sw = StrippedSWHip(device=0)
    yield sw
    sw.close()


def test_inversion_shape(scorer):
    refs, qrys = inversion_pairs()
    job = scorer.submit_scores(refs, qrys)
    _check(job.wait(), refs, qrys)


def test_interval_shape(scorer):
    refs, qrys = interval_pairs()
    got = scorer.submit_scores(refs, qrys).wait()
    _check(got, refs, qrys)
    assert got.max() > 255        # scores above 255: ssw's word path
    assert scorer.kernel_ms() > 0.0


def test_only_a_gapped_path_wins(scorer):
    ref, qry = gapped_pair()
    got = scorer.submit_scores([ref, qry], [qry, ref]).wait()
    assert list(got) == [545.0, 545.0]
    _check(got, [ref, qry], [qry, ref])


def test_odd_strings_and_limits(scorer):
    refs, qrys = odd_pairs()
    got = scorer.submit_scores(refs, qrys).wait()
    assert got[7] == -1.0 and got[10] == -1.0                  # a string of 100 000 with its NUL
    assert got[3] == 0.0 and got[4] == 0.0 and got[5] == 0.0
    _check(got, refs, qrys)


def test_empty_call(scorer):
    job = scorer.submit_scores([], [])
    assert job.poll()
    assert len(job.wait()) == 0


def test_shuffled_mix_several_jobs_in_flight(scorer):
    refs, qrys = all_pairs()
    n = len(refs)
    cuts = [0, n // 5, n // 2, (3 * n) // 4, n]
    jobs = [scorer.submit_scores(refs[a:b], qrys[a:b]) for a, b in zip(cuts, cuts[1:])]
    whole = scorer.submit_scores(refs, qrys)
    got = np.concatenate([j.wait() for j in jobs])
    assert whole.poll() in (True, False)
    got_whole = whole.wait()
    _check(got, refs, qrys)
    assert np.array_equal(got, got_whole)
    # the blocking call keeps its own kernel choice and agrees
    assert np.array_equal(scorer.batch_score(refs, qrys), got)


def test_one_handle_per_thread(built):
    from ngmlr_amd.aligner import StrippedSWHip
    refs, qrys = all_pairs(seed=67)
    results, errors = {}, []

    def work(k):
        try:
            sw = StrippedSWHip(device=0)
            a = sw.submit_scores(refs[k::4], qrys[k::4])
            b = sw.submit_scores(refs[k::4][::-1], qrys[k::4][::-1])
            results[k] = (a.wait(), b.wait()[::-1])
            sw.close()
        except Exception as e:      # pragma: no cover - reported below
            errors.append(repr(e))
    ths = [threading.Thread(target=work, args=(k,)) for k in range(4)]
    [t.start() for t in ths]
    [t.join() for t in ths]
    assert not errors, errors
    got = np.zeros(len(refs), dtype=np.float32)
    for k in range(4):
        assert np.array_equal(results[k][0], results[k][1])
        got[k::4] = results[k][0]
    _check(got, refs, qrys)


def test_stage_kernel_ms_follows_the_last_scoring_call(scorer):
    from ngmlr_amd import capi
    import ctypes as C
    refs, qrys = interval_pairs(seed=71, n=8)
    scorer.submit_scores(refs, qrys).wait()
    ms = C.c_float()
    capi.check(scorer.lib.cvx_stage_kernel_ms(scorer._al.h, capi.STAGE_SCORE, C.byref(ms)))
    assert ms.value > 0.0
