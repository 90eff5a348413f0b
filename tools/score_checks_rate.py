"""Dev tool (GPU): the scoring kernel of ngmlr's interval / inversion checks (score_wave_kernel, cvx_score_wave.hip) against
score_kernel, which cvx_score_batch picks for any call with a window over 512 columns (cvx_score.hip) -- device time of the
kernels (CVX_STAGE_SCORE, HIP events) and G cell updates/s on the same pairs -- plus the whole-call rate of cvx_score_submit
(strings in host memory in, scores out) on a mixed batch, and the reference's StrippedSW + ssw on one core for scale.

    python tools/score_checks_rate.py [pairs_per_batch]
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from ngmlr_amd import synth  # noqa: E402
from ngmlr_amd.aligner import StrippedSWHip  # noqa: E402
from oracle.pyoracle import ScoreOracle, have_score_ref  # noqa: E402


def interval(rng, n, short, long_):
    refs, qrys = [], []
    for _ in range(n):
        s = int(rng.integers(*short))
        L = int(rng.integers(max(s, long_[0]), long_[1]))
        ref = synth.random_ref(rng, L)
        a = int(rng.integers(0, max(1, L - s)))
        qrys.append(synth.mutate(rng, ref[a:a + s], float(rng.uniform(0.0, 0.4)), ratio=(4, 4, 2))[:1023].tobytes())
        refs.append(ref.tobytes())
    return refs, qrys


def cells(refs, qrys):
    return sum((len(r) + 1) * (len(q) + 1) for r, q in zip(refs, qrys))


def best_of(fn, reps=3):
    out = []
    for _ in range(reps):
        out.append(fn())
    return min(out)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    rng = np.random.default_rng(7)
    sw = StrippedSWHip(device=0)
    kind = "reference" if have_score_ref() else "port"
    orc = ScoreOracle(kind)
    shapes = [("inversion 100 x 500-5500", n, (100, 101), (500, 5501)),
              ("interval 100-1000 x 1000-5000", n, (100, 1001), (1000, 5001)),
              ("interval 900-1000 x 5000", n // 2, (900, 1001), (5000, 5001)),
              ("interval 1-1023 x 50-30000", n // 4, (1, 1024), (50, 30001))]
    print("device time of the kernels (min of 3), G cell updates/s")
    for name, m, short, long_ in shapes:
        refs, qrys = interval(rng, m, short, long_)
        c = cells(refs, qrys)
        sw.submit_scores(refs[:8], qrys[:8]).wait()

        def wave():
            sw.submit_scores(refs, qrys).wait()
            return sw.kernel_ms()

        def rows():
            sw.batch_score(refs, qrys)
            return sw.kernel_ms()
        ms_w, ms_r = best_of(wave), best_of(rows)
        got, base = sw.submit_scores(refs, qrys).wait(), sw.batch_score(refs, qrys)
        print("  %-32s %5d pairs: score_wave_kernel %8.3f ms %7.1f Gcells/s | score_kernel %8.3f ms %7.1f Gcells/s | x%.1f | equal %s" % (
            name, m, ms_w, c / ms_w / 1e6, ms_r, c / ms_r / 1e6, ms_r / ms_w, bool(np.array_equal(got, base))))
    # one pair on one wave: the latency a lone check sees
    refs, qrys = interval(rng, 1, (1000, 1001), (5000, 5001))
    c = cells(refs, qrys)
    sw.submit_scores(refs, qrys).wait()
    ms_w = best_of(lambda: (sw.submit_scores(refs, qrys).wait(), sw.kernel_ms())[1])
    ms_r = best_of(lambda: (sw.batch_score(refs, qrys), sw.kernel_ms())[1])
    t0 = time.perf_counter()
    orc.scores(refs * 5, qrys * 5)
    cpu_ms = (time.perf_counter() - t0) * 1e3 / 5
    print("  one 1000 x 5000 pair:            score_wave_kernel %8.3f ms | score_kernel %8.3f ms | %s StrippedSW one core %.3f ms" % (
        ms_w, ms_r, kind, cpu_ms))
    # whole calls on a mixed batch: diag-class sub-reads, inversion and interval checks, a few pairs for score_kernel
    refs, qrys = [], []
    for spec in ((n // 2, (256, 257), (300, 309)), (n // 4, (100, 101), (500, 5501)), (n // 4 - 8, (1, 1024), (50, 10001)), (8, (1100, 1500), (1600, 3000))):
        r, q = interval(rng, *spec)
        refs += r
        qrys += q
    perm = rng.permutation(len(refs))
    refs, qrys = [refs[i] for i in perm], [qrys[i] for i in perm]
    c = cells(refs, qrys)
    sw.submit_scores(refs, qrys).wait()
    t0 = time.perf_counter()
    reps = 5
    for _ in range(reps):
        got = sw.submit_scores(refs, qrys).wait()
    dt = (time.perf_counter() - t0) / reps
    t1 = time.perf_counter()
    jobs = [sw.submit_scores(refs, qrys) for _ in range(reps)]
    [j.wait() for j in jobs]
    dt2 = (time.perf_counter() - t1) / reps
    t0 = time.perf_counter()
    want = orc.scores(refs, qrys)
    cpu = time.perf_counter() - t0
    print("  mixed batch of %d pairs, whole cvx_score_submit + wait: %.2f ms per call (%.1f Gcells/s, %.0f k pairs/s); %d jobs in flight: %.2f ms per call" % (
        len(refs), dt * 1e3, c / dt / 1e9, len(refs) / dt / 1e3, reps, dt2 * 1e3))
    print("  the same batch, %s StrippedSW on one core: %.1f ms; parity %d/%d" % (kind, cpu * 1e3, int((got == want).sum()), len(refs)))
    sw.close()


if __name__ == "__main__":
    main()
