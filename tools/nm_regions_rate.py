"""Dev tool (GPU): the region scan of the NM profile on the device (cvx_job_nm_regions: nm_regions_kernel, both passes and
the offset scan) against the profile kernel it replaces for a consumer of regions (cvx_job_nm_profile with a NULL buffer:
nm_profile_kernel, triples left in HBM) -- device time of the kernels (HIP events) on the same tile ranges of one job of
PacBio 10 kb tiles, alternating in one process -- plus the whole job in one cvx_job_nm_regions call: wall time up to the call's
own synchronise, bytes brought back, bytes the triples would have been.

    python tools/nm_regions_rate.py [tiles [tiles_per_range [reps]]]
"""
import ctypes as C
import multiprocessing as mp
import os
import statistics
import sys
import time
from concurrent.futures import ProcessPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from ngmlr_amd import synth  # noqa: E402


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 49152
    per = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 7
    # tiles first: the worker processes are forked before HIP exists
    with ProcessPoolExecutor(max(1, min(os.cpu_count() or 1, 16)), mp_context=mp.get_context("fork")) as pool:
        ts = synth.pacbio_tileset(n, seed=7, pool=pool)
    from ngmlr_amd import capi
    from ngmlr_amd.aligner import ConvexAlignHip
    al = ConvexAlignHip(device=0)
    ts.use_closed_form()
    ts.pin(al.lib)
    job = al.submit(ts)
    job.wait()
    recs, _off, _buf = job.text_raw()
    valid = sum(1 for i in range(n) if recs[i].ret >= 0)
    columns = sum(recs[i].alignment_length for i in range(n) if recs[i].ret >= 0)
    print("%d PacBio 10 kb tiles (%d valid, %.1f M alignment columns), ranges of %d tiles, %d repetitions, both kernels alternating"
          % (n, valid, columns / 1e6, per, reps))
    ranges = [(f, min(per, n - f)) for f in range(0, n, per)]
    job.nm_regions(0, ranges[0][1])          # first-call allocations stay out of the numbers
    job.nm_profile(0, ranges[0][1], to_host=False)
    reg_ms = {r: [] for r in ranges}
    pro_ms = {r: [] for r in ranges}
    entries = regions = 0
    for rep in range(reps):
        for r in ranges:
            off, reg, _opn, ms = job.nm_regions(*r)
            reg_ms[r].append(ms)
            poff, _none, pms = job.nm_profile(r[0], r[1], to_host=False)
            pro_ms[r].append(pms)
            if rep == 0:
                entries += int(poff[r[1]])
                regions += len(reg)
    print("range          regions kernels ms: min / median / max      profile kernel ms: min / median / max      median ratio")
    for r in ranges:
        a, b = reg_ms[r], pro_ms[r]
        print("  %6d +%5d   %9.3f / %9.3f / %9.3f           %9.3f / %9.3f / %9.3f              x%.2f" % (
            r[0], r[1], min(a), statistics.median(a), max(a), min(b), statistics.median(b), max(b), statistics.median(b) / statistics.median(a)))
    tot_a = [sum(reg_ms[r][k] for r in ranges) for k in range(reps)]
    tot_b = [sum(pro_ms[r][k] for r in ranges) for k in range(reps)]
    print("all ranges, per repetition, regions kernels ms: %s" % " ".join("%.2f" % v for v in tot_a))
    print("all ranges, per repetition, profile kernel ms:  %s" % " ".join("%.2f" % v for v in tot_b))
    print("all ranges, median over repetitions: regions kernels %.2f ms (spread %.2f .. %.2f), profile kernel %.2f ms (spread %.2f .. %.2f), profile / regions x%.2f"
          % (statistics.median(tot_a), min(tot_a), max(tot_a), statistics.median(tot_b), min(tot_b), max(tot_b),
             statistics.median(tot_b) / statistics.median(tot_a)))
    # the whole job in one call
    lib = al.lib
    off = np.zeros(n + 1, dtype=np.uint64)
    ptr = C.c_void_p()
    kms = C.c_double()
    opn = np.zeros(n, dtype=np.dtype([("open", np.int32), ("distance", np.int32), ("region", np.int32, (4,))]))
    walls, kern = [], []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        capi.check(lib.cvx_job_nm_regions(al.h, job.j, 0, n, off.ctypes.data, C.byref(ptr), opn.ctypes.data, C.byref(kms)))
        walls.append((time.perf_counter() - t0) * 1e3)
        kern.append(kms.value)
    walls, kern = walls[1:], kern[1:]
    back = 8 * (n + 1) + 24 * n + 16 * int(off[n])
    print("whole job, one cvx_job_nm_regions call (%d tiles): wall %.2f ms median (%.2f .. %.2f), of which kernels %.2f ms median"
          % (n, statistics.median(walls), min(walls), max(walls), statistics.median(kern)))
    print("  regions found %d (%.2f per valid tile), tiles whose scan ends in an open run %d" % (int(off[n]), int(off[n]) / max(valid, 1), int(opn["open"].sum())))
    print("  bytes brought back %d (offsets %d + end states %d + regions %d); the triples would have been %d bytes (12 x %d entries): x%.0f less"
          % (back, 8 * (n + 1), 24 * n, 16 * int(off[n]), 12 * entries, entries, 12 * entries / back))
    assert regions == int(off[n]), (regions, int(off[n]))
    job.release()
    al.close()


if __name__ == "__main__":
    main()
