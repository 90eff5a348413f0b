#!/usr/bin/env python3
"""What a job pays for finding its low-identity regions with its results (CVX_CREATE_NM_REGIONS): one PacBio-shaped step through
a plain handle and through a handle with the flag, both in this process, alternating, `--runs` runs each.  Prints per run the
step's wall time (submit -> wait returned) and the compute stage's device time (cvx_timing.total_ms), then the medians, the
difference, and what the two-round-trip entry (text stage + cvx_job_nm_regions) costs on the plain handle for comparison.

    python tools/job_regions_cost.py --tiles 24576 --runs 5 > profiles/r19_job_regions.txt
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=24576)
    ap.add_argument("--read-len", type=int, default=10000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--seed", type=int, default=7)
    args = ap.parse_args()
    from ngmlr_amd import synth
    from ngmlr_amd.aligner import ConvexAlignHip
    ts = synth.pacbio_tileset(args.tiles, seed=args.seed, read_len=args.read_len)
    handles = {"off": ConvexAlignHip(device=0), "on": ConvexAlignHip(device=0, nm_regions=True)}
    print("# %d PacBio tiles of %d bases, build %s" % (args.tiles, args.read_len, handles["off"].lib.cvx_build_id().decode()))
    wall = {"off": [], "on": []}
    dev = {"off": [], "on": []}
    ref = None
    for run in range(-1, args.runs):      # run -1 warms both handles up (allocations, code objects)
        for name in ("off", "on") if run % 2 == 0 else ("on", "off"):
            al = handles[name]
            t0 = time.perf_counter()
            job = al.submit(ts)
            res, ops = job.wait()
            t1 = time.perf_counter()
            tm = job.timing()
            sig = (res.tobytes(), ops.tobytes())
            if ref is None:
                ref = sig
            assert sig == ref, "results differ between the handles"
            extra = ""
            if name == "on":
                info = job.regions_info()
                extra = "  regions %d (arena first held %d, %d rewrites)" % (info["total"], info["first_capacity"], info["rewrites"])
            job.release()
            if run >= 0:
                wall[name].append((t1 - t0) * 1e3)
                dev[name].append(tm.total_ms)
            print("run %2d  flag %-3s  wall %8.2f ms  device %8.2f ms (fill %.2f, walk and after %.2f)%s" % (
                run, name, (t1 - t0) * 1e3, tm.total_ms, tm.fill_ms, tm.backtrack_ms, extra))
    for name in ("off", "on"):
        print("flag %-3s  wall median %8.2f ms (min %.2f, max %.2f)  device median %8.2f ms (min %.2f, max %.2f)" % (
            name, np.median(wall[name]), min(wall[name]), max(wall[name]), np.median(dev[name]), min(dev[name]), max(dev[name])))
    print("on - off  wall %+.2f ms  device %+.2f ms  (spread of the repeats: wall %.2f / %.2f ms, device %.2f / %.2f ms)" % (
        np.median(wall["on"]) - np.median(wall["off"]), np.median(dev["on"]) - np.median(dev["off"]),
        max(wall["off"]) - min(wall["off"]), max(wall["on"]) - min(wall["on"]), max(dev["off"]) - min(dev["off"]), max(dev["on"]) - min(dev["on"])))
    # the two-round-trip entry on the plain handle, after its device text stage
    job = handles["off"].submit(ts)
    job.wait()
    t0 = time.perf_counter()
    job.text_raw()
    t1 = time.perf_counter()
    _off, reg, _opn, ms = job.nm_regions()
    t2 = time.perf_counter()
    job.release()
    print("plain handle: device text stage %.2f ms, then cvx_job_nm_regions %.2f ms wall (%.2f ms in its kernels), %d regions" % (
        (t1 - t0) * 1e3, (t2 - t1) * 1e3, ms, len(reg)))
    for al in handles.values():
        al.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
