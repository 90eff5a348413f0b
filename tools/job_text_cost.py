#!/usr/bin/env python3
"""What a job pays for bringing its CIGAR / MD strings back with its results (CVX_CREATE_JOB_TEXT): one PacBio-shaped step through
a plain handle (what every handle did before the flag), a regions handle and a regions + text handle, all in this process,
alternating, `--runs` runs each.  Prints per run the step's wall time (submit -> wait returned) and the compute stage's device
time (cvx_timing.total_ms), then the medians and differences, and what cvx_job_text (two round trips on the text stream) costs
on the plain handle for comparison.

    python tools/job_text_cost.py --tiles 24576 --runs 5 >> profiles/r21_job_text.txt
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NAMES = ("plain", "regions", "regions+text")


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=24576)
    ap.add_argument("--read-len", type=int, default=10000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--create", default=",".join(NAMES),
                    help="the order in which the three handles are created (a process's streams share its hardware queues: the handle created last need not get the queues the first one got)")
    args = ap.parse_args()
    from ngmlr_amd import synth
    from ngmlr_amd.aligner import ConvexAlignHip
    ts = synth.pacbio_tileset(args.tiles, seed=args.seed, read_len=args.read_len)
    order = args.create.split(",")
    assert sorted(order) == sorted(NAMES), "--create takes the three names %s in some order" % (NAMES,)
    handles = {name: ConvexAlignHip(device=0, nm_regions=name != "plain", job_text=name == "regions+text") for name in order}
    print("# %d PacBio tiles of %d bases, build %s, fill %s; handles created in the order %s" % (
        args.tiles, args.read_len, handles["plain"].lib.cvx_build_id().decode(), handles["plain"].lib.cvx_source_id(b"fill").decode(), ", ".join(order)))
    wall = {k: [] for k in NAMES}
    dev = {k: [] for k in NAMES}
    ref = None
    for run in range(-1, args.runs):      # run -1 warms the handles up (allocations, code objects)
        order = NAMES[run % 3:] + NAMES[:run % 3]
        for name in order:
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
            if name == "regions+text":
                info = job.texts_info()
                extra = "  text %d bytes (arena first held %d, %d rewrites)" % (info["total_bytes"], info["first_capacity"], info["rewrites"])
            job.release()
            if run >= 0:
                wall[name].append((t1 - t0) * 1e3)
                dev[name].append(tm.total_ms)
            print("run %2d  %-12s  wall %8.2f ms  device %8.2f ms (fill %.2f, walk and after %.2f)%s" % (
                run, name, (t1 - t0) * 1e3, tm.total_ms, tm.fill_ms, tm.backtrack_ms, extra))
            sys.stdout.flush()
    for name in NAMES:
        print("%-12s  wall median %8.2f ms (min %.2f, max %.2f)  device median %8.2f ms (min %.2f, max %.2f)" % (
            name, np.median(wall[name]), min(wall[name]), max(wall[name]), np.median(dev[name]), min(dev[name]), max(dev[name])))
    for a, b in (("regions", "plain"), ("regions+text", "regions"), ("regions+text", "plain")):
        print("%s - %s  wall %+.2f ms  device %+.2f ms  (spread of the repeats: wall %.2f / %.2f ms, device %.2f / %.2f ms)" % (
            a, b, np.median(wall[a]) - np.median(wall[b]), np.median(dev[a]) - np.median(dev[b]),
            max(wall[a]) - min(wall[a]), max(wall[b]) - min(wall[b]), max(dev[a]) - min(dev[a]), max(dev[b]) - min(dev[b])))
    # the entry with two round trips of its own, on the plain handle
    times = []
    for _ in range(3):
        job = handles["plain"].submit(ts)
        job.wait()
        t0 = time.perf_counter()
        _out, _off, buf = job.text_raw()
        t1 = time.perf_counter()
        n_bytes = len(buf) if buf is not None else 0
        job.release()
        times.append((t1 - t0) * 1e3)
    print("plain handle: cvx_job_text after cvx_wait %.2f ms wall (median of %s), %d bytes of text" % (
        np.median(times), ", ".join("%.2f" % t for t in times), n_bytes))
    for al in handles.values():
        al.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
