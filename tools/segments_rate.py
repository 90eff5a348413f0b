#!/usr/bin/env python
"""What taking alignment queries as segments of a read block costs and saves, per call (needs an MI355X).

  A  cvx_submit            host-built queries: every tile's string packed into the job's staging and sent over PCIe
  B  cvx_submit_segments   the call's distinct reads sent once, 16 bytes per tile, stage_segments_kernel writes the strings

alternating on one handle: wall time of the submit call (the host side: packing against copying the read block), bytes of query
that cross PCIe, wall time until the job's results are back; and the kernel alone (cvx_stage_segments, HIP events) in GB/s read +
written, to hold against the streaming-copy figure of the device.

  python tools/segments_rate.py [--tiles 4096] [--read-len 10000] [--per-read 4] [--reps 5]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ngmlr_amd import capi, synth  # noqa: E402
from ngmlr_amd.aligner import ConvexAlignHip, SEGMENT_DTYPE  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=4096)
    ap.add_argument("--read-len", type=int, default=10000)
    ap.add_argument("--per-read", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    ts = synth.pacbio_tileset(a.tiles, read_len=a.read_len).use_closed_form(True)
    n = len(ts)
    tab = ts.table()
    # the read block: per_read tiles share a read; every other tile lies reverse-complemented in it (half the tiles CVX_SEG_REVCOMP)
    seg = np.zeros(n, dtype=SEGMENT_DTYPE)
    parts, offsets, at, read = [], [0], 0, 0
    for i in range(n):
        q = ts.qry[int(ts.qry_off[i]):int(ts.qry_off[i + 1])]
        seg[i] = (read, at - offsets[-1], i & 1, 0)
        parts.append(synth.revcomp(q) if i & 1 else q)
        at += len(q)
        if (i + 1) % a.per_read == 0 or i + 1 == n:
            parts.append(np.zeros(1, dtype=np.uint8))
            at += 1
            offsets.append(at)
            read += 1
    arena = np.concatenate(parts + [np.zeros(64, dtype=np.uint8)])
    offsets = np.array(offsets, dtype=np.uint64)
    n_reads = len(offsets) - 1
    tab_seg = tab.copy()
    tab_seg["qry"] = 0
    al = ConvexAlignHip(device=0)
    lib = al.lib

    def run(which):
        j = C.c_void_p()
        t0 = time.perf_counter()
        if which == "A":
            capi.check(lib.cvx_submit(al.h, n, tab.ctypes.data_as(C.POINTER(capi.CvxTile)), C.byref(j)))
        else:
            capi.check(lib.cvx_submit_segments(al.h, None, n, tab_seg.ctypes.data_as(C.POINTER(capi.CvxTile)), None, n_reads, arena.ctypes.data,
                                               offsets.ctypes.data, seg.ctypes.data, C.byref(j)))
        t1 = time.perf_counter()
        res, ops, n_ops = C.POINTER(capi.CvxResult)(), C.POINTER(C.c_uint32)(), C.c_uint64()
        capi.check(lib.cvx_wait(al.h, j, C.byref(res), C.byref(ops), C.byref(n_ops)))
        t2 = time.perf_counter()
        out = (bytes(C.string_at(res, n * C.sizeof(capi.CvxResult))), bytes(C.string_at(ops, int(n_ops.value) * 4)))
        lib.cvx_job_release(al.h, j)
        return (t1 - t0) * 1e3, (t2 - t0) * 1e3, out

    run("A"), run("B")      # warm-up: arenas grow to their size
    sub, tot, outs = {"A": [], "B": []}, {"A": [], "B": []}, {}
    for _ in range(a.reps):
        for w in ("A", "B"):
            s, t, outs[w] = run(w)
            sub[w].append(s)
            tot[w].append(t)
    assert outs["A"] == outs["B"], "cvx_submit_segments does not compute what cvx_submit computes"
    # the kernel alone
    lens = ts.H.astype(np.int32)
    qo, used = np.zeros(n, dtype=np.uint64), C.c_uint64()
    out = np.zeros(int(lens.sum()) + 64, dtype=np.uint8)
    kms = []
    for _ in range(a.reps + 1):
        capi.check(lib.cvx_stage_segments(al.h, n_reads, arena.ctypes.data, offsets.ctypes.data, n, seg.ctypes.data, lens.ctypes.data,
                                          out.ctypes.data, len(out), qo.ctypes.data, C.byref(used)))
        kms.append(al.stage_kernel_ms(capi.STAGE_SEGMENTS))
    qbytes = int(ts.H.sum())
    k = float(np.median(kms[1:]))
    print(json.dumps({
        "tiles": n, "read_len": a.read_len, "reads": n_reads, "reverse_tiles": int(seg["flags"].sum()), "reps": a.reps,
        "submit_ms": {w: [round(x, 2) for x in sub[w]] for w in sub}, "submit_ms_median": {w: round(float(np.median(sub[w])), 2) for w in sub},
        "submit_to_results_ms_median": {w: round(float(np.median(tot[w])), 2) for w in tot},
        "query_bytes_over_pcie": {"A": qbytes, "B": int(offsets[-1]) + 16 * n},
        "stage_segments_kernel_ms": [round(x, 4) for x in kms[1:]], "stage_segments_kernel_GBps_read_plus_written": round(2 * qbytes / (k * 1e-3) / 1e9, 1),
        "identical_results": True}))
    al.close()


if __name__ == "__main__":
    main()
