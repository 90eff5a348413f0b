#!/usr/bin/env python
"""The measurement behind kJobTextBytesPerRow (ngmlr_amd/csrc/cvx_job_text_logic.h): bytes of text (CIGAR + NUL + MD + NUL) per read
row, as the host text stage writes them with both external clips zero, over the synthetic PacBio and ONT workloads -- the ops
come from the port oracle, as in tests/test_host_format_cpu.py.  No device.

    python tools/job_text_bytes_per_row.py [--pacbio 48] [--ont 400]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measure(tiles, orc, lib):
    from ngmlr_amd import capi
    from ngmlr_amd.aligner import format_alignment
    worst, total_bytes, total_rows, valid = 0.0, 0, 0, 0
    for t in tiles:
        t.ext_qstart = t.ext_qend = 0
        w = orc.align(t)
        total_rows += t.H
        if w["ret"] < 0:
            total_bytes += 2
            continue
        f, ops = orc.last_fwd(), orc.last_ops()
        r = capi.CvxResult()
        r.score, r.status = w["score"], 0
        r.ref_position, r.qstart, r.qend = f["ref_position"], f["qstart"], f["qend"]
        r.n_ops, r.ops_begin = len(ops), 0
        d = format_alignment(lib, r, ops if len(ops) else np.zeros(1, np.uint32), t, want_nm=False)
        b = d["cigar_len"] + d["md_len"] + 2
        worst = max(worst, b / t.H)
        total_bytes += b
        valid += 1
    return worst, total_bytes / max(total_rows, 1), valid


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pacbio", type=int, default=48)
    ap.add_argument("--ont", type=int, default=400)
    a = ap.parse_args()
    from ngmlr_amd import capi, synth
    from oracle.pyoracle import Oracle
    orc, lib = Oracle("port"), capi.load()
    worst = 0.0
    for name, tiles in (("pacbio", synth.workload_pacbio(a.pacbio)), ("ont", synth.workload_ont(a.ont))):
        w, mean, valid = measure(tiles, orc, lib)
        worst = max(worst, w)
        print("%-7s %4d tiles (%d valid): largest (cigar_len + md_len + 2) / H of a tile %.3f, of the whole set %.3f" % (name, len(tiles), valid, w, mean))
    print("largest %.3f, with a quarter on top %.3f" % (worst, worst * 1.25))


if __name__ == "__main__":
    main()
