#!/usr/bin/env python3
"""What taking CIGAR and MD from the device is worth inside the pipeline: oracle/_ref/ngmlr_hip_regions with CVX_JOB_TEXT=1 against
=0 (the same binary with every alignment formatted on the host), alternating on one box, `--runs` runs each, on N synthetic
PacBio-like 10 kb reads (tools/e2e_rates.py's workload and settings).  Per run: wall, mapping time, the process's CPU-seconds,
the alignment contexts' CPU-seconds (AlignPool's exit line) and the job text line; with --pcsample a CVX_PC_SAMPLE report of one
further run per side (where cvx_format_alignment_ex, cvx_text_reclip and the copies went).

    python tools/job_text_bound.py 20000 80000 --runs 3 --pcsample >> profiles/r21_job_text.txt
"""
import argparse
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("reads", type=int, nargs="+")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--pcsample", action="store_true")
    ap.add_argument("--top", type=int, default=25)
    args = ap.parse_args()
    import e2e_rates
    name = "ngmlr_hip_regions"
    if not os.path.exists(os.path.join(ROOT, "oracle", "_ref", name)):
        print("oracle/_ref/%s not built (tools/build_ngmlr_hip.sh)" % name)
        return 1
    t, ctx, target, hold = 20, 4096, 2048, 10000      # e2e_rates.pipeline_summary's settings
    base_env = {"CVX_POOL_CONTEXTS": str(ctx), "CVX_BATCH_TARGET": str(target), "CVX_BATCH_HOLD_US": str(hold), "CVX_CS_BATCH": "20"}
    for n_reads in args.reads:
        fa, fq = os.path.join(e2e_rates.tmp, "jt_ref_%d.fa" % n_reads), os.path.join(e2e_rates.tmp, "jt_reads_%d.fq" % n_reads)
        bases = e2e_rates.write_plain_workload(fa, fq, n_reads, np.random.default_rng(2025), 2000000)
        print("# %d reads, %d bases; -t %d, %d contexts, batch target %d / %d us" % (n_reads, bases, t, ctx, target, hold))
        sys.stdout.flush()
        rows = {"1": [], "0": []}
        sam = {}
        for run in range(args.runs):
            for switch in ("1", "0") if run % 2 == 0 else ("0", "1"):
                r = e2e_rates.run(name, t, fa, fq, dict(base_env, CVX_JOB_TEXT=switch))
                pool = e2e_rates._pool_numbers(r.get("pool_stats")) or {}
                line = re.search(r"SharedAligner: \d+ alignments took their CIGAR and MD[^\n]*", r["full_err"])
                ctx_cpu = pool.get("read_code_cpu_s")
                rows[switch].append((r["wall"], r["map_s"], r["cpu_total_s"], ctx_cpu))
                sam.setdefault(switch, sorted(r["recs"]))
                assert sorted(r["recs"]) == sam[switch]
                print("run %d  CVX_JOB_TEXT=%s  rc %d  wall %7.2f s  map %7.2f s  process CPU %7.2f s  contexts' CPU %s s  %d SAM records  %s" % (
                    run, switch, r["rc"], r["wall"], r["map_s"] or -1.0, r["cpu_total_s"], "%.2f" % ctx_cpu if ctx_cpu is not None else "n/a", len(r["recs"]),
                    line.group(0) if line else ""))
                sys.stdout.flush()
        print("SAM records identical between the two sides: %s" % (sam["1"] == sam["0"]))
        for k, label in enumerate(("wall", "map", "process CPU", "contexts' CPU")):
            a = [x[k] for x in rows["1"] if x[k] is not None]
            b = [x[k] for x in rows["0"] if x[k] is not None]
            if a and b:
                print("%-14s device text %7.2f s (min %.2f max %.2f)   host text %7.2f s (min %.2f max %.2f)   device - host %+.2f s, spread of the repeats %.2f / %.2f s" % (
                    label, np.median(a), min(a), max(a), np.median(b), min(b), max(b), np.median(a) - np.median(b), max(a) - min(a), max(b) - min(b)))
        if args.pcsample:
            for switch in ("1", "0"):
                path = os.path.join(e2e_rates.tmp, "pcs_jt_%s_%d.bin" % (switch, n_reads))
                e2e_rates.run(name, t, fa, fq, dict(base_env, CVX_JOB_TEXT=switch, CVX_PC_SAMPLE=path))
                print("## CVX_PC_SAMPLE, CVX_JOB_TEXT=%s, %d reads" % (switch, n_reads))
                rep = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "pcsample_report.py"), path, str(args.top)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
                print(rep.stdout)
                sys.stdout.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
