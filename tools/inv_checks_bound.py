#!/usr/bin/env python3
"""What taking checkForSV's two scores from the job's inversion checks is worth inside the pipeline: oracle/_ref/ngmlr_hip_invchecks
with the binding on against CVX_DEVICE_INV_CHECKS=0 in the same binary (which equals ngmlr_hip_regions), alternating on one box,
`--runs` runs a side, on N synthetic PacBio-like 10 kb reads and on the split-read (SV) workload of tools/e2e_rates.py.  Per run:
wall, mapping time, the process's CPU-seconds, the alignment contexts' CPU-seconds (AlignPool's exit line) and the binding's exit
line.  The project's standing rule: the variant may become a default only if the contexts' CPU-seconds fall by more than the
spread of the repeats.

    python tools/inv_checks_bound.py --plain 20000 --sv 3000 --runs 3 >> profiles/r31_inv_checks_bound.txt
"""
import argparse
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

LINE = re.compile(r"DeviceInvChecks: (\d+) checks taken from the job \((\d+) scored, (\d+) without a read part\), (\d+) through checkForSV's own scoring "
                  r"\((\d+) no window, (\d+) inconsistent record, (\d+) note without checks\), (\d+) verified, (\d+) disagreements")


def side_by_side(e2e_rates, name, label, fa, fq, runs):
    t, ctx, target, hold = 20, 4096, 2048, 10000      # e2e_rates.pipeline_summary's settings
    base_env = {"CVX_POOL_CONTEXTS": str(ctx), "CVX_BATCH_TARGET": str(target), "CVX_BATCH_HOLD_US": str(hold), "CVX_CS_BATCH": "20"}
    print("# %s; %s -x %s -t %d, %d contexts, batch target %d / %d us" % (label, name, e2e_rates.PRESET, t, ctx, target, hold))
    sys.stdout.flush()
    rows = {"1": [], "0": []}
    sam = {}
    for run in range(runs):
        for switch in ("1", "0") if run % 2 == 0 else ("0", "1"):
            r = e2e_rates.run(name, t, fa, fq, dict(base_env, CVX_DEVICE_INV_CHECKS=switch))
            pool = e2e_rates._pool_numbers(r.get("pool_stats")) or {}
            m = LINE.search(r["full_err"])
            ctx_cpu = pool.get("read_code_cpu_s")
            rows[switch].append((r["wall"], r["map_s"], r["cpu_total_s"], ctx_cpu))
            sam.setdefault(switch, sorted(r["recs"]))
            assert sorted(r["recs"]) == sam[switch]
            print("run %d  CVX_DEVICE_INV_CHECKS=%s  rc %d  wall %7.2f s  map %7.2f s  process CPU %7.2f s  contexts' CPU %s s  %d SAM records  %s" % (
                run, switch, r["rc"], r["wall"], r["map_s"] or -1.0, r["cpu_total_s"], "%.2f" % ctx_cpu if ctx_cpu is not None else "n/a", len(r["recs"]),
                m.group(0) if m else "no DeviceInvChecks line"))
            sys.stdout.flush()
    print("SAM records identical between the two sides: %s" % (sam["1"] == sam["0"]))
    for k, what in enumerate(("wall", "map", "process CPU", "contexts' CPU")):
        a = [x[k] for x in rows["1"] if x[k] is not None]
        b = [x[k] for x in rows["0"] if x[k] is not None]
        if a and b:
            print("%-14s checks from the job %7.2f s (min %.2f max %.2f)   checkForSV's own scoring %7.2f s (min %.2f max %.2f)   difference %+.2f s, spread of the repeats %.2f / %.2f s" % (
                what, np.median(a), min(a), max(a), np.median(b), min(b), max(b), np.median(a) - np.median(b), max(a) - min(a), max(b) - min(b)))
    sys.stdout.flush()


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--plain", type=int, default=20000, help="synthetic 10 kb reads (0: skip)")
    ap.add_argument("--sv", type=int, default=3000, help="reads of the split-read workload (0: skip)")
    ap.add_argument("--runs", type=int, default=3)
    args = ap.parse_args()
    import e2e_rates
    name = "ngmlr_hip_invchecks"
    if not os.path.exists(os.path.join(ROOT, "oracle", "_ref", name)):
        print("oracle/_ref/%s not built (tools/build_ngmlr_hip.sh)" % name)
        return 1
    if args.plain > 0:
        fa, fq = os.path.join(e2e_rates.tmp, "icb_ref_%d.fa" % args.plain), os.path.join(e2e_rates.tmp, "icb_reads_%d.fq" % args.plain)
        bases = e2e_rates.write_plain_workload(fa, fq, args.plain, np.random.default_rng(2025), 2000000)
        side_by_side(e2e_rates, name, "%d synthetic reads, %d bases" % (args.plain, bases), fa, fq, args.runs)
    if args.sv > 0:
        fa, fq = os.path.join(e2e_rates.tmp, "icb_sv_ref_%d.fa" % args.sv), os.path.join(e2e_rates.tmp, "icb_sv_reads_%d.fq" % args.sv)
        e2e_rates.write_sv_workload(fa, fq, args.sv)
        e2e_rates.PRESET = "ont"
        side_by_side(e2e_rates, name, "%d reads of the split-read workload" % args.sv, fa, fq, args.runs)
    return 0


if __name__ == "__main__":
    sys.exit(main())
