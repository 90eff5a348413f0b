#!/usr/bin/env python3
"""What handing computeAlignment's retry loop over as one request is worth inside the pipeline: oracle/_ref/ngmlr_hip_ladder with
the binding on against CVX_DEVICE_LADDER=0 in the same binary (which equals ngmlr_hip_regions), alternating on one box, `--runs`
runs a side, on N synthetic PacBio-like 10 kb reads (tools/e2e_rates.py's workload).  Per run: wall, mapping time, the process's
CPU-seconds, the alignment contexts' CPU-seconds (AlignPool's exit line), the dispatcher thread's CPU-seconds (while a ladder
launch is in flight it polls instead of sleeping in Wait) and the device's ladder exit line.  With --pcsample a CVX_PC_SAMPLE
report of one further run per side, the functions the ladder form is meant to remove called out; with --trace one further run
per side under CVX_LAUNCH_TRACE=1 and the medians of its launches: what a ladder launch costs beside a plain one (a launch in
which nobody climbs still pays one ladder_next_kernel, one plan of an empty list and a read-back).

    python tools/ladder_bound.py 20000 80000 --runs 3 --pcsample --trace >> profiles/r30_ladder_binding.txt
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

LADDER = re.compile(r"SharedAligner: device \d+: (\d+) ladder requests, (\d+) with attempts >= 2, (\d+) reported a failed last rung, (\d+) ladder launches")
TRACE = re.compile(r"cvx dispatcher: submit ([0-9.]+) ms, wait entered ([0-9.]+) ms after the cut, blocked in it ([0-9.]+) ms; cvx launch: (\d+) tiles, ([0-9.]+) M cells, "
                   r"oldest request waited ([0-9.]+) ms, in flight ([0-9.]+) ms: plan ([0-9.]+) fill ([0-9.]+) walk ([0-9.]+) device total ([0-9.]+) ms")
CALLED_OUT = ("getCorridorEndpointsWithAnchors", "cvx_corridor_fit", "quotientsAndBoundsAvx2", "verifyRightAvx2", "__default_morecore", "PrepareLadder", "FinishLadder", "dispatchLoop", "cvx_job_poll")


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("reads", type=int, nargs="+")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--pcsample", action="store_true")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--top", type=int, default=25)
    args = ap.parse_args()
    import e2e_rates
    name = "ngmlr_hip_ladder"
    if not os.path.exists(os.path.join(ROOT, "oracle", "_ref", name)):
        print("oracle/_ref/%s not built (tools/build_ngmlr_hip.sh)" % name)
        return 1
    t, ctx, target, hold = 20, 4096, 2048, 10000      # e2e_rates.pipeline_summary's settings
    base_env = {"CVX_POOL_CONTEXTS": str(ctx), "CVX_BATCH_TARGET": str(target), "CVX_BATCH_HOLD_US": str(hold), "CVX_CS_BATCH": "20"}
    sides = (("1", "ladder"), ("0", "loop"))
    for n_reads in args.reads:
        fa, fq = os.path.join(e2e_rates.tmp, "lb_ref_%d.fa" % n_reads), os.path.join(e2e_rates.tmp, "lb_reads_%d.fq" % n_reads)
        bases = e2e_rates.write_plain_workload(fa, fq, n_reads, np.random.default_rng(2025), 2000000)
        print("# %d reads, %d bases; %s -t %d, %d contexts, batch target %d / %d us" % (n_reads, bases, name, t, ctx, target, hold))
        sys.stdout.flush()
        rows = {"1": [], "0": []}
        sam = {}
        for run in range(args.runs):
            for switch in ("1", "0") if run % 2 == 0 else ("0", "1"):
                r = e2e_rates.run(name, t, fa, fq, dict(base_env, CVX_DEVICE_LADDER=switch))
                pool = e2e_rates._pool_numbers(r.get("pool_stats")) or {}
                lines = LADDER.findall(r["full_err"])
                counts = tuple(sum(int(l[k]) for l in lines) for k in range(4)) if lines else None
                ctx_cpu = pool.get("read_code_cpu_s")
                disp_cpu = (r.get("cpu_by_class") or {}).get("cvx-dispatch")
                rows[switch].append((r["wall"], r["map_s"], r["cpu_total_s"], ctx_cpu, disp_cpu))
                sam.setdefault(switch, sorted(r["recs"]))
                assert sorted(r["recs"]) == sam[switch]
                launch = r.get("launch")
                print("run %d  CVX_DEVICE_LADDER=%s  rc %d  wall %7.2f s  map %7.2f s  process CPU %7.2f s  contexts' CPU %s s  dispatcher CPU %s s  %d SAM records  %s  %s" % (
                    run, switch, r["rc"], r["wall"], r["map_s"] or -1.0, r["cpu_total_s"], "%.2f" % ctx_cpu if ctx_cpu is not None else "n/a",
                    "%.2f" % disp_cpu if disp_cpu is not None else "n/a", len(r["recs"]),
                    ("%d requests in %d launches" % (launch[0], launch[1])) if launch else "",
                    ("ladder requests %d, attempts >= 2: %d, failed last rung: %d, ladder launches %d" % counts) if counts else "no ladder line"))
                sys.stdout.flush()
        print("SAM records identical between the two sides: %s" % (sam["1"] == sam["0"]))
        for k, label in enumerate(("wall", "map", "process CPU", "contexts' CPU", "dispatcher CPU")):
            a = [x[k] for x in rows["1"] if x[k] is not None]
            b = [x[k] for x in rows["0"] if x[k] is not None]
            if a and b:
                print("%-14s ladder %7.2f s (min %.2f max %.2f)   loop %7.2f s (min %.2f max %.2f)   ladder - loop %+.2f s, spread of the repeats %.2f / %.2f s" % (
                    label, np.median(a), min(a), max(a), np.median(b), min(b), max(b), np.median(a) - np.median(b), max(a) - min(a), max(b) - min(b)))
        if args.trace:
            for switch, label in sides:
                r = e2e_rates.run(name, t, fa, fq, dict(base_env, CVX_DEVICE_LADDER=switch, CVX_LAUNCH_TRACE="1"))
                rec = np.array([[float(x) for x in m] for m in TRACE.findall(r["full_err"])])
                lines = LADDER.findall(r["full_err"])
                climbed = sum(int(l[1]) for l in lines) if lines else 0
                if len(rec) == 0:
                    print("## CVX_LAUNCH_TRACE, %s: no launch lines" % label)
                    continue
                over = rec[:, 10] - rec[:, 8] - rec[:, 9]      # device total - fill - walk: plan, the ladder's decision step, everything that is not a fill or a walk
                print("## CVX_LAUNCH_TRACE, %s (CVX_DEVICE_LADDER=%s), %d reads: %d launches, %d requests with attempts >= 2 among them; medians per launch: %d tiles, "
                      "submit %.2f ms, blocked in Wait %.2f ms, in flight %.2f ms, plan %.2f ms, fill %.2f ms, walk %.2f ms, device total %.2f ms, device total - fill - walk %.2f ms "
                      "(mean %.2f ms); in flight per tile %.1f us" % (label, switch, n_reads, len(rec), climbed, int(np.median(rec[:, 3])), np.median(rec[:, 0]), np.median(rec[:, 2]),
                                                                    np.median(rec[:, 6]), np.median(rec[:, 7]), np.median(rec[:, 8]), np.median(rec[:, 9]), np.median(rec[:, 10]),
                                                                    np.median(over), np.mean(over), 1e3 * rec[:, 6].sum() / max(rec[:, 3].sum(), 1.0)))
                sys.stdout.flush()
        if args.pcsample:
            for switch, label in sides:
                path = os.path.join(e2e_rates.tmp, "pcs_lb_%s_%d.bin" % (switch, n_reads))
                e2e_rates.run(name, t, fa, fq, dict(base_env, CVX_DEVICE_LADDER=switch, CVX_PC_SAMPLE=path))
                print("## CVX_PC_SAMPLE, %s (CVX_DEVICE_LADDER=%s), %d reads" % (label, switch, n_reads))
                rep = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "pcsample_report.py"), path, "400"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
                out = rep.stdout.splitlines()
                print("\n".join(out[:args.top + 4]))
                print("   called out (anywhere in the report; absent = no sample):")
                for l in out:
                    if any(f in l for f in CALLED_OUT):
                        print("   " + l)
                sys.stdout.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
