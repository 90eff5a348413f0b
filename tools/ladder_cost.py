"""tools/ladder_cost.py [--tiles 512] [--passes 3] [--flagged] [--lib PATH] [--out FILE] -- what the corridor retry ladder costs inside one device job
(cvx_submit_ladder) against what a caller does today: submit, wait, rebuild the failed tiles' corridors on the host, submit again.

One job of ONT-like tiles (reads of 1-6 kb, 10 % errors, endpoints corridors), about 10 % of which carry a deletion the first rung
cannot hold and about 1 % one that the second cannot hold either.  Both forms run in alternating passes on one device after a
warm-up pass of each; per pass: wall time from the first submit to the last result, the bytes that cross PCIe (computed from the
record sizes and the sequence lengths, not measured), and cvx_timing per rung.  Prints a table; --out writes it to a file too.

--flagged: the same on a handle with CVX_CREATE_NM_REGIONS | _INV_CHECKS | _JOB_TEXT and a resident genome that holds the tiles'
windows (cvx_submit_ladder_ex against cvx_submit_windows / wait / rebuild / submit again): every job's regions, checks and text
are taken inside the timed span, as a caller would take them.  --lib: another build of the library (a parent commit's, say)."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ngmlr_amd import capi, synth  # noqa: E402
from ngmlr_amd.aligner import ConvexAlignHip  # noqa: E402

TILE_IN, ROW_SRC, PLAN, RESULT, LADDER = 32, 32, 32, 48, 16      # bytes per tile of the records that travel


def make_tiles(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        W0 = int(rng.integers(1000, 6000))
        d = 0
        if i % 10 == 3:
            d = 420
        if i % 100 == 7:
            d = 700
        ref = synth.random_ref(rng, W0 + d)
        cut = W0 // 2
        qry = synth.mutate(rng, np.concatenate([ref[:cut], ref[cut + d:]]), 0.10)
        out.append((ref.tobytes(), qry.tobytes(), (1024, 0.0, 0.0, 0)))
    return out


def form_tile(ref, qry, ladder, m):
    desc = capi.ladder_rung(len(ref), len(qry), ladder, m)
    return None if desc is None else synth.Tile(ref, qry, np.zeros(0, np.int32), np.zeros(0, np.int32), desc=desc)


def timing_row(t):
    return "plan %.3f fill %.3f walk %.3f total %.3f ms, %d launches" % (t.plan_ms, t.fill_ms, t.backtrack_ms, t.total_ms, t.n_fill_launches)


def take_stages(job):
    """what a caller of a flagged handle reads from a finished job -> (regions, text bytes)"""
    off, _reg, _opn = job.regions()
    job.checks()
    _recs, toff, _raw = job.texts_raw()
    return int(off[-1]), int(toff[-1])


def run_ladder(al, cases, flagged=None):
    tiles = [synth.Tile(r, q, np.zeros(0, np.int32), np.zeros(0, np.int32), desc=(2, 0.0, 0.0, 0.0, 0, 0)) for r, q, _ in cases]
    stages = None
    t0 = time.perf_counter()
    if flagged:
        job = al.submit_ladder_ex(tiles, [l for _, _, l in cases], genome=flagged[0], ref_positions=flagged[1])
    else:
        job = al.submit_ladder(tiles, [l for _, _, l in cases])
    res, ops = job.wait()
    if flagged:
        stages = take_stages(job)
    wall = time.perf_counter() - t0
    info = job.ladder_info()
    lad = job.ladder()
    up = sum(len(r) + len(q) for r, q, _ in cases) + len(cases) * (TILE_IN + ROW_SRC + LADDER)
    down = len(cases) * (PLAN + RESULT) + 4 * len(ops)
    # behind every rung but the fifth, the next rung's list, tile records, corridors and plan come back for every slot of that rung
    # (an upper bound: a job whose tiles have no further rung skips the step behind its last one)
    for r in range(min(info["rungs_run"], 4)):
        down += (info["tiles"][r] + 1) * 4 + info["tiles"][r] * (TILE_IN + ROW_SRC + PLAN)
    down += sum(info["tiles"][1:]) * RESULT
    out = dict(wall_ms=wall * 1e3, up=up, down=down, rungs=info["tiles"], timing=timing_row(job.timing()), valid=int((res["status"] == 0).sum()),
               seq_after=info["seq_bytes_after_submit"], reported=[int((lad["rung"] == r).sum()) for r in range(1, 6)], stages=stages)
    if flagged:
        out["rewrites"] = (job.regions_info()["rewrites"], job.texts_info()["rewrites"])
    job.release()
    return out


def submit_forms(al, tiles, genome=None, positions=None):
    arr, keep = al._pack(tiles, closed_form=True)
    j = C.c_void_p()
    if genome is None:
        capi.check(al.lib.cvx_submit(al.h, len(tiles), arr, C.byref(j)))
    else:
        pos = np.ascontiguousarray(positions, dtype=np.uint64)
        keep = (keep, pos)
        capi.check(al.lib.cvx_submit_windows(al.h, genome.g, len(tiles), arr, pos.ctypes.data, C.byref(j)))
    from ngmlr_amd.aligner import Job
    return Job(al, j, len(tiles), (arr, keep))


def run_today(al, cases, flagged=None):
    """submit, wait, rebuild the failed tiles' forms on the host, submit again"""
    live = list(range(len(cases)))
    up = down = 0
    regions = text = 0
    rungs, timings = [], []
    valid = 0
    t0 = time.perf_counter()
    for m in range(1, 6):
        tiles, who = [], []
        for i in live:
            t = form_tile(*cases[i], m)
            if t is not None:
                tiles.append(t)
                who.append(i)
        if not tiles:
            break
        job = submit_forms(al, tiles, flagged[0], [flagged[1][i] for i in who]) if flagged else submit_forms(al, tiles)
        res, ops = job.wait()
        if flagged:
            # (what a failed attempt left is read with the rest, as a caller that takes a job's stages reads all of them)
            r_, t_ = take_stages(job)
            regions, text = regions + r_, text + t_
        up += sum(len(t.ref) + len(t.qry) for t in tiles) + len(tiles) * (TILE_IN + ROW_SRC)
        down += len(tiles) * (PLAN + RESULT) + 4 * len(ops)
        rungs.append(len(tiles))
        timings.append(timing_row(job.timing()))
        valid += int((res["status"] == 0).sum())
        live = [i for i, s in zip(who, res["status"]) if s != 0]
        job.release()
        if not live:
            break
    wall = time.perf_counter() - t0
    return dict(wall_ms=wall * 1e3, up=up, down=down, rungs=rungs + [0] * (5 - len(rungs)), timing=" | ".join(timings), valid=valid,
                stages=(regions, text) if flagged else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=512)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--seed", type=int, default=25)
    ap.add_argument("--out", default=None)
    ap.add_argument("--flagged", action="store_true")
    ap.add_argument("--lib", default=None)
    args = ap.parse_args()
    cases = make_tiles(args.tiles, args.seed)
    flagged = None
    if args.flagged:
        from ngmlr_amd.aligner import Genome, encode_genome
        al = ConvexAlignHip(device=0, lib_path=args.lib, nm_regions=True, inv_checks=True, job_text=True)
        genome = encode_genome(al.lib, [b"".join(r for r, _, _ in cases)])
        at = np.concatenate([[0], np.cumsum([len(r) for r, _, _ in cases])])[:-1]
        flagged = (Genome(al, *genome), [int(genome[2][0]) + int(a) for a in at])
    else:
        al = ConvexAlignHip(device=0, lib_path=args.lib)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    lib = al.lib
    lib.cvx_build_id.restype = C.c_char_p
    say("tools/ladder_cost.py --tiles %d --passes %d --seed %d%s   (build %s%s)" % (args.tiles, args.passes, args.seed, " --flagged" if args.flagged else "",
                                                                                 lib.cvx_build_id().decode(), ", " + args.lib if args.lib else ""))
    say("%d tiles, %d read bases, %d reference bases" % (len(cases), sum(len(q) for _, q, _ in cases), sum(len(r) for r, _, _ in cases)))
    run_ladder(al, cases, flagged)      # warm-up: arenas, kernels loaded
    run_today(al, cases, flagged)
    rows = {"ladder": [], "today": []}
    for p in range(args.passes):
        for name, fn in (("ladder", run_ladder), ("today", run_today)):
            r = fn(al, cases, flagged)
            rows[name].append(r)
            say("pass %d %-6s wall %8.3f ms  up %9d B  down %8d B  tiles per rung %s  valid %d" % (p, name, r["wall_ms"], r["up"], r["down"], r["rungs"], r["valid"]))
            say("        %s" % r["timing"])
            if r["stages"]:
                say("        regions %d, text %d B%s" % (r["stages"][0], r["stages"][1], "  rewrites (regions, text) %s" % (r["rewrites"],) if "rewrites" in r else ""))
    for name in ("ladder", "today"):
        w = sorted(r["wall_ms"] for r in rows[name])
        say("%-6s wall ms: min %.3f median %.3f max %.3f over %d passes" % (name, w[0], w[len(w) // 2], w[-1], len(w)))
    say("ladder: tiles reported at rung 1..5: %s; sequence bytes moved after the submit call: %d" % (rows["ladder"][-1]["reported"], rows["ladder"][-1]["seq_after"]))
    assert rows["ladder"][-1]["valid"] == rows["today"][-1]["valid"], "the two forms disagree on how many tiles resolve"
    if flagged:
        flagged[0].free()
    al.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
