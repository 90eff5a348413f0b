"""tools/inv_checks_cost.py [--tiles 2048] [--runs 3] -- what CVX_CREATE_INV_CHECKS costs a job, and what the same checks cost
as parked scoring round trips (profiles/r23_inv_checks.txt).

PacBio-like tiles (synth.pacbio_tileset) go through cvx_submit_windows on a CVX_CREATE_NM_REGIONS handle and on a
CVX_CREATE_NM_REGIONS | CVX_CREATE_INV_CHECKS handle, alternating, `runs` times a side after one warm-up each: the compute stage's
device time (cvx_timing.total_ms: plan + fills + walk + finalize + compaction + finder, and the checks where they run) and the
wall time from submit to the end of wait.  A second handle without the flag, created last, runs in the same rotation: it tells a
difference that comes with the flag from one that comes with a handle's place in the process.  Then cvx_inv_checks' kernel_ms
for the same regions, the bytes the records add to the download, and the same pairs -- (window, read part) and (window, reverse
complement) of every scored region, strings built on the host -- through cvx_score_submit / cvx_score_wait in calls of two pairs, one after the other: a parked check today."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=2048)
    ap.add_argument("--runs", type=int, default=3)
    args = ap.parse_args()
    from ngmlr_amd import aligner, synth
    from ngmlr_amd.aligner import ConvexAlignHip, Genome, StrippedSWHip

    ts = synth.pacbio_tileset(args.tiles, seed=7)
    rng = np.random.default_rng(8)
    lead = 1500
    contig = np.concatenate([synth.random_ref(rng, lead), ts.ref, synth.random_ref(rng, lead)]).tobytes()
    base, checks = ConvexAlignHip(device=0, nm_regions=True), ConvexAlignHip(device=0, nm_regions=True, inv_checks=True)
    base2 = ConvexAlignHip(device=0, nm_regions=True)
    genome = aligner.encode_genome(base.lib, [contig])
    positions = (int(genome[2][0]) + lead + ts.ref_off[:-1]).astype(np.uint64)
    gb, gc, gb2 = Genome(base, *genome), Genome(checks, *genome), Genome(base2, *genome)

    def run(g, keep=False):
        t0 = time.perf_counter()
        job = g.submit(ts, positions)
        res, _ops = job.wait()
        wall = (time.perf_counter() - t0) * 1e3
        out = (job.timing().total_ms, wall, job.regions_info()["total"])
        kept = (res.copy(),) + job.regions()[:2] + (job.checks(),) if keep else None
        job.release()
        return out, kept

    run(gb)
    run(gc)
    run(gb2)
    rows = {"regions": [], "regions+checks": [], "regions (2nd)": []}
    kept = None
    for _ in range(args.runs):
        rows["regions"].append(run(gb)[0])
        r, kept = run(gc, keep=True)
        rows["regions+checks"].append(r)
        rows["regions (2nd)"].append(run(gb2)[0])
    print("%d PacBio-like tiles (%.1f Mbp of reads), %d regions per job, cvx_submit_windows, %d alternating runs a side" %
          (ts.n, ts.H.sum() / 1e6, rows["regions"][0][2], args.runs))
    for name, rr in rows.items():
        dev, wall = np.array([x[0] for x in rr]), np.array([x[1] for x in rr])
        print("  %-15s compute stage %s ms (median %.3f, spread %.3f)   submit..wait %s ms (median %.2f)" %
              (name, " ".join("%.3f" % x for x in dev), np.median(dev), dev.max() - dev.min(), " ".join("%.2f" % x for x in wall), np.median(wall)))
    med = {k: float(np.median([x[0] for x in v])) for k, v in rows.items()}
    print("  compute stage, medians: with the flag %+.3f ms against the first handle without it, %+.3f ms against the second" %
          (med["regions+checks"] - med["regions"], med["regions+checks"] - med["regions (2nd)"]))

    res, off, reg, chk = kept
    qrys = [ts.qry[int(ts.qry_off[i]):int(ts.qry_off[i + 1])].tobytes() for i in range(ts.n)]
    ms = [base.inv_checks(gb, qrys, positions, res["ref_position"], off, reg)[1] for _ in range(args.runs + 1)][1:]
    print("cvx_inv_checks over the same %d regions: kernel_ms %s" % (len(reg), " ".join("%.3f" % x for x in ms)))
    print("download: %d bytes of check records per job (16 per region) beside %d bytes of regions" % (16 * len(reg), 16 * len(reg)))
    st, n_st = np.unique(chk["status"], return_counts=True)
    print("outcomes: %s" % ", ".join("%s %d" % ({0: "scored", 1: "too short", 2: "no read part", 3: "no window"}[int(s)], int(n)) for s, n in zip(st, n_st)))

    # the same checks as parked round trips: two pairs a call, each call submitted and waited for before the next
    tile_of = np.searchsorted(off[1:], np.arange(len(reg)), side="right")
    scored = np.flatnonzero(chk["status"] == 0)
    pairs, parts = [], []
    for r in scored:
        t = int(tile_of[r])
        rs, re_, qs, qe = (int(x) for x in reg[r])
        inv, mid = abs(re_ - rs), (qs + qe) // 2
        pairs.append((int(positions[t]) + int(res["ref_position"][t]) + (rs + re_) // 2 - 250 - inv // 2, inv + 500, 0, 0))
        parts.append(qrys[t][mid - 50:mid + 50])
    windows, _q, _s = aligner.stage_windows_host(base.lib, genome[0], genome[1], genome[2], [b"A"], pairs)
    cpl = bytes.maketrans(b"ACGT", b"TGCA")
    sw = StrippedSWHip(device=0)
    for k in range(min(64, len(scored))):      # warm-up
        sw.submit_scores([windows[k]] * 2, [parts[k], parts[k].translate(cpl)[::-1]]).wait()
    t0 = time.perf_counter()
    same = 0
    for k in range(len(scored)):
        sc = sw.submit_scores([windows[k]] * 2, [parts[k], parts[k].translate(cpl)[::-1]]).wait()
        same += int(sc[0] == chk["score_fwd"][scored[k]] and sc[1] == chk["score_rev"][scored[k]])
    dt = (time.perf_counter() - t0) * 1e3
    print("cvx_score_submit / cvx_score_wait, %d calls of two pairs one after the other: %.1f ms in all, %.4f ms a call (%d of %d calls give the job's two scores)" %
          (len(scored), dt, dt / max(len(scored), 1), same, len(scored)))
    sw.close()
    gb.free()
    gc.free()
    gb2.free()
    base2.close()
    base.close()
    checks.close()


if __name__ == "__main__":
    main()
