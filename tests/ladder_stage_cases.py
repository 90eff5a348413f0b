"""The engineered tiles of a ladder job whose rungs run the regions, checks and text stages (cvx_submit_ladder_ex,
tests/test_gpu_ladder_stages.py): tests/ladder_cases.py's set, plus deletion tiles that climb AND carry what those stages look
for -- planted substitution bursts (24-base runs, as tests/test_gpu_job_regions.py's burst_tile plants them) and
tests/nm_region_cases.py's inverted stretch.

A plain module (no fixtures, no device).  tests/test_ladder_stage_cases_cpu.py checks on the CPU -- the port oracle, the host
text stage inside it and cvx_nm_regions_host -- that the set holds what the GPU tests rely on; without that they could pass
on tiles that never climb or never have a region."""
import numpy as np

from ngmlr_amd import synth
from tests import ladder_cases as lc

BURST_RUN, BURST_PERIOD = 24, 110


def _substitute(seq, a, n):
    seq[a:a + n] = synth._ACGT[(synth._CODE[seq[a:a + n]].astype(np.int64) + 1) % 4]


def staged_tile(genome, at, flank, d, bursts=True, inv=0, run=BURST_RUN, period=BURST_PERIOD):
    """-> (ref bytes, qry bytes, (first, last) read base of the planted inversion or None): `flank` matched bases, a deletion
    of d, `flank` matched bases, read against the window it spans (the endpoints corridor runs corner to corner, the path
    bulges d / 2 columns off it).  bursts: every `period`-th base of both flanks starts `run` substituted bases (one region
    each).  inv: that many bases in the middle of the right flank are the reverse complement of the window's."""
    ref = genome[at:at + 2 * flank + d]
    left, right = ref[:flank].copy(), ref[flank + d:].copy()
    planted = None
    if inv:
        a = (flank - inv) // 2
        right[a:a + inv] = synth.revcomp(right[a:a + inv])
        planted = (flank + a, flank + a + inv - 1)
    if bursts:
        for part in (left, right):
            for a in range(60, flank - 60 - run, period):
                if inv and part is right and a + run > (flank - inv) // 2 - 40 and a < (flank + inv) // 2 + 40:
                    continue                              # (the inverted stretch and its surroundings stay as they are)
                _substitute(part, a, run)
    return ref.tobytes(), np.concatenate([left, right]).tobytes(), planted


def staged(seed=2026):
    """-> list of (tag, ref, qry, ladder, planted): the tiles this module adds.  Reads of 1 200 to 2 000 bases."""
    rng = np.random.default_rng(seed)
    genome = synth.random_ref(rng, 6000)
    out = []
    # the endpoints ladder at corridor 256: rung m is 64 m columns wide around the corner-to-corner line
    for k, d in enumerate((0, 40, 70, 80, 90, 100, 110, 130, 150, 170, 190, 220)):
        out.append(("bursts-d%d" % d, *staged_tile(genome, 50 + 37 * k, 600, d)[:2], (256, 0.0, 0.0, 0), None))
    # the anchors ladder: rungs 1 and 2 in the anchors form, the endpoints form from rung 3 on
    for k, d in enumerate((60, 120, 200)):
        out.append(("bursts-anchors-d%d" % d, *staged_tile(genome, 900 + 41 * k, 600, d)[:2], (256, 40.0, 40.0, lc.ANCHORS), None))
    # REALIGN keeps the whole corridor
    out.append(("bursts-realign-d150", *staged_tile(genome, 1500, 600, 150)[:2], (100, 0.0, 0.0, lc.REALIGN), None))
    # planted inversions: on tiles that climb, and on one that does not
    for k, d in enumerate((0, 100, 160)):
        ref, qry, planted = staged_tile(genome, 2000 + 53 * k, 1000, d, bursts=(k == 2), inv=200)
        out.append(("inv200-d%d" % d, ref, qry, (256, 0.0, 0.0, 0), planted))
    return out


def engineered():
    """-> list of (tag, ref, qry, ladder, planted): tests/ladder_cases.py's engineered tiles (planted None), then staged()"""
    return [(tag, ref, qry, ladder, None) for tag, ref, qry, ladder in lc.engineered()] + staged()


def grow_tiles(seed=2027, n=6, flank=1490, d=100):
    """n climbing tiles of 2 * flank read bases with a 20-base burst every 60 bases (the 40 matches behind a burst still close
    its region and keep the alignment on the diagonal): some 45 regions each.  A rung of n tiles asks for an arena of
    8 n + 64 regions and gets 9 n + 136 (the growth rule of the runtime's buffers, cvx_buf.h): six such tiles outgrow it."""
    rng = np.random.default_rng(seed)
    genome = synth.random_ref(rng, 2 * flank + d + 64 * n)
    return [("grow%d" % i, *staged_tile(genome, 32 * i, flank, d, run=20, period=60)[:2], (256, 0.0, 0.0, 0), None) for i in range(n)]


def straddle(n=300, seed=2028, every=4):
    """n short tiles (reads of 600 bases) of which every `every`-th climbs: the climbing tiles lie on both sides of entry 256
    of ladder_next_kernel's scan, and each carries a few bursts so that its checks exist"""
    rng = np.random.default_rng(seed)
    genome = synth.random_ref(rng, 4000)
    out = []
    for i in range(n):
        d = (90, 130)[(i // every) % 2] if i % every == 1 else int(rng.integers(0, 30))
        at = int(rng.integers(0, 4000 - 600 - d))
        ref, qry, _ = staged_tile(genome, at, 300, d)
        out.append(("straddle%d" % i, ref, qry, (256, 0.0, 0.0, 0), None))
    return out


def expectation(cases, valid, align=None):
    """per case: the rung the rule reports over `valid` (lc.climb), the rungs' row-array tiles, whether the last one has
    cells, and (align given: an oracle's align) the last tile's alignment"""
    out = []
    for tag, ref, qry, ladder, planted in cases:
        n, tiles = lc.climb(ref, qry, ladder, valid)
        live = lc.has_cells(tiles[-1])
        out.append(dict(tag=tag, ref=ref, qry=qry, ladder=ladder, planted=planted, rung=n, tiles=tiles, live=live,
                        port=align(tiles[-1]) if (align is not None and live) else None))
    return out
