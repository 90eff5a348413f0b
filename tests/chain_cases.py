"""Script-written tiles for the chained row-block fill (kFillChain of fill_ring_kernel / fill_ring_twin_kernel, cvx_fill_ring.inc;
planned by plan_chain_tile, cvx_host_logic.h; merged by chain_reduce_kernel) at the edges of its own geometry.

A corridor with more live rows than the widest ring allowed is cut into row blocks of N = 64, 128 or 256 read rows.  Block g
takes the `up` inputs of its first row from 8-byte boundary records (score, run, insertion bit) that block g - 1 writes as its
last row advances, 16 steps (a chunk) at a time; it begins on a multiple of 32 steps behind the tile's first step r0, at least
one step before its first cell, and has its own region of direction words.  The best cell is merged over the blocks with the
reference's tie-break (first strict maximum in (y, x) order).

The tiles are written as tests/walk_cases.py writes them (its `tile`, `op_list` and scorings, sse_row_cases' `_realize`): rows of
one length L = 200 -- about 100 live rows, so a handle whose whole-tile rings are capped at 64 slots chains them -- and events
placed relative to the block height N.  The step of row y's first cell behind r0 is (off[y] + y) - off[0].

    cross   =(N - k) I n =70      an insertion of n rows, k of them above the boundary row N: the record carries the run and the
                                  insertion bit, and the penalty moves until run 27 under the default scoring
    brow    =lead D d =100        lead = N, N + 1: deletion cells in the last row of a block and in the first row of the next
    phase   =56 D d =100          row N's first cell 2 N + d steps behind r0: every residue of a 32-step word and a 16-record
                                  chunk; path at column 100 (valid) and at columns 0 and 1 (the row's first cells: rejected)
    rows    =H                    a last block of 1, N - 1 and N rows, the best cell in the tile's last row
    ties    X ... =30 ... X       equal maxima in two or more blocks
    clip    =(N - 4) D3 =70 I4 =(N + 56)   the window cut from the left or the right around row N - 1 and the last block

A plain module (no fixtures, no device).  tests/test_chain_cases_cpu.py asserts under the port oracle that the families do what
they are for; tests/test_gpu_chain_edges.py sends them through every chained form of the device fill."""
from collections import namedtuple

import numpy as np

from ngmlr_amd import synth
from tests import walk_cases as wc

DEFAULT = wc.DEFAULT
ONT = dict(match=1.0, mismatch=-1.0, gap_open=-1.0, gap_extend=-1.0, gap_extend_min=-0.5, gap_decay=0.15)      # ngmlr -x ont
params = wc.params
op_list = wc.op_list

HEIGHTS = (64, 128, 256)
L0 = 200
FAMILIES = ("cross", "brow", "phase", "rows", "ties", "clip")

# ops: the expected (len << 4) | op list, None where the oracle alone says what the alignment is (clip);  info: the quantities
# the family is named after, N among them
Case = namedtuple("Case", "tile family kind script ops scoring info")


def gap_cost(sc, n):
    """an upper bound of what a gap of n costs: the opening and n extensions min(gap_extend_min, gap_extend + run * decay)"""
    return -sc["gap_open"] - sum(min(sc["gap_extend_min"], sc["gap_extend"] + r * sc["gap_decay"]) for r in range(n))


def first_steps(t):
    """the step of every row's first cell (clipped to the window) behind the first step of row 0, and the clipped spans"""
    off = np.asarray(t.row_offset, dtype=np.int64)
    ln = np.asarray(t.row_length, dtype=np.int64)
    lo = np.maximum(off, 0)
    hi = np.maximum(np.minimum(off + ln, t.W), lo)
    y = np.arange(len(off))
    return lo + y, lo, hi


def _case(out, N, family, kind, script, L, p, scoring=DEFAULT, ops="script", **info):
    rng = np.random.default_rng([2828, N, len(out)])
    tag = "%s N%d %s%s" % (family, N, kind, " ont" if scoring is ONT else "")
    t, path, _, _ = wc.tile(rng, script, L, p, tag)
    info.update(N=N, L=L, col=p)
    out.append(Case(t, family, kind, list(script), op_list(script) if ops == "script" else ops, scoring, info))
    return t, path


CROSS_N = (1, 2, 3, 26, 27, 28, 40, 57, 90)
CROSS_TAIL = 70


def cross_ks(N, n, sc):
    """the rows k of an insertion of n above the boundary row N: 0 (opened from a boundary record), 1, 2, n / 2, 26, 27 (the run
    at which the default penalty stops moving), n - 1 and n (the run ends on the block's last row) -- where they exist, and where
    the leading block of N - k matches and the tail pay for the gap (else the local alignment starts behind it or ends before)"""
    cost = gap_cost(sc, n) + 2 * sc["match"]
    ks = sorted({k for k in (0, 1, 2, n // 2, 26, 27, n - 1, n) if 0 <= k <= n and k < N})
    return [k for k in ks if min(N - k, CROSS_TAIL) * sc["match"] > cost]


def cross_cases(out, N):
    for sc in (DEFAULT, ONT):
        for n in CROSS_N:
            L = max(L0, 4 * n + 60)
            for k in cross_ks(N, n, sc):
                _case(out, N, "cross", "I%d k%d" % (n, k), [("=", N - k), ("I", n), ("=", CROSS_TAIL)], L, L // 2, sc, n=n, k=k)


BROW_D = tuple(range(1, 34))


def brow_cases(out, N):
    for lead in (N, N + 1):
        for d in BROW_D:
            _case(out, N, "brow", "lead%d D%d" % (lead, d), [("=", lead), ("D", d), ("=", 100)], L0, 100, d=d, row=lead - 1)


PHASE_LEAD = 56      # (a deletion of 32 costs about 92: the 80 of 40 matches would not pay for it, and the alignment would start behind it)
PHASE_COLS = (100, 0, 1)
PHASE_L = ((207, "partial"), (208, "full"), (209, "one"))      # records of row N - 1: 12 chunks and 15, 13 chunks, 13 and 1


def phase_cases(out, N):
    def add(d, L, col, kind):
        script = [("=", PHASE_LEAD)] + ([("D", d)] if d else []) + [("=", max(100, N + 20))]      # (row N exists at every N)
        t, _ = _case(out, N, "phase", kind, script, L, col, d=d, residue=(2 * N + d) % 32, chunk=(2 * N + d) % 16, valid=col == 100)
        assert int(first_steps(t)[0][N] - first_steps(t)[0][0]) == 2 * N + d
    for d in range(33):
        for col in PHASE_COLS:
            add(d, L0, col, "d%d c%d" % (d, col))
    for L, _ in PHASE_L:
        for d in (0, 1, 15):
            for col in (100, 0):
                add(d, L, col, "L%d d%d c%d" % (L, d, col))


def rows_heights(N):
    return (N + 1, 2 * N - 1, 2 * N, 2 * N + 1, 3 * N, 3 * N + 1)


def rows_cases(out, N):
    for H in rows_heights(N):
        _case(out, N, "rows", "H%d" % H, [("=", H)], L0, 100, H=H, last=(H - 1) % N + 1)


def _ties_script(H, segs):
    """X everywhere, = over [first, first + n) for every (first, n) of segs"""
    script, y = [], 0
    for first, n in segs:
        script += [("X", first - y), ("=", n)]
        y = first + n
    return script + [("X", H - y)]


TIES_H = 4400
# (blocks, lengths) of the many-block tiles and the best row each must report: blocks 1 and 65 share lane 1 of the reduction
# (g += 64), 3 and 66 meet in the cross-lane merge with the later block in the lower lane, 2 / 64 / 67 both
TIES_MANY = ((((1, 30), (65, 30)), 103), (((3, 30), (66, 30)), 231), (((3, 30), (66, 31)), 4264), (((2, 30), (64, 30), (67, 30)), 167))


def ties_cases(out, N):
    # two blocks: the first segment in block 0, the second from row 6 of block 1 on
    for a, b, row in ((30, 30, 29), (30, 31, N + 6 + 30), (31, 30, 30)):
        script = [("=", a), ("X", N - 24 - (a - 30)), ("=", b), ("X", 4)]
        win = max(a, b)
        _case(out, N, "ties", "=%d =%d" % (a, b), script, L0, 100, ops=op_list([("=", win)]), best_row=row, blocks=(0, 1))
    if N != 64:
        return
    for segs, row in TIES_MANY:
        spans = [(g * N + 10, n) for g, n in segs]
        win = max(n for _, n in segs)
        _case(out, N, "ties", "blocks " + " ".join("%d:%d" % s for s in segs), _ties_script(TIES_H, spans), L0, 100,
              ops=op_list([("=", win)]), best_row=row, blocks=tuple(g for g, _ in segs))


CLIP_CUTS = ("row N-1 40 left", "row N-1 at 0", "row N at 0", "block 0 empty", "block 0 one cell", "rows N-1 on past W", "last block empty")


def clip_script(N):
    return [("=", N - 4), ("D", 3), ("=", 70), ("I", 4), ("=", N + 56)]


def clip_cases(out, N):
    """one script, the window cut from the left (the first c columns dropped, every row start moved by -c) or from the right
    (cut to W columns): row starts keep their order, rows lose cells"""
    script = clip_script(N)
    rng = np.random.default_rng([2828, N, 77])
    base, _, _, _ = wc.tile(rng, script, L0, 100, "clip")
    off = base.row_offset.astype(np.int64)
    ref = np.frombuffer(base.ref, dtype=np.uint8)
    H = base.H
    last0 = (H - 1) // N * N
    cuts = {"row N-1 40 left": ("left", off[N - 1] + 40), "row N-1 at 0": ("left", off[N - 1]), "row N at 0": ("left", off[N]),
            "block 0 empty": ("left", off[N - 1] + L0), "block 0 one cell": ("left", off[N - 1] + L0 - 1),
            "rows N-1 on past W": ("right", off[N - 1] + L0 - 1), "last block empty": ("right", off[last0])}
    for kind in CLIP_CUTS:
        side, c = cuts[kind]
        c = int(c)
        if side == "left":
            t = synth.Tile(ref=ref[c:].tobytes(), qry=base.qry, row_offset=(off - c).astype(np.int32), row_length=base.row_length.copy(),
                           tag="clip N%d %s" % (N, kind))
        else:
            t = synth.Tile(ref=ref[:c].tobytes(), qry=base.qry, row_offset=base.row_offset.copy(), row_length=base.row_length.copy(),
                           tag="clip N%d %s" % (N, kind))
        out.append(Case(t, "clip", kind, list(script), None, DEFAULT, dict(N=N, L=L0, col=100, side=side, cut=c)))


def families(N):
    """-> [Case] for the block height N"""
    assert N in HEIGHTS
    out = []
    cross_cases(out, N)
    brow_cases(out, N)
    phase_cases(out, N)
    rows_cases(out, N)
    ties_cases(out, N)
    clip_cases(out, N)
    return out
