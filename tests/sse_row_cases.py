"""Deterministic tile families for the catch-all fill's SSE-path rules (fill_generic_kernel<SSE = true>, cvx_generic.hip; the
reference's fwdFillMatrixSSESimple, src/ConvexAlignFast.cpp:914-1287) at short and ragged rows.

What a cell of a row is computed by depends on the row's clipped length L = min(off + len, W) - max(off, 0):

    cells [0, sse_n)        the 4-wide loop's relaxed rules (chain A), sse_n = 4 * ceil((L - 4) / 4), none for L <= 4
    cells [L - 12, L)       recomputed by the scalar rules (chain B), all of them for L <= 12
    rows below              see B wherever it exists
    the running maximum     sees A first, then B

so L <= 4, 5 <= L <= 12, 13 <= L <= 16 and L mod 4 beyond are different code, and so is the cell above an A-only cell, a recomputed
one or the empty element.  Every family below is named by its row lengths and by the column at which the alignment's path runs
inside a row.

A plain module (no fixtures, no device): tests/test_sse_fill_pin_cpu.py pins the port's restatement to the reference cell by cell on
these tiles and asserts that the families do what they are for; tests/test_gpu_sse_rows.py sends them through the device.

A tile is written from an alignment script: matching blocks over ACG, 1 - 3 mismatches (A against C), insertions of 1 - 3 (T, in the
read only), deletions of 1 - 2 ('N', in the window only) where the row has room right of the path.  Row y of the corridor has L(y)
cells and starts so that the script's path lies at column p(y) of it.  A flank of 'N' -- a base no read carries -- on both ends of
the window keeps every row inside it (off >= 0, off + len <= W) wherever clipping is not the subject.  150 - 250 read rows, windows of
at most about 400 columns.
"""
from collections import namedtuple

import numpy as np

from ngmlr_amd import synth

KEYS = ("match", "mismatch", "gap_open", "gap_extend", "gap_extend_min", "gap_decay")
DEFAULT = dict(match=2.0, mismatch=-5.0, gap_open=-5.0, gap_extend=-5.0, gap_extend_min=-1.0, gap_decay=0.15)
# gap_open + gap_extend_min >= mismatch - 0.25: the SSE path and the scalar recurrence disagree (the entries of
# tests/test_gpu_parity.py::EXOTIC_SCORING, restated so that this module imports no test)
EXOTIC = [
    dict(match=2.0, mismatch=-10.0, gap_open=-5.0, gap_extend=-5.0, gap_extend_min=-1.0, gap_decay=0.15),
    dict(match=2.0, mismatch=-6.0, gap_open=-5.0, gap_extend=-5.0, gap_extend_min=-1.0, gap_decay=0.15),
    dict(match=2.0, mismatch=-7.0, gap_open=-4.0, gap_extend=-3.0, gap_extend_min=-2.0, gap_decay=0.5),
    dict(match=1.0, mismatch=-4.0, gap_open=-1.0, gap_extend=-1.0, gap_extend_min=-0.5, gap_decay=0.05),
    dict(match=3.0, mismatch=-20.0, gap_open=-2.0, gap_extend=-6.0, gap_extend_min=-1.0, gap_decay=0.3),
]
# scorings without the ring kernels' sign structure, or tie-heavy: every one outside fill_semantics' fast regime
SIGN_FREE = [
    dict(match=2.0, mismatch=0.0, gap_open=-5.0, gap_extend=-5.0, gap_extend_min=-1.0, gap_decay=0.15),      # mismatch 0
    dict(match=2.0, mismatch=-5.0, gap_open=0.0, gap_extend=-5.0, gap_extend_min=-1.0, gap_decay=0.15),      # gap_open 0
    dict(match=2.0, mismatch=-5.0, gap_open=-5.0, gap_extend=-0.5, gap_extend_min=-1.0, gap_decay=0.15),     # extension above its floor
    dict(match=1.0, mismatch=-1.0, gap_open=-0.5, gap_extend=-0.5, gap_extend_min=-0.5, gap_decay=0.0),      # no decay, open == floor
]
NON_DEFAULT = EXOTIC + SIGN_FREE
SEPARATING = EXOTIC[0]      # (2, -10, -5, -5, -1, 0.15): SURVEY.md Appendix A


def params(sc):
    return tuple(sc[k] for k in KEYS)


Case = namedtuple("Case", "tile family kind L col")      # L / col: None where they vary row to row

FLANK = ord("N")


def band(L):
    """(first, last) column of a row of L cells that validPath accepts (src/AlignmentMatrixFast.cpp:213-220, for a row inside the
    window); first > last: none.  Only used to choose columns: what is valid is asserted on the oracle."""
    lo = int(np.float32(0.1) * np.float32(L))
    hi = int(np.float32(lo + L) - np.float32(0.1) * np.float32(L))
    return lo + 1, hi - 1


def is_regular(tile):
    """The rule by which the plan sends a corridor to a ring kernel (cvx_plan_logic.h: row spans on the anti-diagonals that start
    strictly later and end no earlier row after row), restated.  Only ever used to assert that a tile lands where it was aimed."""
    off = np.asarray(tile.row_offset, dtype=np.int64)
    ln = np.asarray(tile.row_length, dtype=np.int64)
    y = np.arange(len(off), dtype=np.int64)
    lo = np.maximum(off, 0)
    hi = np.maximum(np.minimum(off + ln, tile.W), lo)
    gs, ge = y + lo, y + hi
    return bool(np.all(np.diff(gs) > 0) and np.all(np.diff(ge) >= 0))


def clipped_lengths(tile):
    off = np.asarray(tile.row_offset, dtype=np.int64)
    ln = np.asarray(tile.row_length, dtype=np.int64)
    lo = np.maximum(off, 0)
    return np.maximum(np.minimum(off + ln, tile.W), lo) - lo


def _script(rng, dmax):
    """[(op, n)]: '=' blocks of 8 - 29 with one event between two of them, 150 - 250 read rows, a matching block at both ends"""
    H = int(rng.integers(150, 251))
    ops, rows = [], 0
    while True:
        n = int(rng.integers(8, 30))
        if H - (rows + n) < 12:
            n = H - rows
        ops.append(("=", n))
        rows += n
        if rows >= H:
            return ops
        ev = int(rng.integers(0, 3 if dmax > 0 else 2))
        if ev == 0:
            n = int(rng.integers(1, 4))
            ops.append(("X", n))
            rows += n
        elif ev == 1:
            n = int(rng.integers(1, 4))
            ops.append(("I", n))
            rows += n
        else:
            ops.append(("D", int(rng.integers(1, dmax + 1))))


def _realize(rng, ops):
    """-> (window core, read, path): path[y] the window column of read row y's cell on the script's path (an inserted row stays
    in the column of the last base consumed)"""
    ref, qry, path = [], [], []
    x = 0
    for op, n in ops:
        if op == "=":
            r = rng.choice(np.frombuffer(b"ACG", dtype=np.uint8), size=n)
            ref.append(r); qry.append(r); path.extend(range(x, x + n)); x += n
        elif op == "X":
            ref.append(np.full(n, ord("A"), np.uint8)); qry.append(np.full(n, ord("C"), np.uint8))
            path.extend(range(x, x + n)); x += n
        elif op == "I":
            qry.append(np.full(n, ord("T"), np.uint8)); path.extend([max(x - 1, 0)] * n)
        else:
            ref.append(np.full(n, FLANK, np.uint8)); x += n
    return np.concatenate(ref), np.concatenate(qry), np.asarray(path, dtype=np.int64)


def _tile(rng, Lf, pf, tag, follow=True, flank_l=None, flank_r=None, fix=None):
    """Lf(y), pf(y): the row's length and the column wanted for the path.  follow: the column gives way where the row start
    would otherwise move back (p(y) <= p(y - 1) + the path's step), so row starts never decrease.  fix(off, ln, W, path): last
    word on the rows (the clipped family)."""
    ys = np.arange(260)
    Ls = np.array([Lf(int(y)) for y in ys])
    ps = np.array([pf(int(y)) for y in ys])
    room = int(np.min(np.array([band(int(L))[1] for L in Ls]) - ps))
    ops = _script(rng, max(0, min(2, room)))
    core, qry, path = _realize(rng, ops)
    H = len(qry)
    assert 150 <= H <= 250, (tag, H)
    p = ps[:H].copy()
    if follow:
        for y in range(1, H):
            p[y] = min(p[y], p[y - 1] + (path[y] - path[y - 1]))
    fl = int(ps.max()) + 1 if flank_l is None else flank_l
    fr = int(Ls.max()) + 1 if flank_r is None else flank_r
    ref = np.concatenate([np.full(fl, FLANK, np.uint8), core, np.full(fr, FLANK, np.uint8)])
    W = len(ref)
    off = (fl + path - p).astype(np.int64)
    ln = Ls[:H].astype(np.int64)
    if fix is not None:
        off, ln = fix(off, ln, W, fl + path)
    assert W <= 420, (tag, W)
    return synth.Tile(ref=ref.tobytes(), qry=qry.tobytes(), row_offset=off.astype(np.int32), row_length=ln.astype(np.int32), tag=tag)


LEFT_L = (14, 15, 16, 17, 18, 19, 20, 21, 24, 25, 28, 32, 33, 40)
CLIP_UP = (0, 1, 4, 5, 12, 13, 16)      # clipped lengths over consecutive rows at the head of a tile; reversed at its tail


def left_col(L):
    """A column only the 4-wide loop writes (below L - 12), inside the validPath band and with a valid column left of it where the
    row has one.  L = 14 has no such column (the band starts at 2 = L - 12): its path runs in column 1, outside the band."""
    return min(band(L)[0] + 1, L - 13)


def _const(v):
    return lambda y: v


def _cycle(vals, base=0):
    return lambda y: base + vals[y % len(vals)]


def _clip_fix(edge, where, Ln):
    def fix(off, ln, W, xpath):
        H = len(off)
        n = len(CLIP_UP)
        if (edge, where) == ("left", "head"):
            for y in range(n):
                off[y] = CLIP_UP[y] - Ln
            for y in range(n, H):
                off[y] = max(off[y], off[y - 1])
        elif (edge, where) == ("right", "tail"):
            for k in range(n):
                off[H - n + k] = W - CLIP_UP[n - 1 - k]
        elif (edge, where) == ("left", "tail"):
            for k in range(n):
                off[H - n + k] = CLIP_UP[n - 1 - k] - Ln
        else:
            for y in range(n):
                off[y] = W - CLIP_UP[y]
        return off, ln
    return fix


def families(seed=2031, reps=4):
    """-> [Case].  `reps` tiles (scripts) per kind."""
    out = []

    def add(family, kind, L, col, make):
        for r in range(reps):
            rng = np.random.default_rng([seed, len(out)])
            out.append(Case(make(rng, "%s %s #%d" % (family, kind, r)), family, kind, L, col))

    # short: no 4-wide iteration (L <= 4); both chains over the whole row (5 <= L <= 12).  Path at the centre.
    for L in range(1, 13):
        add("short", "L%d" % L, L, L // 2, lambda rng, tag, L=L: _tile(rng, _const(L), _const(L // 2), tag))
    # left: the path in cells only the 4-wide loop writes
    for L in LEFT_L:
        c = left_col(L)
        add("left", "L%d" % L, L, c, lambda rng, tag, L=L, c=c: _tile(rng, _const(L), _const(c), tag))
    add("left", "L16-23", None, 3, lambda rng, tag: _tile(rng, _cycle(range(16, 24)), _const(3), tag))
    # seam: the last A-only cell and the first recomputed one
    for L in (24, 25):
        for c in (L - 13, L - 12):
            add("seam", "L%d c%d" % (L, c), L, c, lambda rng, tag, L=L, c=c: _tile(rng, _const(L), _const(c), tag))
    # overlap: inside the 8 - 11 cells both chains write, one kind per L mod 4
    for L in (32, 33, 34, 35):
        add("overlap", "L%d" % L, L, L - 10, lambda rng, tag, L=L: _tile(rng, _const(L), _const(L - 10), tag))
    # ragged: the cell above belongs to the other class
    for cyc in ((3, 4, 5, 8, 12, 13, 16, 17), (9, 10, 11, 12, 13)):
        add("ragged", "L" + "-".join(map(str, cyc)), None, None,
            lambda rng, tag, cyc=cyc: _tile(rng, _cycle(cyc), _cycle([L // 2 for L in cyc]), tag))
    # steps: the row start moving by 0 (also under an insertion), +1 and +2 ...
    for name, p0 in (("left", 4), ("seam", 11)):
        add("steps", "%s L24 +0+1+2" % name, 24, None,
            lambda rng, tag, p0=p0: _tile(rng, _const(24), _cycle((0, 1, 2, 1, 0, 0), p0), tag))
    # ... and, for the irregular form (a slot per row, nothing re-bound), back by 1 ... 3 with a jitter of +-1
    for name, p0 in (("left", 4), ("seam", 11)):
        def make(rng, tag, p0=p0):
            jit = rng.integers(-1, 2, size=260)
            saw = (0, 2, 5, 9)
            return _tile(rng, _const(24), lambda y: int(min(max(p0 + saw[y % 4] + jit[y], 1), 22)), tag, follow=False)
        add("steps", "%s L24 -1-2-3" % name, 24, None, make)
    # clipped: rows cut by the window's edges down to 16, 13, 12, 5, 4, 1 and 0 cells over consecutive rows
    for edge, where in (("left", "head"), ("right", "tail"), ("left", "tail"), ("right", "head")):
        add("clipped", "%s %s" % (edge, where), None, 8,
            lambda rng, tag, edge=edge, where=where: _tile(rng, _const(24), _const(8), tag,
                                                           flank_l=0 if (edge, where) == ("left", "head") else None,
                                                           flank_r=2 if (edge, where) == ("right", "tail") else None,
                                                           fix=_clip_fix(edge, where, 24)))
    return out


def irregular_by_design(case):
    """the kinds written to leave the ring kernels: row starts that move back"""
    return (case.family == "steps" and case.kind.endswith("-1-2-3")) or (case.family == "clipped" and case.kind in ("left tail", "right head"))
