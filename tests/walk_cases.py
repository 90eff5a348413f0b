"""Script-written tiles for the backtrack walk (backtrack_walk and backtrack_walk_grp<G>, cvx_kernels.hip; the reference's
revBacktrack + validPath, src/ConvexAlignFast.cpp:335-432, src/AlignmentMatrixFast.cpp:213-220) at the edges of its own geometry.

The walk runs backwards from the best cell.  G lanes probe the next G cells along the current direction, a ballot finds how far the
run goes, and the gap that ends a diagonal run is followed inside the direction words the probe already holds: a deletion run in
lane L's 32-step word, an insertion run in the words of the lanes behind L.  After every gap the probe starts again.  A diagonal run
of R cells between two gaps (or between the best cell and a gap) is therefore covered in R // G full probes and its gap lies at lane
R % G of the next one: R = 63 / 64 / 65 (127 / 128 / 129) puts it at lane G - 1 / 0 / 1 for every G in 4, 8, 16, 32, 64 at once.

A tile is written from an alignment script [(op, n)] with sse_row_cases' alphabet: matching blocks over ACG, mismatches A against
C, inserted bases T (never in the window, so an insertion's placement is unique), deleted window bases N, a flank of N one row
length wide on both sides of the window.  All rows have the same length L; row y starts so that the script's path lies at column
p (one value, or one per row) of it, and row starts never decrease (np.maximum.accumulate), so the corridor is regular and goes to
a ring kernel.  The cells of a deletion lie in the row of the last base before it, right of that row's path cell; the cells of an
insertion lie in the inserted rows, in the column of the last base before it.

The step index of cell (x, y) is x + y - r0 with r0 row 0's start: path_x - path_x[0] + y + p for a path cell.  A direction word
holds 32 steps of one row, so p over 32 consecutive values moves an event through every phase of a word.

A plain module (no fixtures, no device).  tests/test_walk_cases_cpu.py asserts under the port oracle that every script is the
alignment its tile has and that the families do what they are for; tests/test_gpu_walk_forms.py sends them through every
lanes-per-tile form of the device walk.
"""
from collections import namedtuple

import numpy as np

from ngmlr_amd import synth
from tests import sse_row_cases as rc

DEFAULT = rc.DEFAULT
# mismatch -1: two mismatches cost less than they gain, so an alignment may alternate X and = cell by cell
MILD = dict(match=2.0, mismatch=-1.0, gap_open=-5.0, gap_extend=-5.0, gap_extend_min=-1.0, gap_decay=0.15)
params = rc.params

OP_CODE = {"=": 7, "X": 8, "I": 1, "D": 2}
GROUPS = (4, 8, 16, 32)      # lanes per tile of backtrack_walk_grp; 64: backtrack_walk

# family: lane / word / subrun / band / ring;  scoring: DEFAULT or MILD;  ops: the expected (len << 4) | op list;  info: the
# quantities the family is named after
Case = namedtuple("Case", "tile family kind script ops scoring info")


def op_list(script):
    """the walk's run-length ops of a script: adjacent equal ops merged, first op first"""
    out = []
    for op, n in script:
        if n <= 0:
            continue
        if out and out[-1][0] == op:
            out[-1][1] += n
        else:
            out.append([op, n])
    return [(n << 4) | OP_CODE[op] for op, n in out]


def gap_events(script):
    """-> [(op, n, R)] in walk order (last event first): R the diagonal cells (= and X) the walk covers between the previous gap,
    or the best cell, and this one.  The gap lies at lane R % G of a probe."""
    out, run = [], 0
    for op, n in reversed(script):
        if op in "=X":
            run += n
        else:
            out.append((op, n, run))
            run = 0
    return out


def tile(rng, script, L, p, tag):
    """-> (Tile, path, p per row, flank): path[y] the column, in the window's core, of row y's path cell"""
    core, qry, path = rc._realize(rng, script)
    H = len(qry)
    p = np.broadcast_to(np.asarray(p, dtype=np.int64), (H,)).copy()
    fl = L + 1
    ref = np.concatenate([np.full(fl, rc.FLANK, np.uint8), core, np.full(fl, rc.FLANK, np.uint8)])
    want = fl + path - p
    off = np.maximum.accumulate(want)
    assert np.array_equal(off, want), (tag, "the wanted columns would move a row start back")
    t = synth.Tile(ref=ref.tobytes(), qry=qry.tobytes(), row_offset=off.astype(np.int32), row_length=np.full(H, L, np.int32), tag=tag)
    return t, path, p, fl


def _first_gap(script, path, p):
    """(row, step) of the first gap cell the walk meets: the last event of the script.  Steps count from row 0's start."""
    y = 0
    ev = None
    for op, n in script:
        if op == "D":
            ev = (op, n, y - 1)               # the deleted cells lie in the row of the last base before them
        elif op == "I":
            ev = (op, n, y + n - 1)           # the last inserted row is met first
        if op != "D":
            y += n
    op, n, row = ev
    x = path[row] + (n if op == "D" else 0)
    return row, int(x - path[0] + row + p[0])


def _case(out, family, kind, script, L, p, scoring=DEFAULT, **info):
    rng = np.random.default_rng([2424, len(out)])
    tag = "%s %s" % (family, kind)
    t, path, pr, fl = tile(rng, script, L, p, tag)
    if any(op in "ID" for op, _ in script):
        info["row"], info["step"] = _first_gap(script, path, pr)
    info.update(L=L, events=gap_events(script))
    out.append(Case(t, family, kind, list(script), op_list(script), scoring, info))


LANE_R = (63, 64, 65, 127, 128, 129)
LANE_EVENTS = ([("I", n) for n in (1, 2, 3, 4, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 70)]
               + [("D", n) for n in (1, 2, 31, 32, 33, 40)] + [("X", 1), ("X", 3)])


def row_len(n):
    return max(120, 4 * n + 60)


def lane_cases(out):
    """=70, ev, =R, ev, =R: both events at lane R % G.  For an insertion of n the probe has G - R % G lanes left: n below, at
    and above that is a run that ends inside the probe, on its last lane (the hand-over to a plain gap probe) and beyond it."""
    for R in LANE_R:
        for op, n in LANE_EVENTS:
            L = row_len(n)
            _case(out, "lane", "R%d %s%d" % (R, op, n), [("=", 70), (op, n), ("=", R), (op, n), ("=", R)], L, L // 2, R=R, ev=(op, n))


WORD_EVENTS = (("I", 3), ("I", 40), ("D", 1), ("D", 5), ("D", 33), ("D", 40))


WORD_EDGE_D = (2, 3, 4, 8, 12, 16, 24, 31, 32)


def have_break(step, n):
    """An insertion run of n met at step `step` behind a diagonal run: its cell k is step - k of row y - k, and the lane that
    holds that row has loaded the word of step - 2 k.  -> the first k < n at which the two are different words (the run is then
    cut there and a plain gap probe takes over), or None."""
    for k in range(1, n):
        if (step - k) >> 5 != (step - 2 * k) >> 5:
            return k
    return None


def word_cases(out):
    """=80, ev, =70 at 32 consecutive p: the event at every phase of a direction word.  in_word: the cells of the deletion's row
    that the word of its first cell holds, that cell included -- a run shorter than, exactly as long as and longer than that ends
    inside the word, at its edge (the walk must look into the previous word) and beyond it."""
    for op, n in WORD_EVENTS:
        L = row_len(n)
        for k in range(32):
            p = L // 2 - 16 + k
            _case(out, "word", "%s%d p%d" % (op, n, p), [("=", 80), (op, n), ("=", 70)], L, p, ev=(op, n), col=p, sweep=True)
            c = out[-1]
            step = c.info["step"]
            if op == "D":
                c.info["in_word"] = (step & 31) + 1
            else:
                c.info["have_break"] = have_break(step, n)
    # a deletion that ends exactly at the edge of its word: the sweeps hold two (D 1 and D 5, one phase each); eight more runs at
    # the one p of the sweep that puts their first cell in_word = n cells above the edge
    for n in WORD_EDGE_D:
        for k in range(32):
            p = 44 + k
            if ((n + 158 + p) & 31) + 1 == n:      # the first cell's step: n + 79 (columns) + 79 (rows) + p
                _case(out, "word", "D%d edge p%d" % (n, p), [("=", 80), ("D", n), ("=", 70)], 120, p, ev=("D", n), col=p)
                out[-1].info["in_word"] = (out[-1].info["step"] & 31) + 1


# (a deletion of 3 costs 14.55: the block in front of it must be worth more)
WORD_EARLY = [(lead + (n == 3), n, R) for lead in (7, 8, 9) for n in (1, 2, 3) for R in (144, 150)]


def word_early_cases(out):
    """A deletion of n <= 3 behind a leading block of 7 - 9 matches only: the score left of it is so small that the cells a few
    columns right of the run, in its own row, are zero and carry STOP.  At the phases where the run reaches the edge of its word
    (in_word <= n) the direction that follows it is in the PREVIOUS word; a walk that looks for it at the other end of the same
    word finds one of those cells.  (Deeper in an alignment every cell near the path carries a direction that sends the walk
    back onto it, and the next probe repairs a wrong guess.)"""
    for lead, n, R in WORD_EARLY:
        for k in range(32):
            p = 44 + k
            if ((n + 2 * (lead - 1) + p) & 31) + 1 <= n:
                _case(out, "word", "early =%d D%d R%d p%d" % (lead, n, R, p), [("=", lead), ("D", n), ("=", R)], 120, p, ev=("D", n), col=p)
                out[-1].info["in_word"] = (out[-1].info["step"] & 31) + 1
                assert out[-1].info["in_word"] <= n


def _repeat(unit, times):
    return [u for _ in range(times) for u in unit]


def subrun_cases(out):
    """EQ / X sub-runs of one diagonal run: the grouped walk finds their starts with a mask and writes them lane-parallel, the
    last one of a probe stays pending and is merged into the first one of the next probe when the op is the same.  The probes
    count from the best cell, so the block walked first (the script's last) shifts every boundary."""
    for t in range(40, 48):
        _case(out, "subrun", "x1e3 +%d" % t, [("=", 40)] + _repeat([("X", 1), ("=", 3)], 30) + [("=", t)], 120, 60, shift=t)
        _case(out, "subrun", "x2e5 +%d" % t, [("=", 40)] + _repeat([("X", 2), ("=", 5)], 20) + [("=", t)], 120, 60, shift=t)
    # a run of 3 cut 1 | 2 and 2 | 1 by the probe boundary at cell 64 (a boundary of every G): X, then EQ between two X runs
    for t, cut in ((63, "1|2"), (62, "2|1")):
        _case(out, "subrun", "x3 cut %s" % cut, [("=", 80), ("X", 3), ("=", t)], 120, 60, shift=t, cut=cut)
        _case(out, "subrun", "e3 cut %s" % cut, [("=", 80), ("X", 2), ("=", 3), ("X", 2), ("=", t - 2)], 120, 60, shift=t - 2, cut=cut)
    # every cell of a probe its own sub-run: as many starts as lanes
    for t in (40, 41):
        _case(out, "subrun", "x1e1 +%d" % t, [("=", 40)] + _repeat([("X", 1), ("=", 1)], 40) + [("=", t)], 120, 60, scoring=MILD, shift=t)
    # (... and 48 pairs: cells 40 ... 135 from the best cell, the whole 64-lane probe 64 ... 127)
    _case(out, "subrun", "x1e1x48 +40", [("=", 40)] + _repeat([("X", 1), ("=", 1)], 48) + [("=", 40)], 120, 60, scoring=MILD, shift=40)


BAND_L = 120


def band_cases(out):
    """validPath (src/AlignmentMatrixFast.cpp:213-220) accepts the columns band(L) of a row: 13 ... 119 of 120.  Its right bound,
    minC + L - 0.1 L, is the row's end, so only the left edge ever rejects a cell; the mirror cases run on the row's last column
    and are valid.  A diagonal path, the cells of a deletion and the cells of an insertion on the first valid column and on the
    last invalid one.  `valid`: what the construction aims at; the oracle decides (tests/test_walk_cases_cpu.py)."""
    L = BAND_L
    lo, hi = rc.band(L)
    assert (lo, hi) == (13, L - 1)
    for edge, col, valid in (("left", lo, True), ("left", lo - 1, False), ("right", hi, True)):
        _case(out, "band", "diag %s c%d" % (edge, col), [("=", 70), ("X", 1), ("=", 80)], L, col, what="diag", edge=edge, col=col, valid=valid)
    for R in (64, 70):
        script = [("=", 80), ("D", 5), ("=", R)]
        H = 80 + R
        # right: the run's rightmost cell (the first one met) on the row's last column
        _case(out, "band", "D5 R%d right c%d" % (R, hi), script, L, hi - 5, what="D", edge="right", col=hi, valid=True)
        # left: the run's leftmost cell on column lo + 1, lo and lo - 1; its row's path cell lies one column left of it.  lo + 1:
        # valid, and the follow must judge the run by its own row's bounds (the probe's first row starts R % G columns further
        # right); lo: the follow's check passes and the next probe rejects the path cell; lo - 1: the follow itself rejects.  Only
        # that row comes near the edge.
        for col in (lo + 1, lo, lo - 1):
            p = np.full(H, 18, np.int64)
            p[79] = col - 1
            p[80:] = col + 5
            _case(out, "band", "D5 R%d left c%d" % (R, col), script, L, p, what="D", edge="left", col=col, valid=col > lo)
    # an insertion of 6 whose column changes inside the run because the row start moves on by one
    script = [("=", 80), ("I", 6), ("=", 70)]
    H = 156
    for edge, first, valid in (("left", lo + 1, True), ("left", lo, False), ("right", hi, True)):
        p = np.full(H, first, np.int64)
        p[83:86] = first - 1          # (the row behind the run steps back onto `first`: its row start stands still)
        _case(out, "band", "I6 %s c%d-%d" % (edge, first, first - 1), script, L, p, what="I", edge=edge, col=first, valid=valid)


RING_EVENTS = (("I", 3), ("I", 33), ("D", 3))
RING_ROWS = (63, 64, 65, 255, 256, 257)


def _lead_for(op, n, row):
    """rows of the leading block that put the event's first-met row at `row`"""
    return row + 1 if op == "D" else row - n + 1


def lead_too_short(op, n, row):
    """an insertion of 33 costs about 88: a leading block of fewer than 45 matches is not worth it and the local alignment would
    start behind the gap.  Such a row is taken 64 rows further down (63, 64, 65 -> 127, 128, 129: the same residues)."""
    return op == "I" and 2 * _lead_for(op, n, row) < 3 * n


def ring_cases(out):
    """The event at lane 0 (R = 64) in a row = 63, 64, 65 (mod 64) and 255, 256, 257 (mod 256): the rows of its probe and of the
    followed run wrap in the ring (64 or 128 slots at L = 120, 256 at L = 420) or, in a chained tile, lie in two row blocks."""
    for L in (120, 420):
        for op, n in RING_EVENTS:
            for row in RING_ROWS:
                if lead_too_short(op, n, row):
                    row += 64
                _case(out, "ring", "L%d %s%d row%d" % (L, op, n, row), [("=", _lead_for(op, n, row)), (op, n), ("=", 64)], L, L // 2,
                      ev=(op, n), chained=False)
                assert out[-1].info["row"] == row and row % 64 in (63, 0, 1)
    # chained: every event at each residue in one script; a deletion of 1 in front of each 64-cell run restarts the probe
    for width in (1100, 1400):
        script, rows, y = [], [], 0
        for res in (63, 64, 65):
            for op, n in RING_EVENTS:
                first = y + 70                                   # earliest row the event may be met in
                row = first + (res - first) % 64
                lead = _lead_for(op, n, row) - y
                script += [("=", lead), (op, n), ("=", 64), ("D", 1)]
                y += lead + (n if op == "I" else 0) + 64
                rows.append(row)
        script.append(("=", 70))
        rng = np.random.default_rng([2424, len(out)])
        core, qry, path = rc._realize(rng, script)
        off, ln = synth.corridor_endpoints(len(qry), len(core), width, realign=True)
        t = synth.Tile(ref=core.tobytes(), qry=qry.tobytes(), row_offset=off, row_length=ln, tag="ring chained w%d" % width)
        out.append(Case(t, "ring", "chained w%d" % width, script, op_list(script), DEFAULT,
                        dict(L=width, events=gap_events(script), chained=True, rows=rows)))


def families():
    """-> [Case]"""
    out = []
    lane_cases(out)
    word_cases(out)
    word_early_cases(out)
    subrun_cases(out)
    band_cases(out)
    ring_cases(out)
    return out


def long_valid(rng, H, tag):
    """-> (a valid tile of about H rows with a gap every 64 rows, its ops): company for the tiles of a shared wave"""
    n = max(H // 128, 1)
    script = _repeat([("=", 61), ("D", 2), ("=", 64), ("I", 3)], n) + [("=", max(H - 128 * n, 40))]
    return tile(rng, script, 120, 60, tag)[0], op_list(script)


def empty_tile():
    """no cell inside the window: every row starts right of it"""
    H, W = 60, 80
    return synth.Tile(b"A" * W, b"A" * H, np.full(H, W + 10, np.int32), np.full(H, 20, np.int32), tag="empty-corridor")
