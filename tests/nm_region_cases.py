"""The low-identity regions of the per-position NM profile (cvx_job_nm_regions, cvx_nm_regions_ops, cvx_nm_regions_host): the
checker and the case families.

A plain module (no fixtures, no device): tests/test_nm_regions_cpu.py runs the host form over it, tests/test_gpu_nm_regions.py
the device forms, tools/nm_regions_rate.py borrows the checker.

The checker, literal_scan, is the loop at the top of AlignmentBuffer::detectMisalignment (reference
src/AlignmentBuffer.cpp:1316-1395, isInversion :1143-1148) written out statement by statement with its three state variables --
not the rule the library implements.  It walks `scan_len` rows (refPosition, readPosition, nm): the profile's entries, then
zeros.

Op lists are [(length, op code), ...] with the codes of include/cvx_align.h.  How the engineered lists place their marks: a row
is an EQ / X / D column once both positions passed 16, its nm the number of mismatched bases and gap-op starts among the last
32 columns.  After 60 clean columns an X run of 9 at columns c .. c + 8 reaches nm = 9 at c + 8 and the EQ columns behind it
keep 9 until the run's first base leaves the window: marks at the 24 rows c + 8 .. c + 31, nothing before and nothing after.
Two such bursts with F >= 33 EQ columns between the X runs have exactly F - 15 unmarked rows between them.
"""
import numpy as np

from ngmlr_amd import synth

I, D, EQ, X = 1, 2, 7, 8
MAX_DISTANCE = 20


def literal_scan(rows, scan_len):
    """-> (regions [(startInv, stopInv, startInvRead, stopInvRead), ...] in the order the reference emits them,
    (open, distance, (startInv, stopInv, startInvRead, stopInvRead)) as the loop leaves them).
    rows: at least scan_len rows of three ints.  (32 - nm) / 32.0f and both constants of isInversion are exact in binary32, so
    Python's doubles take the same branches."""
    rows = np.asarray(rows).tolist()
    inversionPositionShift = 0
    maxDistance = MAX_DISTANCE
    distance = maxDistance
    startInv = stopInv = startInvRead = stopInvRead = -1
    out = []
    for i in range(scan_len):
        refPosition, readPosition, nmv = rows[i]
        nm = (32 - nmv) / 32.0
        isInversion = nm > 0.0 and nm < 0.75
        if startInv == -1:
            if isInversion:
                startInv = refPosition - inversionPositionShift
                startInvRead = readPosition - inversionPositionShift
                stopInv = refPosition - inversionPositionShift
                stopInvRead = readPosition - inversionPositionShift
        else:
            if isInversion:
                stopInv = refPosition - inversionPositionShift
                stopInvRead = readPosition - inversionPositionShift
                distance = maxDistance
            else:
                if distance == 0:
                    out.append((startInv, stopInv, startInvRead, stopInvRead))
                    startInv = stopInv = startInvRead = stopInvRead = -1
                    distance = maxDistance
                else:
                    distance -= 1
    return out, (int(startInv != -1), distance, (startInv, stopInv, startInvRead, stopInvRead))


def padded(triples, scan_len):
    """the rows the consumer walks: the entries, then zeros up to scan_len (cut there when there are more)"""
    tri = np.asarray(triples, dtype=np.int32).reshape(-1, 3)
    rows = np.zeros((max(int(scan_len), 0), 3), dtype=np.int32)
    n = min(len(tri), len(rows))
    rows[:n] = tri[:n]
    return rows


def same(want, got_regions, got_open):
    """None when the literal scan's answer `want` equals (regions int32[r, 4], open record) of the library (fields in the
    library's order: ref_start, ref_stop, read_start, read_stop), else a short description"""
    regs, (op, dist, r) = want
    g = [tuple(int(v) for v in row) for row in np.asarray(got_regions).reshape(-1, 4)]
    if g != [tuple(x) for x in regs]:
        return "regions %s != %s" % (g[:4], regs[:4])
    go = (int(got_open["open"]), int(got_open["distance"]), tuple(int(v) for v in got_open["region"]))
    if go != (op, dist, tuple(r)):
        return "open %s != %s" % (go, (op, dist, tuple(r)))
    return None


# --------------------------------------------------------------------------- tiles with a stretch the read does not share

def stretch_tile(rng, length=3000, stretch=200, kind="inv", err=0.1, tag=""):
    """A mutated read over `length` reference bases whose middle `stretch` bases are the reverse complement (kind "inv") or
    unrelated (kind "random"): the alignment runs through the stretch at low identity.  Full-width anchors corridor."""
    ref = synth.random_ref(rng, length)
    a = (length - stretch) // 2
    src = ref.copy()
    src[a:a + stretch] = synth.revcomp(ref[a:a + stretch]) if kind == "inv" else synth.random_ref(rng, stretch)
    qry = synth.mutate(rng, src, err, (6, 3, 1))
    off, ln = synth.corridor_anchors(len(qry), length, mult=2, scatter_left=20.0, scatter_right=20.0)
    return synth.Tile(ref=ref.tobytes(), qry=qry.tobytes(), row_offset=off, row_length=ln, tag=tag or "%s%d" % (kind, stretch))


def stretch_tiles(n=60, seed=808, length=3000):
    rng = np.random.default_rng(seed)
    return [stretch_tile(rng, length, int(rng.integers(60, 401)), "inv" if i % 2 else "random", float(rng.choice([0.05, 0.1, 0.15])),
                         tag="stretch%d" % i) for i in range(n)]


def plain_tiles(n=12, seed=809, length=5000, err=0.15):
    rng = np.random.default_rng(seed)
    return [synth.make_tile(rng, length, err=err, ratio=(6, 3, 1), corridor="anchors", scatter=25.0, tag="plain%d" % i) for i in range(n)]


def clean_tiles(n=8, seed=810, length=2000):
    """reads at 3 % error: no row comes near 9 mismatches in 32 columns, no region"""
    rng = np.random.default_rng(seed)
    return [synth.make_tile(rng, length, err=0.03, ratio=(6, 3, 1), corridor="anchors", scatter=25.0, tag="clean%d" % i) for i in range(n)]


def tail_tiles(n=10, seed=811, length=400):
    """Reads without indels whose last 32 + k bases are nine substitutions at every other base, then 15 + k matches (every
    suffix of that end scores above zero, so the local alignment runs to the read's last base): the last marked row lies k rows
    in front of the last entry and 17 + k rows -- the head that has no entry -- in front of alignmentLength.  k = 0 .. 3 leave
    the run open, k = 4 closes it.  (The aligner trades the substitutions of about half of these reads for pairs of gaps, whose
    insertion columns lengthen the zero tail and close the run: the tests count what is left, they do not expect it per tile.)"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        k = i % 5
        ref = synth.random_ref(rng, length)
        qry = ref[20:length - 20].copy()
        at = len(qry) - (32 + k) + 2 * np.arange(9)
        qry[at] = synth._ACGT[(synth._CODE[qry[at]].astype(np.int64) + 1) % 4]
        off, ln = synth.corridor_anchors(len(qry), length, mult=2, scatter_left=20.0, scatter_right=20.0)
        out.append(synth.Tile(ref=ref.tobytes(), qry=qry.tobytes(), row_offset=off, row_length=ln, tag="tail%d_k%d" % (i, k)))
    return out


# --------------------------------------------------------------------------- engineered op lists

HEAD = (60, EQ)          # 17 columns without a row, 43 clean rows
BURST = (9, X)           # with the EQ columns behind it: 24 marked rows


def _case(tag, ops, qstart=0, status=0, **expect):
    return dict(tag=tag, ops=list(ops), qstart=qstart, status=status, expect=expect)


def family_between():
    """exactly 20, 21 and 22 unmarked rows between two marks: 20 merge, 21 and 22 split"""
    out = []
    for rows_between, n_regions in ((20, 1), (21, 2), (22, 2)):
        out.append(_case("between%d" % rows_between, [HEAD, BURST, (rows_between + 15, EQ), BURST, (80, EQ)],
                         between=rows_between, regions=n_regions, open=0))
    return out


def family_tail():
    """the last mark exactly 20 and 21 rows in front of scan_len: the run stays open (dropped) / is emitted.  Rows behind the
    last mark: once EQ entries plus the 17 head columns that have no entry, once only insertion columns and that head."""
    out = []
    for behind, n_regions in ((20, 0), (21, 1)):
        # the burst's last mark is 23 columns into the EQ op behind the X run
        out.append(_case("tail_eq%d" % behind, [HEAD, BURST, (23 + behind - 17, EQ)], behind=behind, regions=n_regions, open=1 - n_regions))
        out.append(_case("tail_ins%d" % behind, [HEAD, BURST, (23, EQ), (behind - 17, I)], behind=behind, regions=n_regions, open=1 - n_regions))
        out.append(_case("tail_ins_qstart%d" % behind, [HEAD, BURST, (23, EQ), (behind - 17, I)], qstart=33, behind=behind, regions=n_regions,
                         open=1 - n_regions))
    # (fewer rows behind the last mark: the countdown the open record reports)
    for behind in (17, 18, 19):
        out.append(_case("tail_eq%d" % behind, [HEAD, BURST, (23 + behind - 17, EQ)], behind=behind, regions=0, open=1))
    return out


def family_thresholds():
    """nm at 8, 9, 31, 32, 33 and beyond: 8 and 32 are unmarked, 9 and 31 marked; an X run of 40 columns unmarks its own
    middle (9 rows at 32: still one region), one of 60 splits itself (29 rows at 32); gap ops right behind each other count
    past 32 (the k-th D entry carries 2 k, or 2 k + 1 behind a mismatch)"""
    gaps20 = [(1, I), (1, D)] * 20
    return [
        _case("x8", [HEAD, (8, X), (80, EQ)], regions=0, open=0, max_nm=8),
        _case("x9", [HEAD, (9, X), (80, EQ)], regions=1, open=0, max_nm=9),
        _case("x31", [HEAD, (31, X), (80, EQ)], regions=1, open=0, max_nm=31),
        _case("x32", [HEAD, (32, X), (80, EQ)], regions=1, open=0, max_nm=32),
        _case("x33", [HEAD, (33, X), (80, EQ)], regions=1, open=0, max_nm=32),
        _case("x40", [HEAD, (40, X), (80, EQ)], regions=1, open=0, max_nm=32),
        _case("x60", [HEAD, (60, X), (80, EQ)], regions=2, open=0, max_nm=32),
        _case("gaps33", [HEAD] + gaps20 + [(90, EQ)], open=0, min_max_nm=33),
        _case("gaps33_open", [HEAD] + gaps20 + [(30, EQ)], min_max_nm=33),
        _case("gaps_odd", [HEAD, (1, X)] + gaps20 + [(90, EQ)], open=0, has_nm=(9, 31, 33)),
        _case("gaps_even", [HEAD] + gaps20 + [(90, EQ)], open=0, has_nm=(8, 32, 34)),
    ]


def family_boundaries():
    """regions and breaks across lanes (every op is a lane) and across the 64-op steps of the kernel: `p` one-column EQ ops in
    front move the two bursts and the EQ run between them over op index 64; one EQ op of 5 000 columns between two bursts;
    bursts in many ops; marks that are D entries only"""
    out = []
    for p in (0, 58, 59, 60, 61, 62, 63, 64, 65, 125, 126, 127):
        for rows_between in (20, 21):
            out.append(_case("step%d_%d" % (p, rows_between), [HEAD] + [(1, EQ)] * p + [BURST, (rows_between + 15, EQ), BURST, (80, EQ)],
                             between=rows_between, regions=1 if rows_between == 20 else 2, open=0))
    # the EQ run between the bursts as single columns: the break spans 35 / 36 lanes and a step boundary
    for rows_between in (20, 21):
        out.append(_case("lanes%d" % rows_between, [HEAD] + [(1, EQ)] * 40 + [BURST] + [(1, EQ)] * (rows_between + 15) + [BURST, (80, EQ)],
                         between=rows_between, regions=1 if rows_between == 20 else 2, open=0))
    out.append(_case("long_eq", [HEAD, BURST, (5000, EQ), BURST, (80, EQ)], regions=2, open=0))
    out.append(_case("long_eq_open", [HEAD, BURST, (5000, EQ), BURST, (25, EQ)], regions=1, open=1))
    out.append(_case("long_x", [HEAD, (5000, X), (80, EQ)], regions=2, open=0))
    out.append(_case("many_bursts", [HEAD] + [BURST, (70, EQ)] * 150, regions=150, open=0))
    out.append(_case("many_merged", [HEAD] + [BURST, (35, EQ)] * 150 + [(60, EQ)], regions=1, open=0))
    # gap ops right behind each other: the k-th D entry carries nm = 2 k; the D run of 30 behind them is 30 marked rows at one
    # read position, and the EQ columns behind it see three set bits
    out.append(_case("d_only", [HEAD] + [(1, I), (1, D)] * 4 + [(1, I), (30, D), (80, EQ)], regions=1, open=0, d_only=True))
    out.append(_case("d_only_twice", [HEAD] + ([(1, I), (1, D)] * 4 + [(1, I), (30, D), (80, EQ)]) * 2, regions=2, open=0, d_only=True))
    out.append(_case("d_long", [HEAD] + [(1, I), (1, D)] * 4 + [(1, I), (700, D), (80, EQ)], regions=1, open=0, d_only=True))
    return out


def family_empty():
    """no entries at all (nothing passes position 16; an empty op list), and a tile without a valid alignment"""
    return [
        _case("short_eq", [(10, EQ)], regions=0, open=0, entries=0),
        _case("ins_only", [(30, I)], regions=0, open=0, entries=0),
        _case("del_at_read_start", [(300, D), (10, EQ)], regions=0, open=0, entries=0),
        _case("no_ops", [], regions=0, open=0, entries=0),
        _case("invalid", [], status=1, regions=0, open=0, entries=0),
    ]


def family_random(n=60, seed=4242):
    """seeded op lists no alignment produces: mismatch-rich stretches between clean ones, gap ops behind each other, ops longer
    than a wave, hundreds of ops"""
    rng = np.random.default_rng(seed)
    out = []
    for c in range(n):
        ops = []
        for _seg in range(int(rng.integers(1, 12))):
            dirty = rng.random() < 0.5
            for _k in range(int(rng.integers(1, 60))):
                if dirty:
                    t = int(rng.choice([EQ, X, X, I, D]))
                    ln = int(rng.integers(1, 6)) if rng.random() < 0.85 else int(rng.integers(6, 80))
                else:
                    t = int(rng.choice([EQ, EQ, EQ, EQ, X, I, D]))
                    ln = int(rng.integers(1, 40)) if t == EQ else int(rng.integers(1, 3))
                ops.append((ln, t))
        out.append(_case("random%d" % c, ops, qstart=int(rng.integers(0, 40)) if c % 2 else 0))
    return out


def engineered():
    return family_between() + family_tail() + family_thresholds() + family_boundaries() + family_empty() + family_random()


def pack_ops(cases):
    """-> (capi.CvxResult array, uint32 ops arena) for cvx_nm_regions_ops / cvx_nm_profile_ops / cvx_format_alignment"""
    from ngmlr_amd import capi
    arena, results = [], []
    for c in cases:
        r = capi.CvxResult()
        r.status = c["status"]
        r.ref_position = 0
        r.qstart = c["qstart"]
        r.n_ops = len(c["ops"])
        r.ops_begin = len(arena)
        arena += [(ln << 4) | t for ln, t in c["ops"]]
        results.append(r)
    return (capi.CvxResult * max(len(results), 1))(*results), np.array(arena, dtype=np.uint32)


def host_profile(lib, case, res, arena, seed=1):
    """The profile of one case through the host text stage (cvx_format_alignment, pinned to the reference elsewhere):
    -> (triples int32[entries, 3], alignment_length).  The reference string is arbitrary: the profile depends on the ops alone."""
    import ctypes as C
    from ngmlr_amd import capi
    ops = case["ops"]
    if case["status"] != 0:
        return np.zeros((0, 3), dtype=np.int32), 0
    ref_len = sum(ln for ln, t in ops if t != I) + 300
    qry_len = sum(ln for ln, t in ops if t != D) + case["qstart"]
    ref = synth.random_ref(np.random.default_rng(seed), ref_len).tobytes()
    cap = 16 * (ref_len + qry_len) + 64
    cig, md = C.create_string_buffer(cap), C.create_string_buffer(cap)
    nm = np.zeros((ref_len + qry_len + 16, 3), dtype=np.int32)
    txt = capi.CvxAlignmentText()
    rc = lib.cvx_format_alignment(C.byref(res), arena.ctypes.data, ref, ref_len, qry_len, 0, 0, cig, cap, md, cap, nm.ctypes.data, len(nm), C.byref(txt))
    assert rc == 0, (case["tag"], rc)
    return nm[:txt.nm_count].copy(), int(txt.alignment_length)


def check_expectations(case, rows, want):
    """what a family says about its own cases, asserted on the literal scan's answer and the profile (so that a case that
    misses what it was aimed at fails here, not silently)"""
    e = case["expect"]
    regs, (op, dist, _r) = want
    marked = np.flatnonzero((rows[:, 2] >= 9) & (rows[:, 2] <= 31))
    if "regions" in e:
        assert len(regs) == e["regions"], (case["tag"], len(regs))
    if "open" in e:
        assert op == e["open"], (case["tag"], op, dist)
    if "between" in e:
        gaps = np.diff(marked) - 1
        assert gaps.max() == e["between"] and (gaps > 0).sum() == 1, (case["tag"], gaps[gaps > 0])
    if "behind" in e:
        assert len(rows) - 1 - marked[-1] == e["behind"], (case["tag"], len(rows) - 1 - marked[-1])
    if "max_nm" in e:
        assert rows[:, 2].max() == e["max_nm"], (case["tag"], rows[:, 2].max())
    if "min_max_nm" in e:
        assert rows[:, 2].max() >= e["min_max_nm"], (case["tag"], rows[:, 2].max())
    if "has_nm" in e:
        assert set(e["has_nm"]) <= set(rows[:, 2].tolist()), (case["tag"], sorted(set(rows[:, 2].tolist())))
    if "entries" in e:
        assert not rows[:, 2].any() and not rows[:, 0].any()
    if e.get("d_only"):
        # every marked row is a D entry: the marks of one region share one read position
        assert len(marked) >= 30 and len(set(rows[marked, 1].tolist())) == len(regs), case["tag"]


def random_profiles(n=3000, seed=2718):
    """seeded (triples, scan_len): runs of marked and unmarked rows of every length around the 20 / 21 boundary, nm on both
    sides of both thresholds, tails of -5 .. 60 rows behind the entries (a negative tail cuts the entries)"""
    rng = np.random.default_rng(seed)
    for c in range(n):
        rows = []
        for _seg in range(int(rng.integers(0, 14))):
            ln = int(rng.choice([1, 2, 5, 19, 20, 21, 22, 23, 40])) if rng.random() < 0.7 else int(rng.integers(1, 70))
            if rng.random() < 0.5:
                rows += [int(rng.choice([9, 10, 20, 30, 31])) for _ in range(ln)]
            else:
                rows += [int(rng.choice([0, 0, 1, 8, 32, 33, 40])) for _ in range(ln)]
        n_e = len(rows)
        tri = np.zeros((n_e, 3), dtype=np.int32)
        tri[:, 0] = 1 + np.cumsum(rng.integers(0, 3, size=n_e))
        tri[:, 1] = 1 + np.cumsum(rng.integers(0, 3, size=n_e))
        tri[:, 2] = rows
        tail = int(rng.choice([0, 1, 19, 20, 21, 22])) if rng.random() < 0.7 else int(rng.integers(-5, 61))
        yield tri, max(0, n_e + tail)
