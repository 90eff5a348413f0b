"""The corridor retry ladder of AlignmentBuffer::computeAlignment (reference src/AlignmentBuffer.cpp:259-425) restated in Python
on ngmlr_amd.synth's restatements of the four corridor builders, the expectation of a ladder job from a CPU oracle, and the
engineered tiles of tests/test_gpu_ladder.py.  cvx_ladder_rung / cvx_submit_ladder (include/cvx_align.h) are checked against this."""
import numpy as np

from ngmlr_amd import synth

F32 = np.float32
ANCHORS, REALIGN, SHORT, FULL = 1, 2, 4, 8
MAX_RUNGS = 5


def cap(W):
    """maxCorridorSize = refSeqLen * 2 (:265).  refSeqLen is onRefStop - onRefStart + 1 (:209): the decoded window's length plus
    one; W, a tile's ref_len, is the string's own length (what the builders' k is computed from)."""
    return 2 * (W + 1)


def rung_exists(W, ladder, m):
    """:259-266, :292-294: corridor = min(corridor, 2 * refSeqLen); while corridor * multiplier <= 2 * refSeqLen and retryCount-- > 0"""
    corridor, _, _, flags = ladder
    if m < 1 or m > (1 if flags & FULL else MAX_RUNGS):
        return False
    return min(int(corridor), cap(W)) * m <= cap(W)


def ladder_length(W, ladder):
    m = 0
    while rung_exists(W, ladder, m + 1):
        m += 1
    return m


def rung_desc(H, W, ladder, m):
    """(kind, k, d, right, offset, width) of rung m as Tile.desc has it, None where the rung does not exist: what the builder
    computeAlignment picks at :309-326 writes at multiplier m."""
    corridor, left, right, flags = ladder
    if not rung_exists(W, ladder, m):
        return None
    cm = min(int(corridor), cap(W)) * m
    if flags & FULL:
        return synth.full_desc(H, W + 1)                  # getCorridorFull(refSeqLen)
    if flags & SHORT:
        return synth.linear_desc(H, cm)                   # getCorridorLinear(corridor * m)
    if (flags & ANCHORS) and not (flags & REALIGN) and m < 3:
        # getCorridorEndpointsWithAnchors from :184 on, corridorLeft / corridorRight as they stand after :178-182
        le = F32(F32(left) * F32(m))
        ri = F32(F32(right) * F32(m))
        width = int(np.trunc(F32(le + ri)))
        if H == 0 or W == 0:
            return (2, 0.0, 0.0, 0.0, 0, width)           # no slope: constant rows, the tile is empty (include/cvx_align.h)
        k = synth.anchors_desc(H, W)[1]
        return (1, k, 0.0, float(ri), 0, width)
    if H == 0 or W == 0:
        return (2, 0.0, 0.0, 0.0, 0, cm // (1 if flags & REALIGN else 4))
    return synth.endpoints_desc(H, W, cm, realign=bool(flags & REALIGN))      # getCorridorEndpoints(corridor * m, realign)


def rung_rows(H, desc):
    kind, k, d, right, offset, width = desc
    if kind == 2:
        return np.full(H, offset, dtype=np.int32), np.full(H, width, dtype=np.int32)
    return synth.affine_rows(H, k, d, right, width)


def rung_tile(ref: bytes, qry: bytes, ladder, m, tag=""):
    """the row-array tile of rung m (with its closed form beside it), None where the rung does not exist"""
    desc = rung_desc(len(qry), len(ref), ladder, m)
    if desc is None:
        return None
    off, ln = rung_rows(len(qry), desc)
    return synth.Tile(ref, qry, off, ln, tag="%s@%d" % (tag, m), desc=desc)


def has_cells(tile):
    """a read row and a cell inside [0, W): anything else is CVX_TILE_EMPTY (the reference never aligns such a tile)"""
    off = tile.row_offset.astype(np.int64)
    return bool(len(off)) and bool(np.any(np.maximum(off, 0) < np.minimum(off + tile.row_length, len(tile.ref))))


def too_large(H, desc, max_matrix_mb):
    """src/AlignmentMatrixFast.cpp:45: (ulong) (matrixSize / 1000.0f / 1000.0f) < maxMatrixSizeMB"""
    mb = F32(F32(F32(H * desc[5]) / F32(1000.0)) / F32(1000.0))
    return not (int(mb) < max_matrix_mb)


def climb(ref: bytes, qry: bytes, ladder, valid, max_matrix_mb=10000):
    """The ladder of one tile over `valid(tile) -> bool` (an oracle's verdict on one SingleAlign call): (rung reported,
    [the rungs' tiles])."""
    H, W = len(qry), len(ref)
    tiles = []
    for m in range(1, MAX_RUNGS + 1):
        t = rung_tile(ref, qry, ladder, m)
        if t is None:
            break
        tiles.append(t)
        if not has_cells(t) or too_large(H, t.desc, max_matrix_mb):
            continue                                      # EMPTY / TOO_LARGE: the reference's -1
        if valid(t):
            break
    return len(tiles), tiles


# --------------------------------------------------------------------------- the CPU sweep

def sweep(seed=20, n=1500):
    """(H, W, ladder, m) for cvx_ladder_rung against rung_desc: random cases, then the corners the issue names."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        H = int(rng.integers(1, 30000))
        W = int(rng.integers(1, 40000))
        flags = int(rng.choice([0, ANCHORS, REALIGN, ANCHORS | REALIGN, SHORT, SHORT | ANCHORS, FULL, FULL | SHORT, FULL | ANCHORS | REALIGN]))
        corridor = int(rng.choice([int(rng.integers(0, cap(W) + 1)), int(rng.integers(cap(W), 6 * W + 8)), int(rng.integers(0, 600))]))
        left = float(F32(128 + rng.random() * 900))
        right = float(F32(128 + rng.random() * 900))
        for m in range(1, 7):
            out.append((H, W, (corridor, left, right, flags), m))
    # left / right whose fractions make (int) (left * m + right * m), rounded to binary32 at every step, differ from
    # (int) ((left + right) * m) taken exactly (doubling is exact in binary32: only the sum's rounding can separate them)
    found = 0
    while found < 60:
        left = float(F32(128 + rng.random() * 400))
        right = float(F32(128 + rng.random() * 400))
        for m in (2,):
            a = int(np.trunc(F32(F32(F32(left) * F32(m)) + F32(F32(right) * F32(m)))))
            b = int(np.trunc(F32(F32(F32(left) + F32(right)) * F32(m))))
            c = int(np.trunc((float(left) + float(right)) * m))
            if a != b or a != c:
                found += 1
                for mm in (1, 2, 3):
                    out.append((int(rng.integers(500, 9000)), int(rng.integers(500, 9000)), (4000, left, right, ANCHORS), mm))
    # corridor > 2 * ref_len (the clamp leaves exactly one rung), and the cap cutting the ladder at every length 1 ... 5
    for W in (100, 999, 5000):
        c2 = cap(W)
        for corridor in (c2 + 1, 3 * W, c2, c2 // 2, c2 // 2 + 1, c2 // 3, c2 // 3 + 1, c2 // 4, c2 // 4 + 1, c2 // 5, c2 // 5 + 1, c2 // 6):
            for flags in (0, ANCHORS, SHORT, REALIGN, FULL):
                for m in range(1, 7):
                    out.append((W + 37, W, (corridor, 184.32, 184.32, flags), m))
    # nothing to align
    for H, W in ((0, 0), (0, 50), (50, 0), (1, 1)):
        for flags in (0, ANCHORS, SHORT, REALIGN, FULL):
            for m in range(1, 7):
                out.append((H, W, (64, 140.5, 141.25, flags), m))
    return out


# --------------------------------------------------------------------------- engineered tiles for the GPU suite

def engineered(seed=2025):
    """-> list of (tag, ref, qry, ladder): reads of 600 bases cut from one seeded 2 kb random reference -- 300 matched bases,
    a deletion of d, 300 matched bases -- against the window they span, so that the endpoints corridor runs corner to corner
    and the path bulges d / 2 columns off it; plus the other builders, a REALIGN ladder, 1-row and empty tiles."""
    rng = np.random.default_rng(seed)
    genome = synth.random_ref(rng, 2000)

    def deletion(d, at=100):
        ref = genome[at:at + 600 + d]
        qry = np.concatenate([ref[:300], ref[300 + d:]])
        return ref.tobytes(), qry.tobytes()
    out = []
    for d in (0, 10, 20, 30, 40, 50, 60, 80, 100, 130, 160, 200, 250, 300, 400):
        out.append(("ep256-d%d" % d, *deletion(d), (256, 0.0, 0.0, 0)))
    for d in (10, 100, 300, 600, 900):
        out.append(("ep64-d%d" % d, *deletion(d), (64, 0.0, 0.0, 0)))
    for d in (0, 20, 50, 150, 250, 300, 400):
        out.append(("anchors-d%d" % d, *deletion(d), (256, 184.32, 184.32, ANCHORS)))
    out.append(("anchors-narrow-d300", *deletion(300), (400, 40.0, 40.0, ANCHORS)))      # fails rungs 1 and 2 (widths 80, 160), then the endpoints form
    out.append(("anchors-narrow-d200", *deletion(200), (480, 30.0, 30.0, ANCHORS)))
    for d in (0, 40, 200):
        out.append(("realign-d%d" % d, *deletion(d), (100, 0.0, 0.0, REALIGN)))
        out.append(("realign-anchors-d%d" % d, *deletion(d), (100, 184.32, 184.32, ANCHORS | REALIGN)))
    out.append(("full-d50", *deletion(50), (256, 0.0, 0.0, FULL)))
    out.append(("full-d700", *deletion(700), (64, 0.0, 0.0, FULL | ANCHORS)))
    short = genome[700:800].tobytes()
    out.append(("short-120", short, synth.mutate(rng, genome[700:800], 0.05).tobytes(), (120, 0.0, 0.0, SHORT)))
    out.append(("short-40", short, synth.mutate(rng, genome[700:800], 0.05).tobytes(), (40, 0.0, 0.0, SHORT)))
    out.append(("short-8-shifted", genome[700:860].tobytes(), genome[740:840].tobytes(), (8, 0.0, 0.0, SHORT)))
    out.append(("one-row", genome[20:21].tobytes(), genome[20:21].tobytes(), (2, 0.0, 0.0, REALIGN)))
    out.append(("one-row-no-cell", genome[10:50].tobytes(), genome[20:21].tobytes(), (16, 0.0, 0.0, 0)))      # every rung's row lies left of the window
    out.append(("one-row-anchors", genome[10:50].tobytes(), genome[20:21].tobytes(), (16, 130.0, 130.0, ANCHORS)))
    out.append(("empty-read", genome[10:50].tobytes(), b"", (16, 0.0, 0.0, 0)))
    out.append(("empty-window", b"", genome[10:50].tobytes(), (16, 130.0, 130.0, ANCHORS)))
    out.append(("empty-both", b"", b"", (16, 0.0, 0.0, FULL)))
    return out
