"""Shared by tests/test_inv_checks_cpu.py and tests/test_gpu_inv_checks.py: engineered calls of checkForSV (reference
src/AlignmentBuffer.cpp:1158-1235), what they must give -- the rule restated here from the reference's text, the windows from
cvx_stage_windows_host (the pinned restatement of DecodeRefSequence), the scores from the score oracle -- and the calls the
recorder hook of tools/make_golden_inv_checks.sh took from the unmodified reference (tests/golden/inv_checks_*.npz)."""
import gzip
import hashlib
import os

import numpy as np

from ngmlr_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
MASK64 = (1 << 64) - 1
SCORED, TOO_SHORT, NO_READ, NO_WINDOW = 0, 1, 2, 3


def cdiv2(a):
    """C's int division by two: towards zero"""
    return -((-a) // 2) if a < 0 else a // 2


def revcomp(q):
    """computeReverseSeq / cplBase (:1117-1141): A<->T, C<->G, every other byte unchanged, order reversed"""
    cpl = {65: 84, 84: 65, 67: 71, 71: 67}
    return bytes(cpl.get(c, c) for c in reversed(q))


class Call:
    """one region of one tile: read (fullReadSeq), P = interval->onRefStart, O = Align::PositionOffset, the region"""

    def __init__(self, tag, read, P, O, region):
        self.tag, self.read, self.P, self.O, self.region = tag, bytes(read), int(P), int(O), tuple(int(x) for x in region)

    def plan(self):
        """-> (status,) or (None, position, buffer_len, midRead): the outcomes in the reference's order"""
        rs, re_, qs, qe = self.region
        mid_ref, mid_read, inv = cdiv2(rs + re_), cdiv2(qs + qe), abs(re_ - rs)
        if inv <= 10:
            return (TOO_SHORT,)
        if not (50 <= mid_read and mid_read + 50 < len(self.read)):
            return (NO_READ,)
        return (None, (self.P + self.O + mid_ref - 250 - inv // 2) & MASK64, inv + 500, mid_read)


def expected(lib, genome, calls, oracle):
    """the records the calls must give, INV_CHECK_DTYPE: windows through cvx_stage_windows_host, scores through the oracle"""
    from ngmlr_amd import aligner
    binref, nib, starts = genome
    out = np.zeros(len(calls), dtype=aligner.INV_CHECK_DTYPE)
    plans = [c.plan() for c in calls]
    win = [i for i, p in enumerate(plans) if p[0] is None]
    pairs = [(plans[i][1], plans[i][2], 0, 0) for i in win]
    windows, _q, status = aligner.stage_windows_host(lib, binref, nib, starts, [b"A"], pairs) if win else ([], [], [])
    refs, qrys = [], []
    for k, i in enumerate(win):
        mid = plans[i][3]
        part = calls[i].read[mid - 50:mid + 50]
        assert len(part) == 100
        w = b"" if status[k] else windows[k]      # the reference scores against the zeroed buffer
        refs += [w, w]
        qrys += [part, revcomp(part)]
        out[i]["status"] = NO_WINDOW if status[k] else SCORED
        out[i]["window_chars"] = len(w)
    sc = oracle.scores(refs, qrys) if refs else np.zeros(0, dtype=np.float32)
    for k, i in enumerate(win):
        out[i]["score_fwd"], out[i]["score_rev"] = sc[2 * k], sc[2 * k + 1]
    for i, p in enumerate(plans):
        if p[0] is not None:
            out[i]["status"] = p[0]
    return out


def as_tiles(calls):
    """consecutive calls with the same (read, P, O) are the regions of one tile -> the arguments of cvx_inv_checks*:
    (qrys, ref_positions, position_offsets, region_off, regions)"""
    qrys, pos, po, off, reg = [], [], [], [0], []
    for c in calls:
        if not qrys or (qrys[-1], pos[-1], po[-1]) != (c.read, c.P, c.O):
            qrys.append(c.read); pos.append(c.P); po.append(c.O); off.append(off[-1])
        reg.append(c.region)
        off[-1] += 1
    return qrys, np.array(pos, dtype=np.uint64), np.array(po, dtype=np.int32), np.array(off, dtype=np.uint64), np.array(reg, dtype=np.int32).reshape(-1, 4)


def with_empty_tiles(args, every=3):
    """the same call with tiles that own no region put between the others (the kernel finds a region's tile by its offset)"""
    qrys, pos, po, off, reg = args
    q2, p2, o2, f2 = [], [], [], [0]
    for i in range(len(qrys)):
        if i % every == 0:
            q2.append(b"ACGT" * 40); p2.append(12345); o2.append(-7); f2.append(f2[-1])
        q2.append(qrys[i]); p2.append(int(pos[i])); o2.append(int(po[i])); f2.append(int(off[i + 1]))
    q2.append(b""); p2.append(0); o2.append(0); f2.append(f2[-1])
    return q2, np.array(p2, dtype=np.uint64), np.array(o2, dtype=np.int32), np.array(f2, dtype=np.uint64), reg


# --------------------------------------------------------------------------- the engineered genome and calls

def small_genome(lib):
    """two contigs (14 000 and 3 000 bases, a run of N in the first) -> ((binref, nibbles, starts), contigs)"""
    from ngmlr_amd import aligner
    rng = np.random.default_rng(606)
    c0, c1 = synth.random_ref(rng, 14000), synth.random_ref(rng, 3000)
    c0[5000:5040] = ord("N")
    contigs = [c0.tobytes(), c1.tobytes()]
    return aligner.encode_genome(lib, contigs), contigs


def _read_over(rng, contig, a, n, err=0.06):
    q = np.frombuffer(contig[a:a + n], dtype=np.uint8).copy()
    hit = rng.random(n) < err
    q[hit] = synth._ACGT[(synth._CODE[q[hit]].astype(np.int64) + 1) % 4]
    return q.tobytes()


def engineered(lib):
    """-> (genome, calls): every family of the issue on the small genome"""
    genome, contigs = small_genome(lib)
    _b, nib, starts = genome
    s0, s1, L = int(starts[0]), int(starts[1]), nib - 1
    rng = np.random.default_rng(707)
    c0 = contigs[0]
    calls = []
    # a read of 1 000 bases over contig 0 from base 2 000: the window of a region at (r, r) lies around genome base 2 000 + r
    read = _read_over(rng, c0, 2000, 1000)
    H, P = len(read), s0 + 2000

    def add(tag, region, O=0, read_=read, P_=P):
        calls.append(Call(tag, read_, P_, O, region))
    add("invLen 10", (400, 410, 400, 410))
    add("invLen 11", (400, 411, 400, 411))
    add("invLen 11, stop before start", (411, 400, 411, 400))
    add("midRead 49", (300, 360, 49, 50))          # (49 + 50) / 2 = 49
    add("midRead 50", (300, 360, 50, 50))
    add("midRead + 50 == H", (300, 360, H - 50, H - 50))
    add("midRead + 50 == H - 1", (300, 360, H - 51, H - 51))
    add("midRead negative", (300, 360, -400, 100))
    for O in (0, 1, 2, 3, -1, -2):                  # odd and even position ...
        for stop in (460, 461):                     # ... odd and even window length
            add("O %d stop %d" % (O, stop), (400, stop, 400, stop), O)
    add("the N run", (2980, 3060, 500, 520))
    add("N run, odd", (2981, 3060, 500, 520), 1)
    # window lengths on either side of one chunk of the kernel and of kDiagMaxRef: characters = (position & 1) + len rounded up to even
    # (a region (a, a + inv) has midRef = a + inv / 2, so its window starts at P + O + a - 250: O picks the parity)
    for odd, inv in ((1, 12), (1, 1548), (0, 1550), (1, 1550), (0, 5502), (1, 3801)):      # 511, 2 047, 2 048, 2 049, 6 000, 4 301
        a = 3000
        add("long window, inv %d" % inv, (a, a + inv, 480, 520), (odd - (P + a - 250)) & 1)
    # a read that carries the reverse complement of its window's middle: score_rev wins
    inv_read = bytearray(read)
    inv_read[450:650] = revcomp(bytes(read[450:650]))
    add("planted inversion", (460, 640, 460, 640), 0, bytes(inv_read))
    # a read part with N, lower case, U and bytes that are no letters
    odd = bytearray(read)
    odd[470:480] = b"NNNNnnnnNN"
    odd[480:500] = bytes(odd[480:500]).lower()
    odd[500:506] = b"-*.0 \x7f"
    odd[506:510] = b"UuUu"
    odd[510:514] = b"acgt"
    add("read part with N, lower case, non-letters", (460, 540, 460, 540), 0, bytes(odd))
    add("the same, odd", (460, 541, 461, 540), 1, bytes(odd))
    # across the spacer between the contigs, across the end of the genome, at and past GetConcatRefLen(), below zero
    end0 = s0 + len(c0)
    tail = _read_over(rng, c0, len(c0) - 600, 600)
    for O in (0, 1):
        calls.append(Call("across the spacer", tail, end0 - 600, O, (500, 580, 500, 580)))
        calls.append(Call("into the spacer only", tail, end0 - 600, O, (900, 960, 300, 360)))
    r2 = _read_over(rng, contigs[1], 2000, 1000)
    for shift in (-700, -400, -251, -250, -249, -1, 0, 1, 2, 5000):
        # position = P + 300 - 250 - 30 = P + 20
        calls.append(Call("position at L %+d" % shift, r2, L + shift - 20, 0, (270, 330, 480, 520)))
        calls.append(Call("position at L %+d, odd length" % shift, r2, L + shift - 20, 0, (270, 331, 480, 520)))
    calls.append(Call("below zero", read, 0, 0, (100, 160, 480, 520)))
    calls.append(Call("below zero by the offset", read, 200, -300, (100, 160, 480, 520)))
    calls.append(Call("just above zero", read, 200, -49, (100, 160, 480, 520)))      # position 1
    calls.append(Call("position zero", read, 200, -50, (100, 160, 480, 520)))
    return genome, calls


def long_genome(lib):
    """one contig of 120 000 bases and the two calls whose windows have 99 998 and 99 999 characters"""
    from ngmlr_amd import aligner
    rng = np.random.default_rng(808)
    c = synth.random_ref(rng, 120000).tobytes()
    genome = aligner.encode_genome(lib, [c])
    s0 = int(genome[2][0])
    read = _read_over(rng, c, 50000, 600)
    # position = P + O + 49 750 - 250 - 49 750 = P + O - 250; len = 99 998: that many characters from an even position, one more from an odd one
    P = s0 + 1000 + (s0 & 1)
    calls = [Call("99 998 characters", read, P, 250, (0, 99500, 290, 310)), Call("99 999 characters", read, P, 251, (0, 99500, 290, 310)),
             Call("99 996 characters", read, P, 250, (0, 99498, 290, 310))]
    return genome, calls


# --------------------------------------------------------------------------- the recorded calls

def read_fasta(path):
    op = gzip.open if path.endswith(".gz") else open
    seqs, cur = [], None
    with op(path, "rt") as f:
        for line in f:
            line = line.strip()
            if line.startswith(">"):
                cur = []
                seqs.append(cur)
            elif cur is not None:
                cur.append(line)
    return [("".join(s)).encode() for s in seqs]


RECORDED = ("inv_checks_test_3.npz", "inv_checks_split.npz")


def recorded(lib, name):
    """-> (genome, calls, the file): per recorded call a tile of its own whose read holds the 100 recorded characters at the
    place checkForSV took them from (the rest of fullReadSeq never reaches the scorer; its length does), the region (midRef,
    midRef + inversionLength) around the recorded midpoints.  A recorded midpoint is the uloc the reference converted its int to:
    taken back as a signed value."""
    from ngmlr_amd import aligner
    with np.load(os.path.join(GOLDEN, name)) as f:
        z = {k: f[k] for k in f.files}      # (read once: an open file decompresses an array every time it is asked for it)
    if "genome_seed" in z:
        ref = synth.random_ref(np.random.default_rng(int(z["genome_seed"])), int(z["genome_len"])).tobytes()
        assert hashlib.sha1(ref).digest() == z["genome_sha1"].tobytes()
        contigs = [ref]
    else:
        contigs = read_fasta(os.path.join(GOLDEN, "e2e", "test_3_reference.fasta.gz"))
    genome = aligner.encode_genome(lib, contigs)
    calls = []
    for i in range(int(z["n"])):
        H, inv = int(z["read_len"][i]), int(z["inv_len"][i])
        mid_ref, mid_read = int(z["mid_ref"][i].astype(np.int64)), int(z["mid_read"][i].astype(np.int64))
        read = bytearray(b"A" * H)
        if int(z["n_read"][i]):
            read[mid_read - 50:mid_read + 50] = z["read"][i].tobytes()
        # (start, stop) with the recorded midpoint and length: start = mid - inv / 2 rounds the sum back to mid for either parity
        lo = mid_ref - inv // 2
        calls.append(Call("%s call %d" % (name, i), bytes(read), int(z["on_ref_start"][i]) & MASK64, int(z["position_offset"][i]),
                          (lo, lo + inv, mid_read, mid_read)))
        assert cdiv2(lo + lo + inv) == mid_ref or lo + lo + inv < 0
    return genome, calls, z


def recorded_records(z):
    """what the reference computed for the calls of recorded(): status (SCORED where the scoring block ran -- an empty window
    included: the reference cannot tell), both scores"""
    from ngmlr_amd import aligner
    out = np.zeros(int(z["n"]), dtype=aligner.INV_CHECK_DTYPE)
    out["status"] = np.array([{0: SCORED, 1: TOO_SHORT, 2: NO_READ}[int(o)] for o in z["outcome"]], dtype=np.int32)
    out["score_fwd"], out["score_rev"] = z["score_fwd"], z["score_rev"]
    return out
