"""Deterministic case families for the sub-read scoring kernels (score_diag_kernel, score_wave_kernel<1..16>, score_reg_kernel<5|8>,
score_kernel): gaps that pay at every row phase of a lane, best paths that end in the matrix's last row and column, the class
boundaries, the alphabet, the length limit, and a seeded volume set shaped for cvx_score_submit's per-pair dispatch.

A plain module (no fixtures, no device): tests/test_score_cases_cpu.py pins the families' properties on the CPU oracles,
tests/test_gpu_score_edges.py sends them through the device, tools/fuzz_score.py --submit draws family (h) with fresh seeds.

Every family returns (refs, qrys, meta): bytes without a NUL (the kernels see one more character, the NUL), and one dict per pair.
Every case is emitted in both orientations, next to each other: pair 2i has the long string as `ref`, pair 2i + 1 as `qry`.
meta keys: family, base (index of the unordered pair), orient ("qry_short" | "ref_short"), cls (expected_class), and where they
apply kind ("h" | "v"), a / b (flank lengths), g (gap bases), j1, floor (a lower bound of the score that only a gapped path
reaches), exact (the score in closed form), group (pairs that must travel in one cvx_score_batch call).

Notation: short = A + B, long = J1 + A + X + B + J2 is a horizontal gap (|X| = g columns of the long string without a row);
short = A + X + B, long = J1 + A + B + J2 a vertical one.
"""
import numpy as np

from ngmlr_amd import synth

CLASSES = ("diag", "wave1", "wave2", "wave4", "wave8", "wave16", "rows")
WAVE_K = (1, 2, 4, 8, 16)


def expected_class(rl, ql, no_diag=False):
    """The kernel cvx_score_submit picks for a pair of rl reference and ql query characters (NULs included), restated from the
    documented thresholds: the diagonal kernel takes ql <= 512 and rl <= 2048; else a shorter side of up to 64 K characters is
    score_wave_kernel<K> for the smallest K of 1, 2, 4, 8, 16; else score_kernel.  Only ever used to assert that a family lands
    where it was aimed -- never to decide what is compared."""
    if ql <= 512 and rl <= 2048 and not no_diag:
        return "diag"
    s = min(rl, ql)
    for k in WAVE_K:
        if s <= 64 * k:
            return "wave%d" % k
    return "rows"


_CODE = np.full(256, 4, dtype=np.int8)
for _i, _c in enumerate(b"ACGT"):
    _CODE[_c] = _CODE[_c | 0x20] = _i
_CODE[ord("U")] = _CODE[ord("u")] = 0


def ungapped_best(ref, qry):
    """The maximum over all diagonals of the best contiguous run under the +1 / -1 / 0 matrix (Kadane), row by row: what the
    score would be if no gap could ever pay.  A pair pays for a gap iff the oracle's score is larger."""
    a, b = (ref, qry) if len(ref) >= len(qry) else (qry, ref)
    cols = _CODE[np.frombuffer(a, dtype=np.uint8)].astype(np.int32)
    rows = _CODE[np.frombuffer(b, dtype=np.uint8)].astype(np.int32)
    if len(rows) == 0 or len(cols) == 0:
        return 0
    h = np.zeros(len(cols) + 1, dtype=np.int32)       # h[j + 1]: the run ending in (previous row, column j)
    best = 0
    col_zero = cols == 4
    for r in rows:
        s = np.where(cols == r, 1, -1).astype(np.int32)
        if r == 4:
            s[:] = 0
        else:
            s[col_zero] = 0
        h[1:] = np.maximum(h[:-1] + s, 0)
        best = max(best, int(h.max()))
    return best


def _rand(rng, n):
    return synth.random_ref(rng, int(n)).tobytes()


def _emit(out, short, long, **meta):
    refs, qrys, metas = out
    base = len(refs) // 2
    for ref, qry, orient in ((long, short, "qry_short"), (short, long, "ref_short")):
        refs.append(ref)
        qrys.append(qry)
        metas.append(dict(meta, base=base, orient=orient, cls=expected_class(len(ref) + 1, len(qry) + 1)))


def _gap_pair(rng, parts, gaps, kind, j1=300, j2=300):
    """(short, long): the matching pieces `parts` with gaps[i] extra bases between piece i and i + 1 -- in the long string
    (kind "h") or in the short one ("v")."""
    pieces = [_rand(rng, p) for p in parts]
    extra = [_rand(rng, g) for g in gaps]
    with_x = pieces[0] + b"".join(x + p for x, p in zip(extra, pieces[1:]))
    without = b"".join(pieces)
    left, right = _rand(rng, j1), _rand(rng, j2)
    if kind == "h":
        return without, left + with_x + right
    return with_x, left + without + right


def _emit_gap(out, rng, family, parts, gaps, kind, j1=300, j2=300, pays=True):
    short, long = _gap_pair(rng, parts, gaps, kind, j1, j2)
    meta = dict(family=family, kind=kind, a=parts[0], b=parts[1], parts=tuple(parts), g=tuple(gaps), j1=j1)
    if pays:
        meta["floor"] = sum(parts) - 255 * sum(gaps)
    _emit(out, short, long, **meta)


# (a) ---------------------------------------------------------------------------------------------------------------------------

A_SWEEP = list(range(300, 332)) + [335, 336, 337, 511, 512, 513, 639, 640, 641, 720, 721, 722]


def family_a_sweep(seed=101):
    """One-base gaps in score_wave_kernel<16>: flanks (a, 300) and (300, a), horizontal and vertical, a over every row phase
    a mod 16 twice and around 336 / 512 / 640 / 720.  Every pair pays: score >= a + 300 - 255 > the best ungapped run."""
    rng = np.random.default_rng(seed)
    out = ([], [], [])
    for a in A_SWEEP:
        for parts in ((a, 300), (300, a)):
            for kind in "hv":
                _emit_gap(out, rng, "a", parts, (1,), kind)
    return out


def family_a_thin(seed=103):
    """Flanks of 255 .. 257 around one base and the two-base gaps a 1 023-character short side admits: the gapped path ties with
    the best ungapped run or beats it by a point or two, random extensions decide.  Oracle comparison only."""
    rng = np.random.default_rng(seed)
    out = ([], [], [])
    cases = [((a, b), 1, kind) for a in (255, 256, 257) for b in (255, 256, 257) for kind in "hv"]
    cases += [((511, 511), 2, "h"), ((511, 512), 2, "h"), ((512, 511), 2, "h"), ((510, 511), 2, "h"), ((510, 510), 2, "v"), ((511, 510), 2, "v")]
    for parts, g, kind in cases:
        short_chars = sum(parts) + (g if kind == "v" else 0)
        j = 900 if short_chars <= 511 else 300           # a long side above 2 047 characters: a wave kernel, not the diagonal one
        _emit_gap(out, rng, "a_thin", parts, (g,), kind, j1=j, j2=j, pays=False)
    return out


# (b) ---------------------------------------------------------------------------------------------------------------------------

def family_b(seed=107):
    """(400, 400) around one base with 0 .. 64 characters in front: the junction column moves through one whole 64-column chunk
    of the long side's feed."""
    rng = np.random.default_rng(seed)
    out = ([], [], [])
    for j1 in range(65):
        for kind in "hv":
            _emit_gap(out, rng, "b", (400, 400), (1,), kind, j1=j1)
    return out


# (c) ---------------------------------------------------------------------------------------------------------------------------

C_LONG = (2049, 2111, 2112, 2113, 4096)
C_ROWS_LONG = (1025, 1087, 1088, 1089, 2048, 4096)


def _emit_ends(out, rng, family, n, long_chars, **meta):
    piece = _rand(rng, n)
    for where in ("end", "start"):
        junk = _rand(rng, long_chars - n)
        long = junk + piece if where == "end" else piece + junk
        _emit(out, piece, long, family=family, n=n, where=where, exact=n, **meta)


def family_c_wave(seed=109):
    """An exact copy of the short string at the very end (and the very start) of the long one: the best path ends in the last
    real row and the last real column.  The short side has S = 32 K + 1, 64 K - 1 and 64 K characters with its NUL (64 K: no slack
    in the step count beyond the NUL column), S = 1 and 2 for K = 1; the long side 0 and +-1 mod 64.  Score: S - 1 exactly."""
    rng = np.random.default_rng(seed)
    out = ([], [], [])
    for k in WAVE_K:
        for s in ([1, 2] if k == 1 else []) + [32 * k + 1, 64 * k - 1, 64 * k]:
            for long_chars in C_LONG:
                _emit_ends(out, rng, "c", s - 1, long_chars, k=k)
    return out


def family_c_rows(seed=113):
    """The same for score_kernel's class (both sides above 1 024 characters)."""
    rng = np.random.default_rng(seed)
    out = ([], [], [])
    for n in (1024, 1500):
        for long_chars in C_ROWS_LONG:
            if long_chars >= n:
                _emit_ends(out, rng, "c_rows", n, long_chars, k=0)
    return out


C_REG_LONGEST = (320, 321, 512, 513)


def family_c_reg(seed=127):
    """The same for cvx_score_batch's kernels by the call's longest reference (NUL included): 320 -> score_reg_kernel<5>, 321 and
    512 -> <8>, 513 -> score_kernel.  meta["group"]: the pairs of one call; the long side of every pair of a group has the group's
    length, so the longest reference of the call is that length ("qry_short") or at most that length ("ref_short")."""
    rng = np.random.default_rng(seed)
    out = ([], [], [])
    for longest in C_REG_LONGEST:
        for n in (0, 1, 63, 64, 65, 255, 256, 257, 319, longest - 2, longest - 1):
            _emit_ends(out, rng, "c_reg", n, longest - 1, k=0, group=longest)
    return out


# (d) ---------------------------------------------------------------------------------------------------------------------------

D_CASES = (((600, 700), (1,)), ((900, 600), (1,)), ((700, 700), (2,)), ((800, 900), (3,)), ((810, 810), (3,)), ((1100, 1200), (1,)),
           ((1300, 1100), (4,)), ((500, 500, 500), (1, 1)), ((600, 450, 700), (2, 1)))


def family_d(seed=131):
    """Gaps that pay in score_kernel's class: up to four bases, two gaps in one pair, and a one-base gap whose column moves through
    a 64-column chunk carry of that kernel.  The reference string is the columns there, so the orientations differ."""
    rng = np.random.default_rng(seed)
    out = ([], [], [])
    for parts, gaps in D_CASES:
        for kind in "hv":
            _emit_gap(out, rng, "d", parts, gaps, kind)
    for j1 in range(65):
        for kind in "hv":
            _emit_gap(out, rng, "d", (600, 600), (1,), kind, j1=j1)
    return out


# (e) ---------------------------------------------------------------------------------------------------------------------------

E_XY = ((1, 2), (2, 1), (3, 1), (1, 3), (5, 2), (2, 5), (10, 11), (0, 1), (1, 0))
E_AB = ((300, 300), (400, 500), (256, 257))


def family_e(seed=137):
    """An insertion next to a deletion: short = A + Y + B, long = J1 + A + X + B + J2.  (ssw's lazy-F loop forbids exactly this
    adjacency; oracle/score_oracle.c argues that it cannot matter at a gap cost of 255.)"""
    rng = np.random.default_rng(seed)
    out = ([], [], [])
    for a, b in E_AB:
        for x, y in E_XY:
            pa, pb = _rand(rng, a), _rand(rng, b)
            short = pa + _rand(rng, y) + pb
            long = _rand(rng, 300) + pa + _rand(rng, x) + pb + _rand(rng, 300)
            _emit(out, short, long, family="e", a=a, b=b, x=x, y=y)
    return out


# (f) ---------------------------------------------------------------------------------------------------------------------------

def family_f(seed=139):
    """Every byte 1 .. 127 and its other case, against itself and against long ACGT strings, in the diagonal kernel's class, a wave
    class and score_kernel's.  (Bytes >= 128: the reference indexes a 128-entry table with a signed char there and defines
    nothing to match.)"""
    rng = np.random.default_rng(seed)
    every = bytes(range(1, 128))
    out = ([], [], [])
    cases = [(every, every), (every.swapcase(), every), (every * 3, (every * 3).swapcase()), (every, _rand(rng, 300)),
             (every[::-1], every + every.swapcase()),
             (every * 2, _rand(rng, 3000)), (every * 5, _rand(rng, 3000)), (every.swapcase() * 4, every * 20), (every, every * 17),
             (b"acgtuACGTUnNxX-*" * 30, every * 18),
             (every * 9, (every * 9).swapcase()), (every * 9, _rand(rng, 2500)), (every * 9, every.swapcase() * 10)]
    # byte x between perfect 8-base matches, against 'A' (and against x in its other case) in its place: a byte that is wrongly
    # given a base's code adds or takes a point from the run, in a score of several hundred
    def spaced(lo, hi, other):
        return (b"".join(bytes([x]) + b"ACGTACGT" for x in range(lo, hi)),
                b"".join((b"A" if other is None else bytes([x]).swapcase()) + b"ACGTACGT" for x in range(lo, hi)))
    for lo, hi, pad in ((1, 57, 200), (57, 113, 200), (113, 128, 0), (1, 64, 1000), (64, 128, 1000), (1, 128, 1000)):
        for other in (None, "case"):
            short, mid = spaced(lo, hi, other)
            cases.append((short, _rand(rng, pad) + mid + _rand(rng, pad)))
    for short, long in cases:
        _emit(out, short, long, family="f")
    return out


# (g) ---------------------------------------------------------------------------------------------------------------------------

def family_g(seed=149):
    """The length limit in every class: a short side of that class, an exact piece of the long string, against 99 998 characters
    (scored: the piece's length) and 99 999 characters (-1.0: 100 000 with the NUL)."""
    rng = np.random.default_rng(seed)
    big = _rand(rng, 99999)
    out = ([], [], [])
    for k, n in ((1, 50), (2, 100), (4, 200), (8, 450), (16, 1000), (0, 1100)):
        a = int(rng.integers(0, 99998 - n))
        piece = big[a:a + n]
        _emit(out, piece, big[:99998], family="g", k=k, n=n, exact=n)
        _emit(out, piece, big, family="g", k=k, n=n, exact=-1)
    return out


# (h) ---------------------------------------------------------------------------------------------------------------------------

H_ERR = (0.0, 0.002, 0.005, 0.02, 0.1, 0.3)


def family_h(seed=151, n=20000):
    """Seeded random pairs shaped for cvx_score_submit: wave class i mod 5, the short side uniform in that class, the long side of
    2 048 .. 6 000 characters (one pair in seven: below 2 048, where a short query goes to the diagonal kernel), the short side cut
    from the long one and mutated (ins : del : sub = 4 : 4 : 2), 1 % N in one pair of eleven, either string as the reference.
    Not emitted twice: pair i alone decides its orientation."""
    rng = np.random.default_rng(seed)
    refs, qrys, metas = [], [], []
    for i in range(n):
        k = WAVE_K[i % 5]
        s_chars = int(rng.integers(0 if k == 1 else 32 * k, 64 * k))           # S - 1 for S in (32 K, 64 K]
        if rng.integers(0, 7) == 0:
            l_chars = int(rng.integers(max(s_chars, 513), 2048))
        else:
            l_chars = int(rng.integers(2048, 6001))
        long = synth.random_ref(rng, l_chars, n_frac=0.01 if i % 11 == 0 else 0.0)
        err = float(H_ERR[int(rng.integers(0, len(H_ERR)))])
        cut = s_chars + int(s_chars * 0.3) + 8                                  # deletions shorten it: cut more, trim to the class
        a = int(rng.integers(0, max(1, l_chars - cut)))
        short = synth.mutate(rng, long[a:a + cut], err, ratio=(4, 4, 2))[:s_chars]
        long, short = long.tobytes(), short.tobytes()
        ref, qry, orient = (long, short, "qry_short") if rng.integers(0, 2) else (short, long, "ref_short")
        refs.append(ref)
        qrys.append(qry)
        metas.append(dict(family="h", base=i, orient=orient, k=k, err=err, cls=expected_class(len(ref) + 1, len(qry) + 1)))
    return refs, qrys, metas


# -------------------------------------------------------------------------------------------------------------------------------

FAMILIES = {"a": family_a_sweep, "a_thin": family_a_thin, "b": family_b, "c": family_c_wave, "c_rows": family_c_rows,
            "c_reg": family_c_reg, "d": family_d, "e": family_e, "f": family_f, "g": family_g}

# the classes every family is aimed at (family (h): every wave class and the diagonal kernel)
AIMED = {"a": {"wave16"}, "a_thin": {"wave8", "wave16"}, "b": {"wave16"}, "c": {"wave1", "wave2", "wave4", "wave8", "wave16"},
         "c_rows": {"rows"}, "d": {"rows"}, "e": {"wave16"}, "f": {"diag", "wave4", "wave16", "rows"},
         "g": {"wave1", "wave2", "wave4", "wave8", "wave16", "rows"}}

_cache = {}


def family(name):
    """(refs, qrys, meta) of one family, generated once per process."""
    if name not in _cache:
        _cache[name] = family_h() if name == "h" else FAMILIES[name]()
    return _cache[name]


def all_deterministic():
    """Families (a) .. (g) back to back."""
    refs, qrys, metas = [], [], []
    for name in FAMILIES:
        r, q, m = family(name)
        refs += r
        qrys += q
        metas += m
    return refs, qrys, metas


def check_properties(want, refs, qrys, metas):
    """The families' own assertions on oracle scores `want`: the closed form where there is one, and for every pair with a
    floor: score >= floor and score > the best ungapped run (the pair pays for its gap).  No pair is left out.  Returns the
    number of pairs that pay for a gap."""
    paying = 0
    best_of = {}
    for i, m in enumerate(metas):
        if "exact" in m:
            assert want[i] == m["exact"], (m, float(want[i]))
        if "floor" in m:
            key = (m["family"], m["base"])
            if key not in best_of:
                best_of[key] = ungapped_best(refs[i], qrys[i])
            assert want[i] >= m["floor"], (m, float(want[i]))
            assert want[i] > best_of[key], (m, float(want[i]), best_of[key])
            paying += 1
    return paying
