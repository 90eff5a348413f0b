#!/usr/bin/env python3
"""tools/pack_golden_twin.py TWIN_SO FAST_SO OUT_DIR -- record the scalar twin's fixtures (tools/make_golden_twin.sh).

Generates seeded tiles (40-600 read bases) family by family, runs the reference's own Convex::ConvexAlign (TWIN_SO, built from
tools/ref_recorder/twin_wrap.cpp) and its Convex::ConvexAlignFast (FAST_SO, oracle/_ref/libcvx_oracle_ref.so) on each, and
writes data only:

    OUT_DIR/twin_xfree.npz   tiles without an 'x' in the window, the default scoring and three scorings outside the fast regime
    OUT_DIR/twin_x.npz       tiles with 'x' in the window (default scoring), one family per way an 'x' can meet the kernels

Per tile i: t{i}_ref / qry / off / len (inputs), t{i}_meta = (ext_qstart, ext_qend), and for both aligners (prefix w = twin,
f = fast) {p}{i}_ret_fields, {p}{i}_bits (score, identity), {p}{i}_cigar, {p}{i}_md, {p}{i}_nm; plus family[i], params[i].

The families are checked here, not tuned to any implementation: at least 75 % of every family valid under the twin, at least a
fifth of the x-bearing tiles different between the two aligners (tests/test_twin_fixtures_cpu.py checks the same on the file).
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ngmlr_amd import synth                      # noqa: E402
from oracle.pyoracle import OracleOut, DEFAULT_PARAMS    # noqa: E402

FIELDS = ("ret", "position_offset", "qstart", "qend", "nm", "alignment_length", "cigar_op_count", "sv_type",
          "first_ref", "first_read", "last_ref", "last_read")
EXOTIC = ((2.0, -10.0, -5.0, -5.0, -1.0, 0.15), (1.0, -4.0, -2.0, -2.0, -1.0, 0.05), (3.0, -2.0, -1.0, -4.0, -0.5, 0.3))
X = ord("x")


class Recorder:
    """One aligner of either library through oracle/oracle_abi.h."""

    def __init__(self, path, params):
        self.lib = C.CDLL(path)
        self.lib.oracle_create.restype = C.c_void_p
        self.lib.oracle_create.argtypes = [C.POINTER(C.c_float)]
        self.lib.oracle_destroy.argtypes = [C.c_void_p]
        self.lib.oracle_kind.restype = C.c_char_p
        self.lib.oracle_align.restype = C.c_int
        self.lib.oracle_align.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                          C.POINTER(OracleOut), C.c_char_p, C.c_char_p, C.c_int32, C.c_void_p, C.c_int32]
        self.kind = self.lib.oracle_kind().decode()
        self.h = C.c_void_p(self.lib.oracle_create((C.c_float * 6)(*params)))

    def align(self, t):
        H = len(t.qry)
        off = np.ascontiguousarray(t.row_offset, dtype=np.int32)
        ln = np.ascontiguousarray(t.row_length, dtype=np.int32)
        cap = 4 * H + 4 * len(t.ref) + 256
        cig, md = C.create_string_buffer(cap), C.create_string_buffer(cap)
        nm_cap = 2 * (H + 1) + len(t.ref) + 16
        nm = np.zeros((nm_cap, 3), dtype=np.int32)
        out = OracleOut()
        rc = self.lib.oracle_align(self.h, t.ref, t.qry, off.ctypes.data, ln.ctypes.data, H, t.ext_qstart, t.ext_qend,
                                   C.byref(out), cig, md, cap, nm.ctypes.data, nm_cap)
        assert rc == 0, "the reference threw on %s" % t.tag
        d = {k: getattr(out, k) for k, _ in OracleOut._fields_}
        d["score_bits"] = int(np.float32(out.score).view(np.uint32))
        d["identity_bits"] = int(np.float32(out.identity).view(np.uint32))
        d["cigar"], d["md"] = cig.value.decode(), md.value.decode()
        d["nm_per_position"] = nm[:out.nm_count].copy()
        return d

    def close(self):
        self.lib.oracle_destroy(self.h)


def with_ref(t, ref, qry=None, tag=None):
    return synth.Tile(ref=bytes(ref), qry=bytes(qry) if qry is not None else t.qry, row_offset=t.row_offset, row_length=t.row_length,
                      ext_qstart=t.ext_qstart, ext_qend=t.ext_qend, tag=tag or t.tag)


def base_tile(rng, i, lo=40, hi=600, kinds=("anchors", "endpoints", "linear", "full")):
    kind = kinds[i % len(kinds)]
    while True:
        W = int(rng.integers(lo, hi))
        t = synth.make_tile(rng, W, err=float(rng.choice([0.02, 0.1, 0.15, 0.25])), ratio=[(6, 3, 1), (4, 4, 2), (1, 1, 1)][i % 3],
                            corridor=kind, scatter=float(rng.choice([0, 30])), realign=bool(i % 2))
        if lo <= t.H <= hi:
            return t


def families_x(rng):
    fam = []
    # x prefix and suffix runs: the four phases of a per-dword reference fetch (1, 3, 4, 5) and the lane boundary (63, 64, 65)
    for k, run in enumerate((1, 3, 4, 5, 63, 64, 65)):
        for where in ("prefix", "suffix", "both"):
            t = base_tile(rng, k, lo=200)
            r = bytearray(t.ref)
            if where in ("prefix", "both"):
                r[:run] = b"x" * run
            if where in ("suffix", "both"):
                r[len(r) - run:] = b"x" * run
            fam.append(("x_runs", with_ref(t, r, tag="x-%s-%d" % (where, run))))
    # a window that is all x: against reads that carry x themselves (x == x is a match) and one that does not
    for k, frac in enumerate((1.0, 1.0, 0.95, 0.0)):
        t = base_tile(rng, k, lo=100, hi=400, kinds=("linear", "anchors"))
        q = np.frombuffer(t.qry, dtype=np.uint8).copy()
        q[rng.random(len(q)) < frac] = X
        fam.append(("all_x", with_ref(t, b"x" * t.W, q.tobytes(), tag="all-x-%g" % frac)))
    # 5 % scattered x
    for k in range(24):
        t = base_tile(rng, k)
        r = np.frombuffer(t.ref, dtype=np.uint8).copy()
        r[rng.random(len(r)) < 0.05] = X
        fam.append(("scatter", with_ref(t, r.tobytes(), tag="scatter-%d" % k)))
    # x in the read opposite x in the reference: an error-free read, the same positions in both
    for k in range(6):
        t = base_tile(rng, k)
        r = np.frombuffer(t.ref, dtype=np.uint8).copy()
        m = rng.random(len(r)) < 0.04
        r[m] = X
        lin = synth.corridor_linear(len(r), 120)
        q = r.copy()
        q[rng.integers(0, len(q), size=3)] = ord("A")      # a few of them face a base after all
        fam.append(("x_vs_x", synth.Tile(r.tobytes(), q.tobytes(), lin[0], lin[1], tag="x-vs-x-%d" % k)))
    # upper-case X is an ordinary character (in the window, and in both)
    for k in range(6):
        t = base_tile(rng, k)
        r = np.frombuffer(t.ref, dtype=np.uint8).copy()
        r[rng.random(len(r)) < 0.05] = ord("X")
        q = np.frombuffer(t.qry, dtype=np.uint8).copy()
        if k % 2:
            q[rng.random(len(q)) < 0.03] = ord("X")
        fam.append(("upper_X", with_ref(t, r.tobytes(), q.tobytes(), tag="upper-X-%d" % k)))
    # an x in the corridor's first and last column (of several rows), and some on the path
    for k in range(6):
        t = base_tile(rng, k, lo=150, kinds=("linear", "endpoints", "anchors"))
        r = np.frombuffer(t.ref, dtype=np.uint8).copy()
        for y in rng.integers(0, t.H, size=12):
            for x in (int(t.row_offset[y]), int(t.row_offset[y]) + int(t.row_length[y]) - 1):
                if 0 <= x < len(r):
                    r[x] = X
        r[rng.random(len(r)) < 0.01] = X
        fam.append(("corridor_edge", with_ref(t, r.tobytes(), tag="edge-%d" % k)))
    # a corridor wider than 256 live rows (chained row blocks): full matrices of 300 x 300 and thereabouts
    for k, W in enumerate((300, 300, 330, 280)):
        ref = synth.random_ref(rng, W)
        qry = synth.mutate(rng, ref, 0.1)
        r = ref.copy()
        r[rng.random(W) < 0.04] = X
        if k == 1:
            r[:5] = X
            r[W - 65:] = X
        off, ln = synth.corridor_full(len(qry), W)
        fam.append(("chained", synth.Tile(r.tobytes(), qry.tobytes(), off, ln, tag="full-%d" % W)))
    # an irregular corridor (row starts that move back: the catch-all kernel)
    for k in range(4):
        t = base_tile(rng, k, lo=150, kinds=("linear",))
        r = np.frombuffer(t.ref, dtype=np.uint8).copy()
        r[rng.random(len(r)) < 0.04] = X
        off = t.row_offset.copy()
        off[1::7] -= 9
        off[3::11] += 6
        fam.append(("irregular", synth.Tile(r.tobytes(), t.qry, off.astype(np.int32), t.row_length, tag="irregular-%d" % k)))
    return fam


def pack(path, entries, twin_so, fast_so):
    """entries: (family, params, Tile)"""
    z = {"n": np.int64(len(entries)), "family": np.array([e[0] for e in entries]), "params": np.array([e[1] for e in entries], dtype=np.float32)}
    rec = {}
    stats = {}
    for i, (family, params, t) in enumerate(entries):
        key = tuple(params)
        if key not in rec:
            rec[key] = (Recorder(twin_so, params), Recorder(fast_so, params))
            assert rec[key][0].kind == "twin" and rec[key][1].kind == "reference"
        z["t%d_ref" % i] = np.frombuffer(t.ref, dtype=np.uint8)
        z["t%d_qry" % i] = np.frombuffer(t.qry, dtype=np.uint8)
        z["t%d_off" % i] = t.row_offset.astype(np.int32)
        z["t%d_len" % i] = t.row_length.astype(np.int32)
        z["t%d_meta" % i] = np.array([t.ext_qstart, t.ext_qend], dtype=np.int32)
        z["t%d_tag" % i] = np.array(t.tag)
        outs = []
        for p, r in zip("wf", rec[key]):
            d = r.align(t)
            outs.append(d)
            z["%s%d_fields" % (p, i)] = np.array([d[k] for k in FIELDS], dtype=np.int32)
            z["%s%d_bits" % (p, i)] = np.array([d["score_bits"], d["identity_bits"]], dtype=np.uint32)
            z["%s%d_cigar" % (p, i)] = np.frombuffer(d["cigar"].encode(), dtype=np.uint8)
            z["%s%d_md" % (p, i)] = np.frombuffer(d["md"].encode(), dtype=np.uint8)
            z["%s%d_nm" % (p, i)] = d["nm_per_position"].astype(np.int32)
        w, f = outs
        differs = (w["ret"] < 0) != (f["ret"] < 0) or (w["ret"] >= 0 and any(w[k] != f[k] for k in ("score_bits", "cigar", "md", "position_offset", "qstart", "qend")))
        s = stats.setdefault(family, [0, 0, 0])
        s[0] += 1
        s[1] += w["ret"] >= 0
        s[2] += bool(differs)
    for a, b in rec.values():
        a.close()
        b.close()
    np.savez_compressed(path, **z)
    print("%s: %d tiles, %d bytes" % (path, len(entries), os.path.getsize(path)))
    for fam_, (n, valid, diff) in stats.items():
        print("  %-14s %3d tiles, %3d valid under the twin, %3d differ from ConvexAlignFast" % (fam_, n, valid, diff))
        assert valid >= 0.75 * n, "family %s: regenerate with other seeds" % fam_
    return stats


def main():
    twin_so, fast_so, out = sys.argv[1:4]
    rng = np.random.default_rng(20261)
    xfree = [("xfree_default", DEFAULT_PARAMS, base_tile(rng, i)) for i in range(32)]
    for s, params in enumerate(EXOTIC):
        xfree += [("xfree_scoring%d" % (s + 1), params, base_tile(rng, i)) for i in range(16)]
    pack(os.path.join(out, "twin_xfree.npz"), xfree, twin_so, fast_so)
    stats = pack(os.path.join(out, "twin_x.npz"), [(f, DEFAULT_PARAMS, t) for f, t in families_x(np.random.default_rng(20262))], twin_so, fast_so)
    n = sum(v[0] for v in stats.values())
    diff = sum(v[2] for v in stats.values())
    print("x-bearing tiles: %d, twin != fast on %d" % (n, diff))
    assert 5 * diff >= n, "fewer than a fifth of the x-bearing tiles differ: regenerate with other seeds"


if __name__ == "__main__":
    main()
