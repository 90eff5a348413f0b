"""GPU (-m gpu): the plan records the device writes (plan_kernel<256>: row spans staged in LDS strip by strip; plan_kernel<64>:
rows evaluated on demand) against the brute-force restatement of ngmlr_amd/csrc/cvx_plan_logic.h, field for field -- closed
forms handed over as descriptors (evaluated in registers) and the same corridors as row arrays, explicit rows that are
irregular or empty, a 40 000-row tile, in batches whose mean rows per tile lie on either side of the switch between the two
kernels (1 024)."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from ngmlr_amd import capi, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROGRAM = os.path.join(ROOT, "ngmlr_amd", "plan_logic_test")
PLAN_DTYPE = np.dtype([("r0", np.int32), ("rend", np.int32), ("need", np.int32), ("flags", np.int32), ("cells", np.uint64), ("active", np.uint64)])
ROWS_EXPLICIT, ROWS_AFFINE, ROWS_CONST = 1, 2, 3
STRIP, AHEAD = 1536, 511          # kPlanStrip, kPlanAhead


def _tile(rng, H, W, off, ln, desc=None, tag=""):
    return synth.Tile(ref=synth.random_ref(rng, W).tobytes(), qry=synth.random_ref(rng, H).tobytes(), row_offset=np.asarray(off, np.int32),
                      row_length=np.asarray(ln, np.int32), desc=desc, tag=tag)


def _corridors(heights, seed):
    """the families of tests/cpp/plan_logic_test.cpp at the given heights: (tile, closed form or None)"""
    rng = np.random.default_rng(seed)
    out = []
    slopes, widths = (0.5, 0.957, 1.0, 1.045, 2.0), (1, 40, 340, 369, 420, 2048, 8192)
    for i, H in enumerate(heights):
        k, w = slopes[i % 5], widths[(i // 5 + i) % 7]
        W = int(H / k) + 1
        kind = i % 6
        if kind in (0, 1):      # endpoints / anchors, the window a fifth short for every other one: both clips
            Wc = W - W // 5 if (i // 6) % 2 else W
            desc = synth.endpoints_desc(H, max(Wc, 1), w, realign=True) if kind == 0 else (1, float(np.float32(H) / np.float32(max(Wc, 1))), 0.0, float(np.float32(w * 0.55)), 0, w)
            off, ln = synth.affine_rows(H, desc[1], desc[2], desc[3], desc[5])
            out.append((_tile(rng, H, max(Wc, 1), off, ln, desc, "affine"), desc))
            out.append((_tile(rng, H, max(Wc, 1), off, ln, None, "affine as arrays"), None))
        elif kind == 2:
            desc = (2, 0.0, 0.0, 0.0, int(rng.integers(-700, 60)), w)
            out.append((_tile(rng, H, 600, np.full(H, desc[4]), np.full(H, w), desc, "constant"), desc))
        else:
            off, ln = synth.corridor_endpoints(H, W, min(w, 700), realign=True)
            off, ln = off.copy(), ln.copy()
            if kind == 3 and H > 2:
                off[H // 2] -= 3                        # a decreasing row start
                ln[(2 * H) // 3] -= min(5, int(ln[0]))      # a shrinking row end
            elif kind == 4:
                ln[::7] = 0                             # zero-length rows
                off = off + rng.integers(-20, 20, size=H).astype(np.int32)
            else:
                off = off + W + 2 * int(ln[0]) + 10      # entirely right of the window
            out.append((_tile(rng, H, W, off, ln, None, "explicit %d" % kind), None))
    return out


def _brute_force(cases, tmp_path, max_mb=10000):
    """plan records of plan_tile_brute for the corridors as the DEVICE sees them: the closed form where one was handed over, else the rows"""
    blob = [struct.pack("<iQ", len(cases), max_mb)]
    for t, desc in cases:
        if desc is not None:
            kind, k, d, right, off0, width = desc
            blob.append(struct.pack("<5i3f", ROWS_AFFINE if kind == 1 else ROWS_CONST, t.W, t.H, width, off0, k, d, right))
        else:
            blob.append(struct.pack("<5i3f", ROWS_EXPLICIT, t.W, t.H, 0, 0, 0.0, 0.0, 0.0))
            blob.append(np.stack([t.row_offset, t.row_length], axis=1).astype("<i4").tobytes())
    src, dst = tmp_path / "corridors.bin", tmp_path / "plans.bin"
    src.write_bytes(b"".join(blob))
    subprocess.run([PROGRAM, "--plans", str(src), str(dst)], check=True, timeout=120)
    return np.frombuffer(dst.read_bytes(), dtype=PLAN_DTYPE)


def _device_plans(al, cases):
    b = al.upload([t for t, _ in cases], closed_form=True)
    b.run()
    out = np.zeros(len(cases), dtype=PLAN_DTYPE)
    capi.check(al.lib.cvx_batch_plan(b.b, 0, len(cases), out.ctypes.data))
    b.free()
    return out


def _compare(cases, got, want):
    assert len(got) == len(want) == len(cases)
    bad = [(t.tag, t.H, t.W, tuple(g), tuple(w)) for (t, _), g, w in zip(cases, got, want) if tuple(g) != tuple(w)]
    assert not bad, bad[:5]


def test_long_tiles_take_the_strip_form(hip_aligner, tmp_path):
    rng = np.random.default_rng(7)
    edge = [STRIP - 1, STRIP, STRIP + 1, STRIP + AHEAD, STRIP + AHEAD + 1, 2 * STRIP + 3 - 80]      # (<= 3 000 rows)
    heights = edge * 6 + [int(h) for h in rng.integers(1100, 3001, size=108)] + [1, 2, 63, 64, 65, 255, 256, 257] * 2
    cases = _corridors(heights, seed=11)
    tall = synth.endpoints_desc(40000, 40400, 400, realign=True)
    cases.append((_tile(rng, 40000, 40400, *synth.affine_rows(40000, tall[1], tall[2], tall[3], tall[5]), desc=tall, tag="40 000 rows"), tall))
    assert sum(t.H for t, _ in cases) >= 1024 * len(cases) and 150 <= len(cases) <= 320
    want = _brute_force(cases, tmp_path)
    got = _device_plans(hip_aligner, cases)
    _compare(cases, got, want)
    # the workload does what it is for: irregular and empty corridors, searches that leave the staged stretch
    assert (want["flags"] & 1).any() and (want["flags"] & 2).any() and (want["need"] > AHEAD + 1).any()


def test_short_tiles_take_the_on_demand_form(hip_aligner, tmp_path):
    rng = np.random.default_rng(8)
    heights = [1, 2, 63, 64, 65, 255, 256, 257] * 6 + [int(h) for h in rng.integers(3, 900, size=100)]
    cases = _corridors(heights, seed=12)
    assert sum(t.H for t, _ in cases) < 1024 * len(cases)
    want = _brute_force(cases, tmp_path)
    got = _device_plans(hip_aligner, cases)
    _compare(cases, got, want)
    assert (want["flags"] & 1).any() and (want["flags"] & 2).any()
