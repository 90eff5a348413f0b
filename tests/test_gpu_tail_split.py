"""GPU (-m gpu): a whole-tile fill class whose last tiles are filled by a launch of their own on the low-priority stream, the head
walked meanwhile (CVX_TUNE_TAIL_SPLIT=N, build_schedule / stage_compute).  Only the grouping of launches and their streams change:
every case runs on a handle created with the split forced and on one created with it off, and the result records and the ops of
the two must be equal byte for byte; a sample of the tiles is compared with the CPU oracle as well.  The shapes are the smallest
at which the schedule can go wrong: one M = 3 class of 96 tiles under tails of 1, 16 and 95; a mixed batch (three ring classes,
chained tiles, the catch-all kernel, skipped tiles); tiles the exact pass redoes in head and tail; a direct-exact prefix; the
streaming and the resident entry point; the launch records."""
import re

import numpy as np
import pytest

from oracle.pyoracle import same_alignment
from ngmlr_amd import synth

pytestmark = pytest.mark.gpu

MAX_MATRIX_MB = 4          # (the mixed batch holds a tile beyond it)


def _early_best(rng, W, tag):
    """a read whose alignment ends long before the read does (a clean prefix, then junk): a local alignment with its best cell
    in the first 30-60 % of the anti-diagonals"""
    ref = synth.random_ref(rng, W)
    good = int(W * float(rng.uniform(0.3, 0.6)))
    qry = np.concatenate([synth.mutate(rng, ref[:good], 0.1), synth.random_ref(rng, W - good)])
    off, ln = synth.corridor_anchors(len(qry), W)
    return synth.Tile(ref.tobytes(), qry.tobytes(), off, ln, tag=tag)


def _one_class():
    """96 tiles of 300-700 read bases under the anchors corridor without scatter (309 columns: one M = 3 class).  A third of them
    are local alignments with an early best cell, the largest and the smallest tile of the batch among them: whatever the tail
    size, head and tail both hold a tile the exact pass has to redo under a one-group exactly tracked end."""
    rng = np.random.default_rng(1601)
    tiles = []
    for i in range(96):
        if i % 3 == 1:
            W = 300 if i == 1 else 700 if i == 4 else int(rng.integers(360, 640))
            tiles.append(_early_best(rng, W, "early%d" % i))
        else:
            tiles.append(synth.make_tile(rng, int(rng.integers(360, 640)), corridor="anchors", tag="whole%d" % i))
    return tiles


def _mixed():
    """~200 tiles: corridors of 200 / 340 / 420 columns (M = 2, 3, 4), two wide tiles that are chained, one with irregular row starts
    for the catch-all kernel, and tiles that are never filled -- a corridor outside its window, a matrix beyond the handle's cap --
    scattered through the batch, the last tiles included"""
    rng = np.random.default_rng(1602)
    tiles = []
    for i in range(192):
        W = int(rng.integers(300, 700))
        ref = synth.random_ref(rng, W)
        qry = synth.mutate(rng, ref, 0.12)
        off, ln = synth.corridor_endpoints(len(qry), W, (200, 340, 420)[i % 3], realign=True)
        tiles.append(synth.Tile(ref.tobytes(), qry.tobytes(), off, ln, tag="m%d-%d" % (2 + i % 3, i)))
    for k in range(2):
        tiles.insert(40 + 90 * k, synth.make_tile(rng, 2500, err=0.18, ratio=(4, 4, 2), corridor="endpoints", width=1400, realign=True, tag="chained%d" % k))
    W = 500
    ref = synth.random_ref(rng, W)
    qry = synth.mutate(rng, ref, 0.12)
    base, ln = synth.corridor_anchors(len(qry), W)
    tiles.insert(77, synth.Tile(ref.tobytes(), qry.tobytes(), (base + rng.integers(-40, 40, size=len(qry))).astype(np.int32), ln, tag="irregular"))
    for at in (3, 120, len(tiles)):
        r = synth.random_ref(rng, 400)
        tiles.insert(at, synth.Tile(r.tobytes(), r[:380].tobytes(), np.full(380, 450, np.int32), np.full(380, 20, np.int32), tag="empty"))
    for at in (9, len(tiles)):
        r = synth.random_ref(rng, 6200)
        tiles.insert(at, synth.Tile(r.tobytes(), r[:6000].tobytes(), *synth.corridor_endpoints(6000, 6200, 700, realign=True), tag="too-large"))
    return tiles


def _steps(t):
    """first and one-past-last anti-diagonal of the tile's corridor inside its window"""
    H, W = len(t.qry), len(t.ref)
    y = np.arange(H, dtype=np.int64)
    lo = np.maximum(np.asarray(t.row_offset, np.int64), 0)
    hi = np.minimum(np.asarray(t.row_offset, np.int64) + np.asarray(t.row_length, np.int64), W)
    live = hi > lo
    return int((lo + y)[live].min()), int((hi + y)[live].max())


class _Pair:
    """the same environment twice: a handle with the split forced to N tiles and one with it off"""

    def __init__(self, monkeypatch, n, env=None):
        from ngmlr_amd.aligner import ConvexAlignHip
        for k, v in (env or {}).items():
            monkeypatch.setenv(k, v)
        monkeypatch.setenv("CVX_TUNE_TAIL_TRACE", "1")
        monkeypatch.setenv("CVX_TUNE_TAIL_SPLIT", str(n))
        self.split = ConvexAlignHip(device=0, max_matrix_mb=MAX_MATRIX_MB)
        monkeypatch.setenv("CVX_TUNE_TAIL_SPLIT", "0")
        self.plain = ConvexAlignHip(device=0, max_matrix_mb=MAX_MATRIX_MB)

    def close(self):
        self.split.close()
        self.plain.close()


def _run(al, tiles, runs=1):
    """the resident path: -> (record bytes, ops, timing, launch records, alignments) of the last of `runs` runs"""
    batch = al.upload(tiles)
    try:
        for _ in range(runs):
            tm = batch.run()
        res, ops = batch.download()
        return bytes(res)[:len(tiles) * 48], ops.copy(), tm, batch.launches(), batch.alignments()
    finally:
        batch.free()


def _split_lines(capfd):
    """the launches the library reports as split (CVX_TUNE_TAIL_TRACE: one stderr line per split launch of a finished batch)"""
    return [(int(m.group(1)), int(m.group(2)), int(m.group(3)))
            for m in re.finditer(r"cvx tail split: launch \d+ m=(\d+) tiles=(\d+) tail=(\d+)", capfd.readouterr().err)]


def _same_records(a, b):
    """launch records field by field, the event-timed `ms` aside"""
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert {k: v for k, v in x.items() if k != "ms"} == {k: v for k, v in y.items() if k != "ms"}


def _against_oracle(port_oracle, tiles, got, every):
    bad = []
    n_valid = 0
    for t, g in list(zip(tiles, got))[::every]:
        if t.tag in ("empty", "too-large"):
            continue
        want = port_oracle.align(t)
        d = same_alignment(want, g)
        if d is None:
            fs = port_oracle.last_fill_score_bits()      # the raw fill result, valid alignment or not
            if fs != 0xBF800000 and fs != g["fwd_score_bits"]:
                d = "raw fill score %08x vs %08x" % (g["fwd_score_bits"], fs)
        n_valid += want["ret"] >= 0
        if d:
            bad.append((t.tag, d))
    assert not bad, bad[:5]
    assert n_valid > 0


@pytest.fixture(scope="module")
def one_class():
    return _one_class()


@pytest.mark.parametrize("n", [1, 16, 95])
def test_one_class(built, port_oracle, monkeypatch, capfd, one_class, n):
    """one M = 3 class of 96 tiles: a tail of one tile, of a sixth of the class, of all but one tile"""
    p = _Pair(monkeypatch, n)
    capfd.readouterr()
    rec1, ops1, tm1, l1, got = _run(p.split, one_class)
    assert _split_lines(capfd) == [(3, 96, n)]
    rec0, ops0, tm0, l0, _ = _run(p.plain, one_class)
    assert _split_lines(capfd) == []
    p.close()
    assert rec1 == rec0 and np.array_equal(ops1, ops0)
    # one record per class, the unsplit launch's
    assert len(l1) == 1 and l1[0]["slots_per_lane"] == 3 and l1[0]["n_tiles"] == 96 and l1[0]["waves"] == 1
    _same_records(l1, l0)
    assert l1[0]["ms"] > 0 and tm1.fill_ms >= l1[0]["ms"] * 0.99 and tm1.backtrack_ms >= 0
    _against_oracle(port_oracle, one_class, got, every=5)


def test_mixed_batch(built, port_oracle, monkeypatch, capfd):
    """three ring classes of 64 tiles each split at 8; the chained class, the catch-all launch and the skipped tiles are nobody's tail"""
    tiles = _mixed()
    p = _Pair(monkeypatch, 8)
    capfd.readouterr()
    rec1, ops1, tm1, l1, got = _run(p.split, tiles)
    split = _split_lines(capfd)
    rec0, ops0, tm0, l0, _ = _run(p.plain, tiles)
    p.close()
    assert sorted(split) == [(2, 64, 8), (3, 64, 8), (4, 64, 8)], split
    assert rec1 == rec0 and np.array_equal(ops1, ops0)
    _same_records(l1, l0)
    kinds = sorted((li["kind"], li["slots_per_lane"], li["n_tiles"]) for li in l1)
    assert kinds == [(0, 2, 64), (0, 3, 64), (0, 4, 64), (2, 1, 2), (3, 0, 1)], kinds      # whole x 3, chained, catch-all
    status = {t.tag: g["status"] for t, g in zip(tiles, got)}
    assert status["empty"] == 5 and status["too-large"] == 4
    assert tm1.n_tiles_chained == 2 and tm1.n_tiles_fast == 192
    _against_oracle(port_oracle, tiles, got, every=7)
    _against_oracle(port_oracle, [t for t in tiles if t.tag.startswith(("chained", "irregular"))],
                    [g for t, g in zip(tiles, got) if t.tag.startswith(("chained", "irregular"))], every=1)


@pytest.mark.parametrize("n", [1, 16, 95])
def test_exact_pass_in_head_and_tail(built, port_oracle, monkeypatch, capfd, one_class, n):
    """a one-group exactly tracked end (CVX_TUNE_LATE_MIN=1, CVX_TUNE_LATE_SHIFT=16): every tile whose best cell lies before its
    last group of four steps is flagged by the two-phase pass and redone by the exact pass -- the head's pass over the head, the
    tail's over the tail"""
    # the rule as the two-phase fill applies it (cvx_fill_ring.inc): ngroups = ceil(nsteps / 4), the last max(late_min, ngroups >> shift)
    # groups are tracked exactly, and a tile whose best cell lies before them is flagged.  The engineered tiles, on the CPU:
    early = [t for t in one_class if t.tag.startswith("early")]
    sizes = sorted(len(t.qry) for t in one_class)
    assert len(early) == 32 and min(len(t.qry) for t in early) == sizes[0] < sizes[1] - 20 and max(len(t.qry) for t in early) == sizes[-1] > sizes[-2] + 20
    for t in early:
        port_oracle.align(t)
        f = port_oracle.last_fwd()
        r0, rend = _steps(t)
        ngroups = (rend - r0 + 3) // 4
        assert port_oracle.last_fill_score_bits() != 0xBF800000 and f["best_x"] + f["best_y"] - r0 < 4 * (ngroups - 1) - 64, t.tag
    p = _Pair(monkeypatch, n, {"CVX_TUNE_LATE_MIN": "1", "CVX_TUNE_LATE_SHIFT": "16"})
    capfd.readouterr()
    rec1, ops1, tm1, l1, got = _run(p.split, one_class)
    assert _split_lines(capfd) == [(3, 96, n)]
    rec0, ops0, tm0, l0, _ = _run(p.plain, one_class)
    p.close()
    assert tm1.n_tiles_redone > 0
    assert tm1.n_tiles_redone >= len(early) and tm1.n_tiles_redone == tm0.n_tiles_redone
    assert rec1 == rec0 and np.array_equal(ops1, ops0)
    _against_oracle(port_oracle, one_class, got, every=1 if n == 16 else 9)


@pytest.mark.parametrize("n", [16, 90])
def test_direct_exact_prefix(built, monkeypatch, capfd, one_class, n):
    """CVX_TUNE_EXACT_STEPS=1200: the tiles of 1 200 steps and more go straight to the exact fill, in front of the head; a tail that
    would leave the head no two-phase tile (90 of 96 tiles, about eleven of them in the prefix) is no tail"""
    steps = [_steps(t)[1] - _steps(t)[0] for t in one_class]
    lo, hi = sum(1 for k in steps if k >= 1210), sum(1 for k in steps if k >= 1190)      # (whatever the plan makes of a tile at the threshold)
    assert 8 <= lo <= hi <= 20 and 16 < 96 - hi and 90 >= 96 - lo, (lo, hi)
    p = _Pair(monkeypatch, n, {"CVX_TUNE_EXACT_STEPS": "1200"})
    capfd.readouterr()
    rec1, ops1, tm1, l1, _ = _run(p.split, one_class)
    assert _split_lines(capfd) == ([(3, 96, 16)] if n == 16 else [])
    rec0, ops0, tm0, l0, _ = _run(p.plain, one_class)
    p.close()
    assert tm1.n_tiles_redone >= lo and tm1.n_tiles_redone == tm0.n_tiles_redone
    assert rec1 == rec0 and np.array_equal(ops1, ops0)
    _same_records(l1, l0)


def test_streaming_three_jobs_in_flight(built, monkeypatch, capfd, one_class):
    """cvx_submit x 3, then cvx_wait x 3: the tails of the three jobs share the low-priority stream"""
    mixed = _mixed()
    batches = [one_class, mixed, one_class[::-1]]
    p = _Pair(monkeypatch, 8)
    capfd.readouterr()
    out = []
    for al in (p.split, p.plain):
        jobs = [al.submit(b) for b in batches]
        got = []
        for j in jobs:
            res, ops = j.wait()
            got.append((res.tobytes(), ops.copy(), j.launches()))
        for j in jobs:
            j.release()
        out.append(got)
        if al is p.split:
            assert sorted(_split_lines(capfd)) == [(2, 64, 8), (3, 64, 8), (3, 96, 8), (3, 96, 8), (4, 64, 8)]
    p.close()
    for (r1, o1, l1), (r0, o0, l0) in zip(*out):
        assert r1 == r0 and np.array_equal(o1, o0)
        _same_records(l1, l0)


def test_resident_batch_run_twice(built, monkeypatch, capfd, one_class):
    """cvx_batch_run twice on one uploaded batch: the second run's events, counters and results are the first's"""
    p = _Pair(monkeypatch, 16)
    capfd.readouterr()
    rec2, ops2, tm2, l2, _ = _run(p.split, one_class, runs=2)
    assert _split_lines(capfd) == [(3, 96, 16)] * 2
    rec1, ops1, tm1, l1, _ = _run(p.split, one_class)
    rec0, ops0, tm0, l0, _ = _run(p.plain, one_class)
    p.close()
    assert rec2 == rec1 == rec0 and np.array_equal(ops2, ops0) and np.array_equal(ops1, ops0)
    assert tm2.n_tiles_redone == tm0.n_tiles_redone
    _same_records(l2, l0)
