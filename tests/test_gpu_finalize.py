"""GPU (-m gpu): the device-side finalize stage (cvx_kernels.hip: per-block sums, their scan, result records) over batch
sizes on both sides of its 256-tile block and of the 256-block chunk of the scan -- every tile's slice of the dense ops arena
is the exclusive prefix sum of the valid tiles' op counts, the summary agrees with the records, the ops behind ops_begin are
the tile's own, and a batch that is run again reports the same records and a redo count that does not add up."""
import ctypes as C

import numpy as np
import pytest

from ngmlr_amd import capi, synth
from ngmlr_amd.aligner import RESULT_DTYPE, ConvexAlignHip

pytestmark = pytest.mark.gpu

SIZES = (1, 255, 256, 257, 4097, 20000)
POOL = 56                 # distinct tiles; tile i of a batch is pool[i % POOL] unless i % 7 == 0 (an empty corridor)


def _pool():
    rng = np.random.default_rng(1307)
    tiles = []
    for k in range(POOL):
        W = int(rng.integers(30, 61))
        if k % 8 == 3:      # no positive score anywhere: nothing to walk
            tiles.append(synth.Tile(b"A" * W, b"C" * W, *synth.corridor_linear(W, 30), tag="mismatch%d" % k))
        else:
            tiles.append(synth.make_tile(rng, W, err=0.1, corridor="linear", width=64, tag="fin%d" % k))
    return tiles


def _empty_tile():
    """every row lies right of the window: no cell inside [0, W) (CVX_TILE_EMPTY)"""
    H, W = 40, 45
    return synth.Tile(b"A" * W, b"A" * H, np.full(H, W + 10, np.int32), np.full(H, 20, np.int32), tag="empty")


def _records(batch, n):
    res, ops = batch.download()
    rec = np.frombuffer(bytes(memoryview(res)), dtype=RESULT_DTYPE)[:n].copy()
    return rec, ops.copy()


def _summary(al, batch):
    total, valid, redone = C.c_uint64(), C.c_int32(), C.c_int32()
    capi.check(al.lib.cvx_batch_summary(batch.b, C.byref(total), C.byref(valid), C.byref(redone)))
    return int(total.value), int(valid.value), int(redone.value)


@pytest.fixture(scope="module")
def solo(hip_aligner):
    """(status, ops) of every pool tile and of the empty tile, each from a batch of its own"""
    out = []
    for t in _pool() + [_empty_tile()]:
        b = hip_aligner.upload([t])
        b.run()
        rec, ops = _records(b, 1)
        b.free()
        n = int(rec["n_ops"][0])
        assert rec["ops_begin"][0] == 0
        out.append((int(rec["status"][0]), ops[:n].copy()))
    return out


def _batch(n):
    pool, empty = _pool(), _empty_tile()
    idx = [POOL if i % 7 == 0 else i % POOL for i in range(n)]
    return [empty if k == POOL else pool[k] for k in idx], idx


@pytest.mark.parametrize("n", SIZES)
def test_prefix_sums_and_summary(hip_aligner, solo, n):
    tiles, idx = _batch(n)
    b = hip_aligner.upload(tiles)
    b.run()
    rec, ops = _records(b, n)
    total, n_valid, _ = _summary(hip_aligner, b)
    b.free()
    status = np.array([solo[k][0] for k in idx])
    n_ops = np.array([len(solo[k][1]) if solo[k][0] == 0 else 0 for k in idx], dtype=np.uint64)
    assert np.array_equal(rec["status"], status)
    assert np.array_equal(rec["n_ops"].astype(np.uint64), n_ops)          # (invalid tiles report 0)
    begin = np.concatenate([[0], np.cumsum(n_ops)[:-1]]).astype(np.uint64)
    assert np.array_equal(rec["ops_begin"], begin)
    assert total == int(n_ops.sum()) and n_valid == int((status == 0).sum())
    if n > 7:
        assert (status == 5).sum() == (n + 6) // 7 and (n_ops == 0).sum() > (n + 6) // 7      # the workload does what it is for
    for i in range(n):
        k = idx[i]
        if status[i] == 0:
            assert np.array_equal(ops[int(begin[i]):int(begin[i]) + int(n_ops[i])], solo[k][1]), i


def test_second_run_of_a_batch(built, monkeypatch):
    """the counters the summary reads are zeroed behind their last reader: the redo count of a second run is that run's own"""
    monkeypatch.setenv("CVX_TUNE_LATE_MIN", "1")      # a one-group exactly tracked tail: most tiles take the second fill pass
    al = ConvexAlignHip(device=0)
    tiles, _ = _batch(4097)
    b = al.upload(tiles)
    t1 = b.run()
    rec1, ops1 = _records(b, len(tiles))
    s1 = _summary(al, b)
    t2 = b.run()
    rec2, ops2 = _records(b, len(tiles))
    s2 = _summary(al, b)
    b.free()
    al.close()
    assert rec1.tobytes() == rec2.tobytes() and np.array_equal(ops1, ops2)
    assert s1 == s2 and s1[2] > 0
    assert t1.n_tiles_redone == t2.n_tiles_redone == s1[2]
