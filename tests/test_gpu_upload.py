"""GPU (-m gpu): the upload stage's copy schedule (build_upload_schedule, cvx_host_logic.h; pinned on the CPU by
tests/cpp/host_logic_test.cpp) as the device sees it: every way a caller's blocks can lie in page-locked memory
(cvx_host_alloc) gives the results of the packed upload, a batch large enough to be packed and copied in pieces gives
the results of the same tiles in batches that are not, and reads pinned under device-decoded reference windows change
nothing."""
import os

import numpy as np
import pytest

from ngmlr_amd import synth
from tests import util

pytestmark = pytest.mark.gpu


def _pack_thread_bytes():
    """kPackThreadBytes as the library's source has it: at or above this much host packing a batch travels in kUploadPieces pieces."""
    import re
    src = open(os.path.join(os.path.dirname(util.GOLDEN), os.pardir, "ngmlr_amd", "csrc", "cvx_host_logic.h")).read()
    m = re.search(r"kPackThreadBytes = (\d+)ull << (\d+);", src)
    assert m, "kPackThreadBytes not found in cvx_host_logic.h"
    return int(m.group(1)) << int(m.group(2))


@pytest.fixture(scope="module")
def zoo(hip_aligner):
    """The 48 tiles of test_page_locked_arena_travels_without_packing (tests/test_gpu_corridor.py) and what batch_align makes of them."""
    rng = np.random.default_rng(79)
    tiles = [synth.make_tile(rng, int(rng.integers(300, 4000)), corridor=c, scatter=20.0)
             for c in ("anchors", "endpoints", "linear", "full", "anchors", "anchors") for _ in range(8)]
    return tiles, hip_aligner.batch_align(tiles, want_nm=False)


@pytest.mark.parametrize("closed", [False, True], ids=["rows", "closed"])
@pytest.mark.parametrize("which", [("qry",), ("ref",), ("ref", "qry"), ()], ids=["reads", "references", "both", "neither"])
def test_each_pinned_form(hip_aligner, zoo, which, closed):
    tiles, want = zoo
    ts = synth.tileset_from_tiles(tiles).use_closed_form(closed)
    if which:
        assert ts.pin(hip_aligner.lib, which), "cvx_host_alloc failed on a GPU box"
    try:
        for _ in range(2):           # second round: recycled batch arenas
            job = hip_aligner.submit(ts)
            res, ops = job.wait()
            for i, w in enumerate(want):
                r = res[i]
                assert int(r["status"]) == w["status"], tiles[i].tag
                if w["status"] == 0:
                    assert int(np.float32(r["score"]).view(np.uint32)) == w["fwd_score_bits"]
                    assert (int(r["best_ref_index"]), int(r["best_read_index"])) == (w["best_x"], w["best_y"])
                    assert int(r["ref_position"]) == w["position_offset"]
            txt = job.text()
            for i, w in enumerate(want):
                if w["ret"] >= 0:
                    assert txt[i]["cigar"] == w["cigar"] and txt[i]["md"] == w["md"], tiles[i].tag
            job.release()
    finally:
        ts.unpin()


def _records(job):
    """Every result record of a finished job with its ops, as comparable tuples."""
    res, ops = job.wait()
    out = []
    for r in res:
        b, k = int(r["ops_begin"]), int(r["n_ops"])
        out.append((int(r["status"]), int(np.float32(r["score"]).view(np.uint32)), int(r["best_ref_index"]), int(r["best_read_index"]),
                    int(r["ref_position"]), int(r["qstart"]), int(r["qend"]), int(r["cells"]), ops[b:b + k].tobytes()))
    return out


def test_eight_pieces_equal_three_small_batches(hip_aligner):
    """Row arrays whose packing work just passes the threshold: packed and copied in eight pieces, each piece's copies
    under the packing of the next.  The same tiles in three batches below the threshold are packed in one piece each."""
    PACK_THREAD_BYTES = _pack_thread_bytes()
    ts = synth.pacbio_tileset(94, seed=83, read_len=8000)
    work = lambda t: int((t.W + t.H + 9 * t.H + 64).sum())  # noqa: E731    (UploadLayout::wprefix, cvx_host_logic.h)
    assert work(ts) >= PACK_THREAD_BYTES, work(ts)
    assert work(ts) < PACK_THREAD_BYTES * 9 // 8        # the smallest batch that takes the path, not a large one
    job = hip_aligner.submit(ts)
    got = _records(job)
    job.release()
    want = []
    for lo in range(0, len(ts), 32):
        part = ts.subset(np.arange(lo, min(lo + 32, len(ts))))
        assert work(part) < PACK_THREAD_BYTES
        job = hip_aligner.submit(part)
        want += _records(job)
        job.release()
    assert len(got) == len(want) == len(ts)
    assert sum(r[0] == 0 for r in want) > 80
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, i


def test_windows_with_pinned_reads(hip_aligner):
    """cvx_submit_windows with the reads in page-locked memory: the pads around the reads come from the block of zeros, the
    references and the pad behind them from the device.  Results equal those of the call with ordinary memory."""
    from ngmlr_amd.aligner import Genome
    from oracle.pyoracle import DecodeOracle
    z = np.load(os.path.join(util.GOLDEN, "decode_test_3.npz"))
    starts = [int(x) for x in z["starts"]]
    orc = DecodeOracle()
    rng = np.random.default_rng(8)
    tiles, positions = [], []
    for k in range(24):
        c = int(rng.integers(0, len(starts) - 1))
        W = int(rng.integers(200, 5000))
        p = int(rng.integers(starts[c], max(starts[c] + 1, starts[c + 1] - 1000 - W) + 1))
        ref = orc.window(z["binref"], z["starts"], p, W + 1)[:W]
        qry = synth.mutate(rng, np.frombuffer(ref.replace(b"x", b"A"), dtype=np.uint8), 0.12)
        off, ln = synth.corridor_anchors(len(qry), W)
        tiles.append(synth.Tile(ref, qry.tobytes(), off, ln, tag="win%d" % k))
        positions.append(p)
    g = Genome(hip_aligner, z["binref"], int(z["nibbles"]), z["starts"])
    ts = synth.tileset_from_tiles(tiles)
    try:
        job = g.submit(ts, positions)
        want = _records(job)
        job.release()
        assert ts.pin(hip_aligner.lib, ("qry",)), "cvx_host_alloc failed on a GPU box"
        for _ in range(2):           # second round: recycled batch arenas
            job = g.submit(ts, positions)
            got = _records(job)
            job.release()
            assert got == want
        assert sum(r[0] == 0 for r in want) > 12
    finally:
        ts.unpin()
        g.free()
