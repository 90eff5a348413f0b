"""GPU: cvx_submit_segments -- every tile's query named as a segment of a read block and written on the device -- against
cvx_submit / cvx_submit_windows on host-built queries: result records and ops byte-identical, with and without a resident genome,
on a default and on a scalar-twin handle, the read block pageable and in memory from cvx_host_alloc.  Argument errors leave the
handle usable; a job of plain tiles in the slot a job of segments used finds clean pads."""
import ctypes as C
import os

import numpy as np
import pytest

from tests.segment_cases import embed_queries, want_string

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _queries(rng, refs):
    from ngmlr_amd import synth
    return [synth.mutate(rng, np.frombuffer(r.replace(b"x", b"A"), dtype=np.uint8), 0.12).tobytes() for r in refs]


def _tiles(refs, queries, chained_last=False):
    from ngmlr_amd import synth
    tiles = []
    for k, (r, q) in enumerate(zip(refs, queries)):
        off, ln = synth.corridor_full(len(q), len(r)) if chained_last and k == len(refs) - 1 else synth.corridor_anchors(len(q), len(r))
        tiles.append(synth.Tile(r, q, off, ln, tag="seg%d" % k))
    return tiles


@pytest.fixture(scope="module")
def plain_case(built):
    """64 tiles of 300-1 500 rows with mixed flags, four tiles per read; two 10 kb tiles; one tile whose corridor is chained"""
    from ngmlr_amd import synth
    rng = np.random.default_rng(21)
    refs = [synth.random_ref(rng, int(rng.integers(300, 1500)), n_frac=0.01).tobytes() for _ in range(64)]
    refs += [synth.random_ref(rng, 10000).tobytes() for _ in range(2)] + [synth.random_ref(rng, 700).tobytes()]
    queries = _queries(rng, refs)
    flags = [int(x) for x in rng.integers(0, 2, size=len(refs))]
    flags[64], flags[65] = 0, 1
    reads, segs = embed_queries(rng, queries, flags)
    assert all(want_string(reads[r], s, len(q), f) == q for (r, s, f), q in zip(segs, queries))
    return _tiles(refs, queries, chained_last=True), reads, segs, None


@pytest.fixture(scope="module")
def window_case(built):
    """the same with every reference a window of the resident genome (some hang over a chromosome's end)"""
    from oracle.pyoracle import DecodeOracle
    z = np.load(os.path.join(ROOT, "tests", "golden", "decode_test_3.npz"))
    starts = [int(x) for x in z["starts"]]
    orc = DecodeOracle()
    rng = np.random.default_rng(22)
    refs, positions = [], []
    for k in range(40):
        c = int(rng.integers(0, len(starts) - 1))
        W = int(rng.integers(300, 1500)) if k else 10000
        lo = starts[c] - (300 if k % 7 == 0 else 0)
        hi = max(lo + 1, starts[c + 1] - 1000 - W + (300 if k % 5 == 0 else 0))
        p = int(rng.integers(lo, hi + 1))
        refs.append(orc.window(z["binref"], z["starts"], p, W + 1)[:W])
        positions.append(p)
    queries = _queries(rng, refs)
    flags = [int(x) for x in rng.integers(0, 2, size=len(refs))]
    reads, segs = embed_queries(rng, queries, flags)
    return _tiles(refs, queries), reads, segs, (z["binref"], int(z["nibbles"]), z["starts"], positions)


@pytest.fixture(scope="module")
def aligners(built):
    from ngmlr_amd.aligner import ConvexAlignHip
    als = {False: ConvexAlignHip(device=0), True: ConvexAlignHip(device=0, scalar_twin=True)}
    yield als
    for al in als.values():
        al.close()


def _same(job_a, job_b):
    ra, oa = job_a.wait()
    rb, ob = job_b.wait()
    assert ra.tobytes() == rb.tobytes()
    assert oa.tobytes() == ob.tobytes() and len(oa) > 0
    return ra


@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "host_alloc"])
@pytest.mark.parametrize("twin", [False, True], ids=["default", "twin"])
@pytest.mark.parametrize("case", ["plain", "windows"])
def test_segments_equal_host_built_queries(aligners, plain_case, window_case, case, twin, pinned):
    from ngmlr_amd.aligner import Genome, KmerIndex
    al = aligners[twin]
    tiles, reads, segs, gen = plain_case if case == "plain" else window_case
    g = Genome(al, gen[0], gen[1], gen[2]) if gen else None
    arena, offsets, pin = KmerIndex.make_arena(reads, lib=al.lib if pinned else None)
    assert (pin is not None) == pinned
    before = arena.copy()
    want = g.submit(tiles, gen[3]) if gen else al.submit(tiles)
    got = al.submit_segments(tiles, (arena, offsets), segs, genome=g, ref_positions=gen[3] if gen else None)
    # the read block travelled straight from the page-locked arena, or through the job's staging (the tiles' references are pageable)
    assert got.zero_copy_bytes() == (int(offsets[-1]) if pinned else 0) and want.zero_copy_bytes() == 0
    res = _same(want, got)
    assert int((res["status"] == 0).sum()) > len(tiles) // 2
    if case == "plain" and not twin:
        assert got.timing().n_tiles_chained >= 1
    if gen:      # cvx_job_window_refs keeps working
        ptrs = (C.c_void_p * len(tiles))()
        assert al.lib.cvx_job_window_refs(al.h, got.j, ptrs) == 0
        assert all(C.string_at(p, len(t.ref)) == t.ref for t, p in zip(tiles, ptrs))
    assert (arena == before).all()      # never modified
    want.release()
    got.release()
    if g:
        g.free()
    if pin:
        pin[0].cvx_host_free(pin[1])


def test_argument_errors_leave_the_handle_usable(aligners, plain_case):
    from ngmlr_amd import capi
    al = aligners[False]
    tiles, reads, segs, _ = plain_case
    tiles, segs = tiles[:6], list(segs[:6])
    r0, s0, _ = segs[2]
    for bad in ((len(reads), 0, 0), (-1, 0, 0), (r0, -1, 0), (r0, len(reads[r0]) - len(tiles[2].qry) + 1, 0), (r0, s0, 2), (r0, s0, -1)):
        with pytest.raises(capi.CvxError) as e:
            al.submit_segments(tiles, reads, segs[:2] + [bad] + segs[3:])
        assert e.value.code == -3, bad
    from ngmlr_amd.aligner import KmerIndex
    arena, offsets, _ = KmerIndex.make_arena(reads)
    down = offsets.copy()
    down[2] = down[1]
    with pytest.raises(capi.CvxError) as e:
        al.submit_segments(tiles, (arena, down), segs)
    assert e.value.code == -3 and "ascend" in str(e.value)
    want, got = al.submit(tiles), al.submit_segments(tiles, reads, segs)
    _same(want, got)
    want.release()
    got.release()


def test_plain_job_after_segments_in_the_same_slot(aligners, plain_case):
    """the pads the device cleared itself are clean: a plain job that reuses the slot's arenas gives what a fresh handle gives;
    an empty job of segments is a job like any other"""
    from ngmlr_amd.aligner import ConvexAlignHip
    tiles, reads, segs, _ = plain_case
    fresh = ConvexAlignHip(device=0)
    ref = fresh.submit(tiles[:40])
    rr, ro = ref.wait()
    al = aligners[False]
    for _ in range(2):
        j = al.submit_segments(tiles, reads, segs)
        j.wait()
        j.release()
        p = al.submit(tiles[:40])
        pr, po = p.wait()
        assert pr.tobytes() == rr.tobytes() and po.tobytes() == ro.tobytes()
        p.release()
    e = al.submit_segments([], reads, [])
    r, o = e.wait()
    assert len(r) == 0 and len(o) == 0
    e.release()
    ref.release()
    fresh.close()


@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "host_alloc"])
def test_read_block_of_several_pieces(aligners, pinned):
    """a read block of 9.4 MB: pageable, it goes through the job's staging in three pieces of 4 MB, copied there on the pack threads
    (8 MB and more); from cvx_host_alloc it is pulled as it is.  Segments at both ends of the block, across both piece boundaries
    and across the reads' own boundaries' neighbourhoods, both directions."""
    from ngmlr_amd import synth
    from ngmlr_amd.aligner import KmerIndex
    al = aligners[False]
    rng = np.random.default_rng(33)
    reads = [bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=n)) for n in (3_300_000, 3_000_001, 3_100_000)]
    arena, offsets, pin = KmerIndex.make_arena(reads, lib=al.lib if pinned else None)
    assert int(offsets[-1]) > (8 << 20) and (pin is not None) == pinned
    piece = 4 << 20
    where = [0, piece - 500, 2 * piece - 300, int(offsets[-1]) - 1 - 900, int(offsets[1]) - 1 - 900, int(offsets[1]), int(offsets[2]) - 1 - 1000, piece + 17]
    segs, tiles = [], []
    for k, at in enumerate(where):
        r = int(np.searchsorted(offsets, at, side="right")) - 1
        start, length, flags = at - int(offsets[r]), 600 + 37 * k, k & 1
        assert start + length <= len(reads[r])
        q = want_string(reads[r], start, length, flags)
        ref = synth.mutate(rng, np.frombuffer(q, dtype=np.uint8), 0.1).tobytes()
        off, ln = synth.corridor_anchors(len(q), len(ref))
        tiles.append(synth.Tile(ref, q, off, ln, tag="big%d" % k))
        segs.append((r, start, flags))
    want = al.submit(tiles)
    got = al.submit_segments(tiles, (arena, offsets), segs)
    assert got.zero_copy_bytes() == (int(offsets[-1]) if pinned else 0)
    res = _same(want, got)
    assert int((res["status"] == 0).sum()) == len(tiles)
    want.release()
    got.release()
    if pin:
        pin[0].cvx_host_free(pin[1])
