"""GPU (-m gpu): search and score in one device call (cvx_search_score_arena: plan_candidate_windows_kernel of cvx_score_cands.hip
between the search's compaction and the staging and scoring kernels).  Everything it returns against the two calls it replaces --
cvx_search_batch_arena, then cvx_score_windows on pairs built on the host from the lists -- and, independently of the device,
against the CPU checkers: oracle.pyoracle's search, cvx_stage_windows_host's strings, the StrippedSW restatement."""
import ctypes as C
import functools
import os
from types import SimpleNamespace

import numpy as np
import pytest

from tests import util

pytestmark = pytest.mark.gpu

K, REF_SKIP, BIN_SHIFT = 13, 2, 4


def _bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32)


def _build_table(lib, binref, nibbles, starts, lens):
    """cvx_index_build over an encoded genome -> (index bytes, locations)"""
    from ngmlr_amd import capi
    lens = np.ascontiguousarray(lens, dtype=np.uint64)
    st = np.ascontiguousarray(starts, dtype=np.uint64)
    idx = np.zeros(((1 << (2 * K)) + 2) * 5, dtype=np.uint8)
    locs = np.zeros(int(lens.sum()) // (REF_SKIP + 1) + 64, dtype=np.uint32)
    nl = C.c_uint64()
    capi.check(lib.cvx_index_build(binref.ctypes.data, int(nibbles), st.ctypes.data, lens.ctypes.data, len(lens), K, REF_SKIP, BIN_SHIFT,
                                   idx.ctypes.data, locs.ctypes.data, len(locs), C.byref(nl)))
    return idx.view(np.dtype([("tab", "<u4"), ("rc", "i1")])), locs[:nl.value].copy()


@functools.lru_cache(maxsize=None)
def _test_3():
    """the sub-reads of tests/golden/cs_test_3.npz over the genome they were recorded on (tests/golden/decode_test_3.npz), the table
    rebuilt from that genome by cvx_index_build and held against the recorded one; buffer_len / window_lead as the recorded
    ScoreBuffer::DoRun calls have them (tests/golden/score_windows_test_3.npz: refMaxLen 308, corridor >> 1 = 20)"""
    from ngmlr_amd import capi
    from oracle.pyoracle import SearchFixture
    lib = capi.load()
    g = np.load(os.path.join(util.GOLDEN, "decode_test_3.npz"))
    binref, nibbles, starts = np.ascontiguousarray(g["binref"]), int(g["nibbles"]), g["starts"]
    # a sequence is followed by a pad nibble when its length is odd, then by 1 000 N: its length from the start table (an N at a
    # sequence's very end would be taken for the pad, which changes nothing: no k-mer holds it)
    lens = []
    for i in range(len(starts) - 1):
        d = int(starts[i + 1] - starts[i]) - 1000
        p = int(starts[i]) + d - 1
        last = (binref[p >> 1] & 0xF) if (p & 1) else (binref[p >> 1] >> 4)
        lens.append(d - 1 if last == 4 else d)
    idx, locs = _build_table(lib, binref, nibbles, starts, lens)
    fx = SearchFixture(os.path.join(util.GOLDEN, "cs_test_3.npz"))
    want_idx, want_locs = fx.index_arrays()
    assert np.array_equal(locs, want_locs) and np.array_equal(idx[:-1], want_idx[:-1]), "the rebuilt table is not the recorded one"
    z = np.load(os.path.join(util.GOLDEN, "score_windows_test_3.npz"))
    do_run = z["kind"] == 0
    buffer_len = int(z["buffer_len"][do_run][0])
    lead = int(z["location"][do_run][0]) - int(z["position"][do_run][0])
    assert (buffer_len, lead) == (308, 20)
    return SimpleNamespace(name="test_3", binref=binref, nibbles=nibbles, starts=starts, idx=idx, locs=locs, reads=fx.seqs, recorded=fx.want,
                           buffer_len=buffer_len, lead=lead)


def _revcomp(s):
    return s[::-1].translate(bytes.maketrans(b"ACGT", b"TGCA"))


@functools.lru_cache(maxsize=None)
def _corners():
    """A two-contig genome (the first of odd length) with a repeat of four copies and a reverse-complement palindrome, and 256-base
    reads from both strands at the contigs' starts and ends."""
    from ngmlr_amd import capi, synth
    from ngmlr_amd.aligner import encode_genome
    lib = capi.load()
    rng = np.random.default_rng(77)
    a = synth.random_ref(rng, 2301).tobytes()
    b = synth.random_ref(rng, 1800).tobytes()
    unit = synth.random_ref(rng, 256).tobytes()
    half = synth.random_ref(rng, 128).tobytes()
    pal = half + _revcomp(half)                       # its own reverse complement: votes on both strands of the same window
    a = a[:500] + unit + a[756:1100] + unit + a[1356:1700] + pal + a[1956:]
    b = b[:400] + unit + b[656:1000] + unit + b[1256:]
    assert len(a) == 2301 and len(b) == 1800
    binref, nibbles, starts = encode_genome(lib, [a, b])
    idx, locs = _build_table(lib, binref, nibbles, starts, [len(a), len(b)])
    reads = [a[:256], _revcomp(a[:256]),             # the first contig's start: a location behind the leading spacer
             unit,                                    # four copies: a list that reaches a max_cmrs of 3
             a[-256:], _revcomp(a[-256:]),
             b"N" * 256,                              # no list, between two reads with lists
             b[:256], _revcomp(b[10:266]),
             pal,
             _revcomp(unit),
             b[-256:], _revcomp(b[-256:])]            # the genome's end: a long window runs past L
    return SimpleNamespace(name="corners", binref=binref, nibbles=nibbles, starts=starts, idx=idx, locs=locs, reads=reads)


@pytest.fixture(scope="module")
def dev(hip_aligner):
    """both genomes and both tables resident on ONE handle"""
    from ngmlr_amd.aligner import Genome, KmerIndex
    out = {}
    for case in (_test_3(), _corners()):
        out[case.name] = SimpleNamespace(case=case, genome=Genome(hip_aligner, case.binref, case.nibbles, case.starts),
                                         ix=KmerIndex(hip_aligner, K, case.idx, case.locs, 0), al=hip_aligner)
    yield out
    for d in out.values():
        d.ix.free()
        d.genome.free()


@pytest.fixture(params=["wave", "wave_hbm"])
def search_kernel(request, monkeypatch):
    """where the dense list comes from: the LDS-map form of the vote, or every read over the table in HBM"""
    if request.param == "wave_hbm":
        monkeypatch.setenv("CVX_TUNE_SEARCH_WAVE", "2")
    return request.param


def _pairs_of(ncand, begin, cands, buffer_len, lead, max_cmrs):
    """the pairs the host builds from the lists for the second call -> (WINDOW_DTYPE table, the candidate each pair belongs to)"""
    from ngmlr_amd.aligner import WINDOW_DTYPE
    rows, owner = [], []
    for i in range(len(ncand)):
        if ncand[i] <= 0 or ncand[i] >= max_cmrs:      # no list, or one that is not handed to AllocScores (src/CS.cpp:264-266)
            continue
        for q in range(int(begin[i]), int(begin[i]) + int(ncand[i])):
            rows.append(((int(cands["location"][q]) - lead) & 0xFFFFFFFFFFFFFFFF, buffer_len, i, int(cands["reverse"][q]), 0))
            owner.append(q)
    return np.array(rows, dtype=WINDOW_DTYPE), np.array(owner, dtype=np.int64)


def _dropped(ncand, begin, used, max_cmrs):
    st = np.zeros(used, dtype=np.int32)
    for i in range(len(ncand)):
        if ncand[i] >= max_cmrs:
            st[int(begin[i]):int(begin[i]) + int(ncand[i])] = 2
    return st


def _two_calls(d, arena, offsets, buffer_len, lead, max_cmrs):
    """cvx_search_batch_arena, then cvx_score_windows on the same handle -> everything the fused call returns"""
    from ngmlr_amd import capi
    ncand, begin, cands, mh, ms = d.ix.search_arena(arena, offsets)
    tab, owner = _pairs_of(ncand, begin, cands, buffer_len, lead, max_cmrs)
    scores = np.full(len(cands), -1.0, dtype=np.float32)
    status = _dropped(ncand, begin, len(cands), max_cmrs)
    if len(tab):
        sc = np.zeros(len(tab), dtype=np.float32)
        st = np.zeros(len(tab), dtype=np.int32)
        capi.check(d.al.lib.cvx_score_windows(d.al.h, d.genome.g, len(offsets) - 1, arena.ctypes.data, offsets.ctypes.data, len(tab), tab.ctypes.data,
                                              sc.ctypes.data, st.ctypes.data))
        scores[owner], status[owner] = sc, st
    return ncand.copy(), begin.copy(), cands.copy(), mh.copy(), ms.copy(), scores, status


@functools.lru_cache(maxsize=None)
def _oracle(name, buffer_len, lead, max_cmrs):
    """the same from the CPU checkers alone: cs_oracle's lists, cvx_stage_windows_host's strings, the StrippedSW restatement's scores
    -> (per-read lists or None, scores, status, the staged windows); computed once per case"""
    from ngmlr_amd import capi
    from ngmlr_amd.aligner import stage_windows_host
    from oracle.pyoracle import ScoreOracle, SearchOracle
    case = _test_3() if name == "test_3" else _corners()
    o = SearchOracle(raw=(K, 0, case.idx, case.locs))
    lists = [o.search(r, cap=1 << 14) for r in case.reads]
    o.close()
    ncand = np.array([w["n"] for w in lists], dtype=np.int32)
    begin = np.concatenate([[0], np.cumsum(np.maximum(ncand, 0))]).astype(np.uint64)
    used = int(begin[-1])
    cands = np.zeros(used, dtype=[("location", np.uint64), ("score", np.float32), ("reverse", np.int32)])
    for i, w in enumerate(lists):
        if w["n"] > 0:
            s = slice(int(begin[i]), int(begin[i]) + w["n"])
            cands["location"][s], cands["score"][s], cands["reverse"][s] = w["loc"], w["score"], w["rev"]
    tab, owner = _pairs_of(ncand, begin[:-1], cands, buffer_len, lead, max_cmrs)
    scores = np.full(used, -1.0, dtype=np.float32)
    status = _dropped(ncand, begin[:-1], used, max_cmrs)
    win = []
    if len(tab):
        win, qry, st = stage_windows_host(capi.load(), case.binref, case.nibbles, case.starts, case.reads, tab)
        ok = np.flatnonzero(st == 0)
        sc = np.full(len(tab), -1.0, dtype=np.float32)
        sc[ok] = ScoreOracle("port").scores([win[i] for i in ok], [qry[i] for i in ok])
        scores[owner], status[owner] = sc, st
    return lists, cands, scores, status, win


def _check_against_oracle(name, got, buffer_len, lead, max_cmrs):
    ncand, begin, cands, mh, ms, sw, st = got
    lists, o_cands, o_scores, o_status, _ = _oracle(name, buffer_len, lead, max_cmrs)
    for i, w in enumerate(lists):      # (a read the reference gives up on has a negative count on both sides)
        assert (w["n"] < 0 and ncand[i] < 0) or int(ncand[i]) == w["n"], (i, int(ncand[i]), w["n"])
    assert np.array_equal(cands["location"], o_cands["location"]) and np.array_equal(cands["reverse"], o_cands["reverse"])
    assert np.array_equal(_bits(cands["score"]), _bits(o_cands["score"]))
    assert np.array_equal(st, o_status), np.flatnonzero(st != o_status)[:10]
    assert np.array_equal(_bits(sw), _bits(o_scores)), np.flatnonzero(sw != o_scores)[:10]


def _same_as(got, want):
    for a, b, what in zip(got, want, ("n_candidates", "cand_begin", "cands", "max_hit", "kmer_misses", "sw_scores", "sw_status")):
        if what == "cands":
            assert a.tobytes() == b.tobytes(), what
        elif a.dtype == np.float32:
            assert np.array_equal(_bits(a), _bits(b)), (what, np.flatnonzero(_bits(a) != _bits(b))[:10])
        else:
            assert np.array_equal(a, b), (what, np.flatnonzero(a != b)[:10])


def _arena(reads):
    from ngmlr_amd.aligner import KmerIndex
    arena, offsets, _ = KmerIndex.make_arena(reads)
    return arena, offsets


def _fused_ms(al):
    from ngmlr_amd import capi
    return al.stage_kernel_ms(capi.STAGE_SEARCH_SCORE)


def test_the_fused_call_equals_the_two_calls_on_test_3(dev, search_kernel):
    d = dev["test_3"]
    c = d.case
    arena, offsets = _arena(c.reads)
    max_cmrs = 1000
    got = d.ix.search_score_arena(d.genome, arena, offsets, c.buffer_len, c.lead, max_cmrs)
    assert _fused_ms(d.al) > 0.0
    want = _two_calls(d, arena, offsets, c.buffer_len, c.lead, max_cmrs)
    _same_as(got, want)
    _check_against_oracle("test_3", got, c.buffer_len, c.lead, max_cmrs)
    ncand, begin, cands, _, _, sw, st = got
    # ... which are the lists the unmodified reference recorded, and scores worth comparing
    for i, (loc, sc, rev) in enumerate(c.recorded):
        mine = cands[int(begin[i]):int(begin[i]) + max(int(ncand[i]), 0)]
        assert np.array_equal(mine["location"], loc) and np.array_equal(mine["score"], sc) and np.array_equal(mine["reverse"], rev), i
    # (15 % error and a gap at 255 per base: a score is the best ungapped stretch, a few dozen at most -- but never that of an empty string)
    assert len(cands) > 1000 and not st.any() and float(sw.min()) >= 10.0 and float(sw.max()) > 100.0


# (buffer_len, window_lead, max_cmrs)
CORNER_CALLS = [(308, 20, 1000),        # ScoreBuffer's own shape
                (308, 1200, 1000),      # a lead longer than the leading spacer: the first contig's locations wrap (status 1)
                (1500, 20, 1000),       # windows that run past L: the 'x' tail
                (1501, 21, 3),          # the other parities; the repeat's list reaches max_cmrs (status 2)
                (2048, 1200, 4),        # the largest window
                (2048, 21, 1000)]       # ... with the 'x' tail from an odd position: 2 048 characters, one more than score_class calls diagonal


@pytest.mark.parametrize("buffer_len,lead,max_cmrs", CORNER_CALLS)
def test_engineered_corners(dev, search_kernel, buffer_len, lead, max_cmrs):
    d = dev["corners"]
    c = d.case
    arena, offsets = _arena(c.reads)
    got = d.ix.search_score_arena(d.genome, arena, offsets, buffer_len, lead, max_cmrs)
    want = _two_calls(d, arena, offsets, buffer_len, lead, max_cmrs)
    _same_as(got, want)
    _check_against_oracle("corners", got, buffer_len, lead, max_cmrs)
    ncand, begin, cands, _, _, sw, st = got
    lists = [cands[int(begin[i]):int(begin[i]) + max(int(ncand[i]), 0)] for i in range(len(c.reads))]
    # the case is what it was built to be
    assert ncand[5] <= 0 and ncand[4] > 0 and ncand[6] > 0                               # the read of N between two reads with lists
    assert ncand[2] >= 4 and ncand[9] >= 4                                                # the repeat's four copies
    pal = lists[8]
    assert any(np.any((pal["location"] == loc) & (pal["reverse"] == 0)) and np.any((pal["location"] == loc) & (pal["reverse"] == 1))
               for loc in pal["location"]), "the palindrome does not vote on both strands of one window"
    assert {int(x) for x in lists[0]["reverse"]} == {0} and 1 in {int(x) for x in lists[1]["reverse"]}
    first = int(begin[0])
    covers = lead + 256 <= buffer_len - 2      # the window reaches from the lead in front of the location to behind the read's end
    if lead == 1200:
        assert st[first] == 1 and sw[first] == -1.0, "the location behind the leading spacer does not wrap"
        assert int(lists[0]["location"][0]) < lead
    else:
        assert st[first] == 0 and sw[first] == 256.0
    if max_cmrs <= 4:
        rep = slice(int(begin[2]), int(begin[2]) + int(ncand[2]))
        assert np.all(st[rep] == 2) and np.all(sw[rep] == -1.0)
        # its neighbours are scored as ever
        assert st[int(begin[1])] in (0, 1) and st[int(begin[3])] == 0 and (sw[int(begin[3])] == 256.0 or not covers)
    else:
        assert not np.any(st == 2)
    if buffer_len >= 1500 and lead < 100:
        win = _oracle("corners", buffer_len, lead, max_cmrs)[4]
        assert any(w.endswith(b"x" * 50) for w in win), "no window runs past the genome's end"
    assert np.any(st == 0)


def test_a_call_without_candidates_launches_nothing(dev):
    d = dev["test_3"]
    c = d.case
    arena, offsets = _arena(c.reads[:40])
    got = d.ix.search_score_arena(d.genome, arena, offsets, c.buffer_len, c.lead, 1000)
    assert len(got[2]) > 0 and _fused_ms(d.al) > 0.0
    arena, offsets = _arena([b"N" * 256, b"ACGT", b"", b"N" * 30])
    ncand, begin, cands, mh, ms, sw, st = d.ix.search_score_arena(d.genome, arena, offsets, c.buffer_len, c.lead, 1000)      # CVX_OK
    assert len(cands) == 0 and len(sw) == 0 and len(st) == 0 and np.all(ncand <= 0)
    assert _fused_ms(d.al) == 0.0


def test_calls_in_a_row_and_between_other_calls(dev):
    """a smaller call behind a larger one on the same handle (descriptors, pairs and strings of the larger one are still in the
    buffers), then the two single calls on that handle, then the fused call again: all as when run alone"""
    d = dev["test_3"]
    c = d.case
    big, small = _arena(c.reads[:400]), _arena(c.reads[100:160])
    alone_big = _two_calls(d, big[0], big[1], c.buffer_len, c.lead, 1000)
    alone_small = _two_calls(d, small[0], small[1], c.buffer_len, c.lead, 1000)
    assert len(alone_small[2]) < len(alone_big[2]) and len(alone_small[2]) > 0
    _same_as(d.ix.search_score_arena(d.genome, big[0], big[1], c.buffer_len, c.lead, 1000), alone_big)
    _same_as(d.ix.search_score_arena(d.genome, small[0], small[1], c.buffer_len, c.lead, 1000), alone_small)
    other = dev["corners"]
    oa = _arena(other.case.reads)
    alone_other = _two_calls(other, oa[0], oa[1], 1500, 20, 3)      # (a search and a cvx_score_windows on the handle, other genome and table)
    _same_as(d.ix.search_score_arena(d.genome, small[0], small[1], c.buffer_len, c.lead, 1000), alone_small)
    _same_as(other.ix.search_score_arena(other.genome, oa[0], oa[1], 1500, 20, 3), alone_other)
    _same_as(_two_calls(d, big[0], big[1], c.buffer_len, c.lead, 1000), alone_big)
    _same_as(d.ix.search_score_arena(d.genome, big[0], big[1], c.buffer_len, c.lead, 1000), alone_big)


def test_argument_errors(dev):
    from ngmlr_amd import capi
    from ngmlr_amd.aligner import CANDIDATE_DTYPE
    d = dev["test_3"]
    c = d.case
    lib = d.al.lib
    arena, offsets = _arena(c.reads[:30])
    n = len(offsets) - 1
    ncand, begin = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.uint64)
    cands = np.zeros(4096, dtype=CANDIDATE_DTYPE)
    sw, st = np.zeros(4096, dtype=np.float32), np.zeros(4096, dtype=np.int32)
    used = C.c_uint64()

    def call(buffer_len=c.buffer_len, lead=c.lead, max_cmrs=1000, cap=4096, scores=sw, genome=None, a=arena, o=offsets):
        used.value = 12345
        return lib.cvx_search_score_arena(d.al.h, d.ix.ix, (genome or d.genome).g, len(o) - 1, a.ctypes.data, o.ctypes.data, 0.8, 0.0, BIN_SHIFT, 0,
                                          buffer_len, lead, max_cmrs, ncand.ctypes.data, begin.ctypes.data, cands.ctypes.data, cap, C.byref(used),
                                          None, None, scores.ctypes.data if scores is not None else None, st.ctypes.data)
    ERR_ARG, ERR_CAPACITY = -3, -6
    assert call(buffer_len=2) == ERR_ARG
    assert call(buffer_len=2049) == ERR_ARG
    assert call(max_cmrs=0) == ERR_ARG
    assert call(lead=-1) == ERR_ARG
    assert call(scores=None) == ERR_ARG
    long_arena, long_offsets = _arena([c.reads[0], c.reads[1] + c.reads[2]])      # a read of 512 characters
    assert call(a=long_arena, o=long_offsets) == ERR_ARG
    ok_arena, ok_offsets = _arena([c.reads[0], (c.reads[1] + c.reads[2])[:511]])   # 511 are taken
    assert call(a=ok_arena, o=ok_offsets) == 0
    st[:] = -7
    assert call(cap=3) == ERR_CAPACITY and used.value > 3 and np.all(st == -7)      # the need comes back, nothing is scored
    need = int(used.value)
    assert call() == 0 and int(used.value) == need and np.all(st[:need] == 0) and np.all(sw[:need] >= 0.0)
    assert call(buffer_len=2048) == 0 and call(buffer_len=3) == 0
    capi.check(call())


def test_a_genome_on_another_device_is_refused(dev):
    from ngmlr_amd.aligner import CANDIDATE_DTYPE, ConvexAlignHip, Genome
    d = dev["test_3"]
    c = d.case
    lib = d.al.lib
    if lib.cvx_device_count() < 2:
        pytest.skip("needs two devices: a genome can only lie on another device than the handle where there is one")
    arena, offsets = _arena(c.reads[:30])
    n = len(offsets) - 1
    ncand, begin = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.uint64)
    cands = np.zeros(4096, dtype=CANDIDATE_DTYPE)
    sw, st = np.zeros(4096, dtype=np.float32), np.zeros(4096, dtype=np.int32)
    used = C.c_uint64()
    al2 = ConvexAlignHip(device=1)
    g2 = Genome(al2, c.binref, c.nibbles, c.starts)
    try:
        rc = lib.cvx_search_score_arena(d.al.h, d.ix.ix, g2.g, n, arena.ctypes.data, offsets.ctypes.data, 0.8, 0.0, BIN_SHIFT, 0, c.buffer_len, c.lead, 1000,
                                        ncand.ctypes.data, begin.ctypes.data, cands.ctypes.data, 4096, C.byref(used), None, None, sw.ctypes.data, st.ctypes.data)
        assert rc == -3
    finally:
        g2.free()
        al2.close()
