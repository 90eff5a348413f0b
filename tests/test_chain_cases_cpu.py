"""CPU: the tile families of tests/chain_cases.py do what they are for.  Under the port oracle, with each case's scoring, every
cross, brow, rows and valid phase tile walks to its script op for op; every phase tile whose path is its rows' first cells is
rejected with a positive raw fill score; the ties tiles report the rows they were written for; the clip tiles are valid.  From
the scripts and rows alone the families reach the edges they are named after: every residue of a 32-step word and a 16-record
chunk for block 1's first cell, every relation of the rows above the boundary to run 27, the three last-block heights, the
clipped and the empty spans of the row above a block.  cross and phase also against the reference's own ConvexAlignFast."""
import numpy as np
import pytest

from oracle.pyoracle import Oracle, same_alignment
from tests import chain_cases as cc
from tests import sse_row_cases as rc


@pytest.fixture(scope="module")
def cases():
    return {N: cc.families(N) for N in cc.HEIGHTS}


@pytest.fixture(scope="module")
def answers(built, cases):
    """N -> (ret, ops, raw fill score bits, best cell) of every case under the port oracle with the case's scoring"""
    orc = {}
    out = {}
    for N, cs in cases.items():
        out[N] = []
        for c in cs:
            key = cc.params(c.scoring)
            if key not in orc:
                orc[key] = Oracle("port", key)
            w = orc[key].align(c.tile, want_nm=False)
            f = orc[key].last_fwd()
            out[N].append((w["ret"], orc[key].last_ops().tolist() if w["ret"] >= 0 else None, orc[key].last_fill_score_bits(),
                           (f["best_x"], f["best_y"])))
    return out


def _every(cases, answers):
    for N in cc.HEIGHTS:
        for c, a in zip(cases[N], answers[N]):
            yield N, c, a


def test_family_sizes(cases):
    for N, cs in cases.items():
        n = {f: sum(1 for c in cs if c.family == f) for f in cc.FAMILIES}
        cross = sum(len(cc.cross_ks(N, k, sc)) for sc in (cc.DEFAULT, cc.ONT) for k in cc.CROSS_N)
        assert n == {"cross": cross, "brow": 2 * len(cc.BROW_D), "phase": 33 * 3 + 18, "rows": 6, "ties": 3 + (4 if N == 64 else 0), "clip": 7}, (N, n)
        assert cross >= 60
        assert len({c.tile.tag for c in cs}) == len(cs)
        # every tile has more live rows than a 64-slot ring holds, lies inside what a ring kernel takes, and is small
        assert all(rc.is_regular(c.tile) for c in cs)
        assert all(c.tile.H * c.info["L"] <= 600 * 300 or c.tile.H == cc.TIES_H for c in cs)
        assert all(c.tile.H > 64 and c.info["L"] >= 200 for c in cs)
    assert 450 <= sum(len(cs) for cs in cases.values()) <= 1000


def test_every_script_is_its_tiles_alignment(cases, answers):
    """no case left out: every cross, brow and rows tile and every phase tile at column 100 is valid and walks to its script"""
    bad = [(c.tile.tag, ret) for N, c, (ret, ops, _, _) in _every(cases, answers)
           if (c.family in ("cross", "brow", "rows") or (c.family == "phase" and c.info["valid"])) and (ret < 0 or ops != c.ops)]
    assert not bad, (len(bad), bad[:8])


def test_phase_tiles_on_the_first_column_are_rejected_with_a_score(cases, answers):
    n = 0
    for N, c, (ret, ops, fs, best) in _every(cases, answers):
        if c.family == "phase" and not c.info["valid"]:
            assert c.info["col"] in (0, 1)
            assert ret < 0 and fs != 0xBF800000 and np.uint32(fs).view(np.float32) > 0, c.tile.tag
            assert best[1] == c.tile.H - 1, c.tile.tag             # the path runs down to the last row, in its first cells
            n += 1
    assert n == 3 * (33 * 2 + 9)


def test_phase_family_sweeps_a_direction_word_and_a_chunk(cases):
    for N, cs in cases.items():
        phase = [c for c in cs if c.family == "phase"]
        for col in cc.PHASE_COLS:
            steps = []
            for c in phase:
                if c.info["col"] == col and c.info["L"] == cc.L0:
                    first, _, _ = cc.first_steps(c.tile)
                    steps.append(int(first[N] - first[0]))
                    assert steps[-1] == 2 * N + c.info["d"] and steps[-1] % 32 == c.info["residue"] and steps[-1] % 16 == c.info["chunk"]
            assert sorted(s % 32 for s in steps) == sorted(list(range(32)) + [0]), (N, col)
            assert {s % 16 for s in steps} == set(range(16))
        assert any(c.info["residue"] == 0 and c.info["col"] == 0 for c in phase)      # block 1's first cell on a multiple of 32 steps
        # the records of row N - 1: a partial, a full and a one-record last chunk
        assert {c.info["L"] % 16 for c in phase if c.info["L"] != cc.L0} == {15, 0, 1}
        assert {(c.info["L"], c.info["d"], c.info["col"]) for c in phase if c.info["L"] != cc.L0} == {(L, d, col) for L, _ in cc.PHASE_L for d in (0, 1, 15) for col in (100, 0)}


def test_cross_family_reaches_every_relation_to_run_27(cases):
    for N, cs in cases.items():
        for sc in (cc.DEFAULT, cc.ONT):
            cross = [c for c in cs if c.family == "cross" and c.scoring is sc]
            ks = {(c.info["n"], c.info["k"]) for c in cross}
            # the rows above the boundary against the run at which the penalty stops moving, and against the whole run.  (Under
            # the default scoring a block of 64 rows cannot pay for a gap of 26 with 26 of its rows: 38 matches are worth 76,
            # the gap costs 81 -- there the ont scoring has the cases, and the default scoring has them from N = 128 on.)
            if sc is cc.ONT or N > 64:
                assert {(k > 27) - (k < 27) for _, k in ks} == {-1, 0, 1}, (N, sorted(ks))
                assert {0, 1, 2, 26, 27} <= {k for _, k in ks}
                assert {n for n, _ in ks} >= {1, 2, 3, 26, 27, 28, 40, 57}
            else:
                assert {0, 1, 2, 13, 14} <= {k for _, k in ks} and {n for n, _ in ks} >= {1, 2, 3, 26, 27, 28}, sorted(ks)
            assert any(k == 0 for _, k in ks) and any(k == n for n, k in ks) and any(k == n - 1 for n, k in ks)
            # the insertion really straddles row N: rows N - k ... N - k + n - 1
            for c in cross:
                assert c.script[0] == ("=", N - c.info["k"]) and c.script[1] == ("I", c.info["n"])
        assert any(c.info["n"] == 90 for c in cs if c.family == "cross" and c.scoring is cc.ONT)


def test_brow_family_puts_deletions_in_both_rows_at_the_boundary(cases):
    for N, cs in cases.items():
        brow = [c for c in cs if c.family == "brow"]
        assert sorted((c.info["row"], c.info["d"]) for c in brow) == [(r, d) for r in (N - 1, N) for d in range(1, 34)]


def test_rows_family_has_the_three_last_block_heights(cases, answers):
    for N in cc.HEIGHTS:
        rows = [(c, a) for c, a in zip(cases[N], answers[N]) if c.family == "rows"]
        assert sorted({c.info["last"] for c, _ in rows}) == [1, N - 1, N]
        assert [c.tile.H for c, _ in rows] == [N + 1, 2 * N - 1, 2 * N, 2 * N + 1, 3 * N, 3 * N + 1]
        for c, (ret, ops, fs, best) in rows:
            assert best[1] == c.tile.H - 1 and (c.tile.H - 1) // N == (c.tile.H + N - 1) // N - 1      # the best cell in the last block


def test_ties_report_the_earlier_block_unless_the_later_scores_more(cases, answers):
    many = []
    for N, c, (ret, ops, fs, best) in _every(cases, answers):
        if c.family != "ties":
            continue
        assert ret >= 0 and ops == c.ops and best[1] == c.info["best_row"], (c.tile.tag, ret, best)
        assert best[1] // N in c.info["blocks"]
        if c.tile.H == cc.TIES_H:
            many.append(best[1])
    assert many == [103, 231, 4264, 167]
    assert (cc.TIES_H + 63) // 64 == 69
    # lanes of the reduction (block g is taken by lane g % 64): the same lane, the later block in the lower lane
    assert [tuple(g % 64 for g, _ in segs) for segs, _ in cc.TIES_MANY] == [(1, 1), (3, 2), (3, 2), (2, 0, 3)]


def test_clip_family_cuts_the_rows_it_names(cases, answers):
    for N in cc.HEIGHTS:
        clip = {c.kind: (c, a) for c, a in zip(cases[N], answers[N]) if c.family == "clip"}
        assert tuple(clip) == cc.CLIP_CUTS
        span = {}
        for kind, (c, (ret, ops, fs, best)) in clip.items():
            assert ret >= 0 and np.uint32(fs).view(np.float32) > 0, (c.tile.tag, ret)
            assert np.all(np.diff(c.tile.row_offset) >= 0)
            _, lo, hi = cc.first_steps(c.tile)
            span[kind] = (lo, hi, c.tile)
        L = cc.L0
        lo, hi, t = span["row N-1 40 left"]
        assert t.row_offset[N - 1] == -40 and (lo[N - 1], hi[N - 1]) == (0, L - 40)
        lo, hi, t = span["row N-1 at 0"]
        assert t.row_offset[N - 1] == 0 and t.row_offset[N - 2] == -1 and hi[N - 1] - lo[N - 1] == L
        lo, hi, t = span["row N at 0"]
        assert t.row_offset[N] == 0 and t.row_offset[N - 1] == -1 and hi[N - 1] - lo[N - 1] == L - 1
        lo, hi, t = span["block 0 empty"]
        assert np.all(hi[:N] == lo[:N]) and hi[N] - lo[N] == 1
        lo, hi, t = span["block 0 one cell"]
        assert np.all(hi[:N - 1] == lo[:N - 1]) and (lo[N - 1], hi[N - 1]) == (0, 1)
        lo, hi, t = span["rows N-1 on past W"]
        assert np.all(t.row_offset[:N - 1] + L <= t.W) and np.all(t.row_offset[N - 1:] + L > t.W) and hi[N - 1] - lo[N - 1] == L - 1
        lo, hi, t = span["last block empty"]
        last0 = (t.H - 1) // N * N
        assert last0 > N and np.all(hi[last0:] == lo[last0:]) and hi[last0 - 1] > lo[last0 - 1]


@pytest.mark.parametrize("N", cc.HEIGHTS)
def test_cross_and_phase_against_the_reference(cases, answers, ref_oracle, N):
    """the reference's own ConvexAlignFast, with each case's scoring (ref_oracle: skipped where the reference is not built)"""
    bad, n = [], 0
    for sc in (cc.DEFAULT, cc.ONT):
        ref, port = Oracle("reference", cc.params(sc)), Oracle("port", cc.params(sc))
        for c in cases[N]:
            if c.family in ("cross", "phase") and c.scoring is sc:
                d = same_alignment(ref.align(c.tile), port.align(c.tile))
                n += 1
                if d is not None:
                    bad.append((c.tile.tag, d))
    assert not bad, (len(bad), bad[:8])
    assert n >= 170
