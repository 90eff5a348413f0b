"""CPU: the tile families of tests/walk_cases.py do what they are for.  Under the port oracle every script is the alignment its
tile has (op for op), and the families reach the edges they are named after: the lane of a probe at which a gap lies, for every
lanes-per-tile form of the device walk; the phase of a direction word; the validPath band, with valid and invalid cases of
each kind; the ring's wrap."""
import numpy as np
import pytest

from oracle.pyoracle import Oracle
from tests import sse_row_cases as rc
from tests import walk_cases as wc


@pytest.fixture(scope="module")
def cases():
    return wc.families()


@pytest.fixture(scope="module")
def answers(built, cases):
    """(ret, ops, raw fill score bits) of every case under the port oracle with the case's scoring"""
    orc = {}
    out = []
    for c in cases:
        key = wc.params(c.scoring)
        if key not in orc:
            orc[key] = Oracle("port", key)
        w = orc[key].align(c.tile, want_nm=False)
        out.append((w["ret"], orc[key].last_ops().tolist() if w["ret"] >= 0 else None, orc[key].last_fill_score_bits()))
    return out


def test_family_sizes(cases):
    n = {f: sum(1 for c in cases if c.family == f) for f in ("lane", "word", "subrun", "band", "ring")}
    assert n == {"lane": len(wc.LANE_R) * len(wc.LANE_EVENTS), "word": 32 * len(wc.WORD_EVENTS) + len(wc.WORD_EDGE_D) + 36, "subrun": 23, "band": 14,
                 "ring": 2 * len(wc.RING_EVENTS) * len(wc.RING_ROWS) + 2}
    assert len({c.tile.tag for c in cases}) == len(cases)


def test_every_script_is_its_tiles_alignment(cases, answers):
    """no case left out: every tile outside `band` is valid and walks to its script's op list"""
    bad = [(c.tile.tag, ret) for c, (ret, ops, _) in zip(cases, answers) if c.family != "band" and (ret < 0 or ops != c.ops)]
    assert not bad, (len(bad), bad[:8])
    # band: a valid case is its script as well
    bad = [c.tile.tag for c, (ret, ops, _) in zip(cases, answers) if c.family == "band" and ret >= 0 and ops != c.ops]
    assert not bad, bad


def test_lane_family_reaches_lane_0_1_and_the_last_of_every_group(cases):
    lane = [c for c in cases if c.family == "lane"]
    for G in wc.GROUPS + (64,):
        for op in "ID":
            at = {}          # lane of the event -> run lengths
            for c in lane:
                for o, n, R in c.info["events"]:
                    if o == op:
                        at.setdefault(R % G, set()).add(n)
            assert {0, 1, G - 1} <= set(at), (G, op, sorted(at))
            if op == "I":
                # the lanes left in the probe, the gap's own included: a run below, at and above them (a run of at least 1
                # cannot be below the single lane that is left behind lane G - 1)
                for ln in (0, 1, G - 1):
                    left = G - ln
                    rel = {(n > left) - (n < left) for n in at[ln]}
                    assert rel == ({-1, 0, 1} if left > 1 else {0, 1}), (G, ln, sorted(at[ln]))
    # the X events: a sub-run boundary at the same lanes
    assert {R % 64 for c in lane for op, n in [c.info["ev"]] if op == "X" for R in [c.info["R"]]} == {63, 0, 1}


def test_word_family_sweeps_a_direction_word(cases):
    word = [c for c in cases if c.family == "word"]
    for ev in wc.WORD_EVENTS:
        assert sorted(c.info["step"] & 31 for c in word if c.info["ev"] == ev and c.info.get("sweep")) == list(range(32)), ev
    rel = [(c.info["ev"][1] > c.info["in_word"]) - (c.info["ev"][1] < c.info["in_word"]) for c in word if c.info["ev"][0] == "D"]
    assert min(rel.count(-1), rel.count(0), rel.count(1)) >= 8, (rel.count(-1), rel.count(0), rel.count(1))
    brk = [c.info["have_break"] for c in word if c.info["ev"][0] == "I"]
    assert brk.count(None) >= 8 and sum(b is not None for b in brk) >= 8
    # the early deletions: every one reaches the edge of its word
    early = [c for c in word if c.kind.startswith("early")]
    assert len(early) == 36 and all(c.info["in_word"] <= c.info["ev"][1] for c in early)
    # ... and a run of 3 is cut at its cell 1 and at its cell 2
    assert {c.info["have_break"] for c in word if c.info["ev"] == ("I", 3)} == {None, 1, 2}


def test_subrun_family_puts_a_boundary_on_every_lane(cases):
    """the sub-run starts of the x1e3 / x2e5 tiles, counted in cells from the best cell: every lane of an 8-lane probe, lanes
    0, 1 and G - 1 of the wider ones; the x1e1 tiles start a sub-run in every cell of at least one probe of every form"""
    def starts(c):
        out, at = set(), 0
        for v in reversed(c.ops):
            out.add(at)
            at += v >> 4
        return out
    sub = [c for c in cases if c.family == "subrun"]
    for name in ("x1e3", "x2e5"):
        s = set().union(*(starts(c) for c in sub if c.kind.startswith(name)))
        assert {v % 8 for v in s if v >= 48} == set(range(8))
        for G in (16, 32, 64):
            assert {0, 1, G - 1} <= {v % G for v in s if v >= 48}, (name, G)
    for c in sub:
        if c.kind.startswith("x1e1"):
            s = starts(c)
            assert all(any(all(b + k in s for k in range(G)) for b in range(0, 128, G)) for G in wc.GROUPS + ((64,) if "x48" in c.kind else ())), c.kind
    assert sorted(c.kind for c in sub if "cut" in c.kind) == ["e3 cut 1|2", "e3 cut 2|1", "x3 cut 1|2", "x3 cut 2|1"]


def test_band_family_has_valid_and_invalid_cases_of_each_kind(cases, answers):
    got = {}
    for c, (ret, ops, fs) in zip(cases, answers):
        if c.family != "band":
            continue
        assert (ret >= 0) == c.info["valid"], (c.tile.tag, ret)          # the construction's aim is what the oracle says
        if ret < 0:
            score = np.uint32(fs).view(np.float32)
            assert fs != 0xBF800000 and score > 0, c.tile.tag            # rejected by validPath, not for want of a score
        got.setdefault(c.info["what"], set()).add((c.info["edge"], ret >= 0))
    for what in ("diag", "D", "I"):
        assert {v for _, v in got[what]} == {True, False}, (what, got[what])
        assert {e for e, _ in got[what]} == {"left", "right"}, (what, got[what])


def test_ring_family_lands_on_ring_kernels_and_the_wrap_rows(cases):
    ring = [c for c in cases if c.family == "ring"]
    for c in ring:
        if not c.info["chained"]:
            assert rc.is_regular(c.tile), c.tile.tag
            assert c.info["row"] % 64 in (63, 0, 1)
        else:
            assert sorted({r % 64 for r in c.info["rows"]}) == [0, 1, 63] and len(c.info["rows"]) == 9
    for L in (120, 420):
        for ev in wc.RING_EVENTS:
            rows = [c.info["row"] for c in ring if c.info["L"] == L and not c.info["chained"] and c.info["ev"] == ev]
            assert sorted(r % 64 for r in rows) == [0, 0, 1, 1, 63, 63] and sorted(r % 256 for r in rows if r > 200) == [0, 1, 255], (L, ev, rows)
    # every other engineered tile is regular too: all of them go to ring kernels
    assert all(rc.is_regular(c.tile) for c in cases if not c.info.get("chained"))
