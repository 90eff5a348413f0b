"""GPU (-m gpu): the FAST form of the ring fill (cvx_fill_ring.inc: a table of {penalty, next address} pairs, the run register of
a cell loaded with its penalty -- no add per cell, no periodic clamp) against the unchanged arithmetic form and the oracle.  Every
tile runs on a default handle and on a handle with the penalty table switched off (CVX_TUNE_PEN_TABLE=0); every result record and
every op must be equal between the two, and the alignments equal to the oracle's (the reference itself where oracle/_ref is built).

Shapes, the smallest that reach each mechanism (H read rows, w corridor columns): H = 40 on 330 columns (one slot per lane, no
hand-over); H = 260 and 420 on 309 / 340 / 369 columns (three slots per lane, the ring wraps); 420 columns (four slots per lane);
H = 700 (the exactly tracked tail starts while rows still start); and two engineered tiles whose gap run passes through 64
consecutive zero-score cells -- past the run from which the table's next address saturates -- one as a deletion, one as an insertion.
Scorings: the default (PacBio), the ont preset's values, a mismatch of 0 (not the rings' sign structure: the catch-all kernel, on
both handles) and a gap_open equal to the first extension penalty: exact-zero sums and ties."""
import re

import numpy as np
import pytest

from ngmlr_amd import synth
from ngmlr_amd.aligner import ConvexAlignHip
from oracle.pyoracle import Oracle, have_ref, same_alignment

pytestmark = pytest.mark.gpu

F32 = np.float32
SCORINGS = [
    dict(match=2.0, mismatch=-5.0, gap_open=-5.0, gap_extend=-5.0, gap_extend_min=-1.0, gap_decay=0.15),
    dict(match=1.0, mismatch=-1.0, gap_open=-1.0, gap_extend=-1.0, gap_extend_min=-0.5, gap_decay=0.15),      # src/ArgParser.cpp:261-265
    dict(match=2.0, mismatch=0.0, gap_open=-5.0, gap_extend=-5.0, gap_extend_min=-1.0, gap_decay=0.15),
    dict(match=2.0, mismatch=-5.0, gap_open=float(F32(F32(-5.0) + F32(0.15))), gap_extend=-5.0, gap_extend_min=-1.0, gap_decay=0.15),
]
ZERO_RUN = 64      # > kPenClamp (56), >= the 60 cells asked for


def _read_tile(rng, H, w, tag):
    """a read of exactly H bases (15 % error) on a corridor of w columns around the line through the window's corners"""
    ref = synth.random_ref(rng, H + 64)
    qry = synth.mutate(rng, ref, 0.15)
    assert len(qry) >= H
    W = max(8, int(round(len(ref) * H / len(qry))))
    ref, qry = ref[:W], qry[:H]
    _, k, d, _, _, _ = synth.anchors_desc(H, W)
    off, ln = synth.affine_rows(H, k, d, float(F32(w) * F32(0.505)), w)
    return synth.Tile(ref=ref.tobytes(), qry=qry.tobytes(), row_offset=off, row_length=ln, tag=tag)


def _zero_run_tile(rng, ins):
    """Six leading bases that score exactly -gap_open under the default scoring (four matches, a mismatch, a match: 5), then ZERO_RUN
    bases of 'T' on one side only, then a clean flank.  The gap opens with score 0 off the sixth cell and runs through ZERO_RUN
    zero-score cells (no 'T' in the leading bases: every other candidate there is negative); the flank's alignment starts from the
    run's last cell, so the backtrack walks the whole run."""
    n_flank = 130 if ins else 150      # three slots per lane either way
    flank = synth.random_ref(rng, n_flank)
    flank[0] = ord("A")
    gap = np.full(ZERO_RUN, ord("T"), dtype=np.uint8)
    lead_ref, lead_qry = np.frombuffer(b"ACGACG", dtype=np.uint8), np.frombuffer(b"ACGAAG", dtype=np.uint8)
    ref = np.concatenate([lead_ref, flank] if ins else [lead_ref, gap, flank])
    qry = np.concatenate([lead_qry, gap, flank] if ins else [lead_qry, flank])
    off, ln = synth.corridor_full(len(qry), len(ref))
    return synth.Tile(ref=ref.tobytes(), qry=qry.tobytes(), row_offset=off, row_length=ln, tag="zero run %s" % ("I" if ins else "D"))


def _tiles():
    rng = np.random.default_rng(1717)
    tiles = [_read_tile(rng, 40, 330, "H40 w330")]
    for H in (260, 420):
        for w in (309, 340, 369):
            tiles.append(_read_tile(rng, H, w, "H%d w%d" % (H, w)))
    tiles.append(_read_tile(rng, 420, 420, "H420 w420"))
    tiles.append(_read_tile(rng, 700, 340, "H700 w340"))
    tiles.append(_zero_run_tile(rng, False))
    tiles.append(_zero_run_tile(rng, True))
    return tiles


def _run(tiles, sc):
    al = ConvexAlignHip(device=0, **sc)
    batch = al.upload(tiles)
    batch.run()
    launches = batch.launches()
    res, ops = batch.download()
    recs = []
    for r in res[:len(tiles)]:
        recs.append(((int(np.float32(r.score).view(np.uint32)), r.status, r.best_ref_index, r.best_read_index, r.ref_position, r.qstart, r.qend, r.n_ops),
                     ops[int(r.ops_begin):int(r.ops_begin) + int(r.n_ops)].tolist()))
    got = batch.alignments()
    batch.free()
    al.close()
    return recs, got, launches


@pytest.mark.parametrize("k", range(len(SCORINGS)))
def test_fast_form_equals_arithmetic_form_and_oracle(built, monkeypatch, k):
    sc = SCORINGS[k]
    params = (sc["match"], sc["mismatch"], sc["gap_open"], sc["gap_extend"], sc["gap_extend_min"], sc["gap_decay"])
    tiles = _tiles()
    fast, got, launches = _run(tiles, sc)
    monkeypatch.setenv("CVX_TUNE_PEN_TABLE", "0")
    plain, got_plain, _ = _run(tiles, sc)
    monkeypatch.delenv("CVX_TUNE_PEN_TABLE")
    if k != 2:
        assert {li["slots_per_lane"] for li in launches} >= {1, 3, 4}, launches
        assert all(li["wrap16"] == 0 for li in launches)
    bad = [(t.tag, a[0], b[0]) for t, a, b in zip(tiles, fast, plain) if a != b]
    assert not bad, bad[:4]
    orc = Oracle("reference" if have_ref() else "port", params)
    for t, g, gp in zip(tiles, got, got_plain):
        assert g["status"] != -1, t.tag
        want = orc.align(t)
        assert same_alignment(want, g) is None, (t.tag, same_alignment(want, g))
        assert same_alignment(want, gp) is None, (t.tag, same_alignment(want, gp))
    assert sum(1 for g in got if g["ret"] >= 0) >= len(tiles) - 1
    if k == 0:
        # the engineered runs are in the alignments, whole
        for g, op in ((got[-2], "D"), (got[-1], "I")):
            runs = [int(m) for m in re.findall(r"(\d+)" + op, g["cigar"])]
            assert runs and max(runs) >= ZERO_RUN, g["cigar"]
