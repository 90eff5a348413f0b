"""CPU: the port's restatement of the reference's SSE-path fill (fill_sse_semantics, oracle/convex_oracle.c) pinned to
fwdFillMatrixSSESimple itself, cell by cell, on the row-length families of tests/sse_row_cases.py -- every direction code, the
fill's score bits and its best cell, not only the alignments that survive validPath -- and the families' own purpose, asserted
on the port alone.  With the first test green the port is the device's cell-level oracle for tests/test_gpu_sse_rows.py."""
import numpy as np
import pytest

from oracle.pyoracle import Oracle, have_ref, same_alignment
from tests import sse_row_cases as rc
from tests import util

NO_SCORE = 0xBF800000      # the fill's start value -1: no cell scored above it, the best cell is whatever it was


@pytest.fixture(scope="module")
def cases():
    return rc.families()


def _fill_diff(port, ref, tile):
    ps, px, py, pd = port.fill(tile)
    rs, rx, ry, rd = ref.fill(tile)
    if len(pd) != len(rd):
        return "cell count %d != %d" % (len(pd), len(rd))
    if not np.array_equal(pd, rd):
        i = int(np.flatnonzero(pd != rd)[0])
        L = rc.clipped_lengths(tile)
        y = int(np.searchsorted(np.cumsum(L), i, side="right"))
        return "direction code at row %d (L %d) column %d: port %d, reference %d (%d cells differ)" % (
            y, int(L[y]), i - int(np.sum(L[:y])), int(pd[i]), int(rd[i]), int(np.sum(pd != rd)))
    if ps != rs:
        return "fill score bits %08x != %08x" % (ps, rs)
    if ps != NO_SCORE and (px, py) != (rx, ry):
        return "best cell (%d, %d) != (%d, %d)" % (px, py, rx, ry)
    return same_alignment(port.align(tile), ref.align(tile))


@pytest.mark.parametrize("k", range(len(rc.NON_DEFAULT) + 1))
def test_port_fill_equals_reference_fill_cell_by_cell(built, cases, k):
    """Every tile of every family under scoring k (the last k: the default): direction codes, score bits, best cell, alignment.
    Under the non-default scorings the zoo and the edge tiles as well."""
    if not have_ref():
        pytest.skip("oracle/_ref not built (no reference tree on this machine and no prebuilt library)")
    sc = rc.NON_DEFAULT[k] if k < len(rc.NON_DEFAULT) else rc.DEFAULT
    port, ref = Oracle("port", rc.params(sc)), Oracle("reference", rc.params(sc))
    tiles = [c.tile for c in cases]
    if k < len(rc.NON_DEFAULT):
        tiles = tiles + util.tile_zoo(seed=600 + k, n=24, max_w=600) + util.edge_tiles()
    bad = []
    for t in tiles:
        d = _fill_diff(port, ref, t)
        if d:
            bad.append((t.tag, d))
    assert not bad, (len(bad), bad[:6])


def test_families_do_what_they_are_for(built, cases):
    """No reference needed.  Conditions on the port, under the seeds of sse_row_cases.families():
    every tile has a positive fill score under every scoring (the device test compares the raw fill of every tile, and a fill
    score of -1 is what it would have to leave out); the seam, overlap and centre-path short (L >= 8) tiles are valid alignments
    under every EXOTIC scoring; under (2, -10, -5, -5, -1, 0.15) the raw fill of the SSE restatement differs from the scalar
    fill's in every `left` width, the alignments differ in every `seam` kind, and are equal wherever the whole row is
    recomputed (short, 5 <= L <= 12).  And the kinds land in the plan class they were written for."""
    for sc in rc.NON_DEFAULT + [rc.DEFAULT]:
        orc = Oracle("port", rc.params(sc))
        none = [c.tile.tag for c in cases if orc.fill(c.tile)[0] == NO_SCORE]
        assert not none, (sc, none[:5])
    for sc in rc.EXOTIC:
        orc = Oracle("port", rc.params(sc))
        invalid = [c.tile.tag for c in cases
                   if (c.family in ("seam", "overlap") or (c.family == "short" and c.L >= 8)) and orc.align(c.tile)["ret"] < 0]
        assert not invalid, (sc, invalid[:5])

    sse, spec = Oracle("port", rc.params(rc.SEPARATING)), Oracle("port", rc.params(rc.SEPARATING))
    spec.set_spec_fill(True)
    raw_differs, aln_differs = {}, {}
    for c in cases:
        a, b = sse.fill(c.tile), spec.fill(c.tile)
        raw_differs.setdefault((c.family, c.kind), []).append(a[:3] != b[:3])
        aln_differs.setdefault((c.family, c.kind), []).append(same_alignment(sse.align(c.tile), spec.align(c.tile)) is not None)
    for (family, kind), v in raw_differs.items():
        if family == "left":
            assert any(v), ("the two fills never separate", family, kind)
    for (family, kind), v in aln_differs.items():
        if family == "seam":
            assert any(v), ("the two alignments never separate", family, kind)
        if family == "short" and 5 <= int(kind[1:]) <= 12:
            assert not any(v), ("a wholly recomputed row told the fills apart", family, kind)

    # the aim of each kind: row lengths, the window's edges, the plan's class
    for c in cases:
        L = rc.clipped_lengths(c.tile)
        t = c.tile
        assert 150 <= t.H <= 250 and t.W <= 420
        inside = np.all(t.row_offset >= 0) and np.all(t.row_offset.astype(np.int64) + t.row_length <= t.W)
        assert inside == (c.family != "clipped"), t.tag
        if c.family == "clipped":
            n = len(rc.CLIP_UP)
            got = L[:n] if c.kind.endswith("head") else L[-n:][::-1]
            assert tuple(int(v) for v in got) == rc.CLIP_UP, (t.tag, got)
        elif c.L is not None:
            assert np.all(L == c.L), t.tag
        if rc.irregular_by_design(c):
            assert not rc.is_regular(t), t.tag
            if c.family == "steps":
                back = -np.diff(t.row_offset.astype(np.int64))
                assert {1, 2, 3} <= set(int(v) for v in back), t.tag
        elif c.family in ("short", "seam", "overlap", "steps") or (c.family == "left" and c.L is not None):
            assert rc.is_regular(t), t.tag
        if c.family == "steps" and not rc.irregular_by_design(c):
            assert {0, 1, 2} <= set(int(v) for v in np.diff(t.row_offset.astype(np.int64))), t.tag
    assert {int(v) for c in cases if c.family == "ragged" for v in rc.clipped_lengths(c.tile)} == {3, 4, 5, 8, 9, 10, 11, 12, 13, 16, 17}
