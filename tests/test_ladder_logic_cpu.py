"""CPU: the retry ladder's rule (ngmlr_amd/csrc/cvx_ladder_logic.h, the functions ladder_next_kernel runs) through cvx_ladder_rung
against the Python restatement of computeAlignment's loop on ngmlr_amd.synth's corridor builders (tests/ladder_cases.py), and
against what the unmodified reference did on its own data (tests/golden/ladder_*.npz, tools/make_golden_ladder.sh)."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

from tests import ladder_cases as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same_form(a, b):
    if a is None or b is None:
        return a is None and b is None
    return (a[0], a[4], a[5]) == (b[0], b[4], b[5]) and all(np.float32(x).tobytes() == np.float32(y).tobytes() for x, y in zip(a[1:4], b[1:4]))


@pytest.fixture(scope="module")
def cases(built):
    return lc.sweep()


def test_rule_equals_the_restatement_over_the_sweep(cases):
    from ngmlr_amd import capi
    bad = [(H, W, l, m, capi.ladder_rung(W, H, l, m), lc.rung_desc(H, W, l, m)) for H, W, l, m in cases
           if not _same_form(capi.ladder_rung(W, H, l, m), lc.rung_desc(H, W, l, m))]
    assert not bad, bad[:5]


def test_the_sweep_holds_what_it_must(cases):
    """fractions that separate (int) (left * m + right * m), each operation rounded to binary32, from (int) ((left + right) * m)
    taken exactly, corridor > 2 * ref_len, the cap
    cutting the ladder at every length 1 ... 5, FULL, and every builder at a rung beyond the first"""
    F32 = np.float32
    split = 0
    lengths = set()
    over = full = 0
    builders = set()
    for H, W, l, m in cases:
        corridor, left, right, flags = l
        if flags & lc.ANCHORS and not flags & (lc.REALIGN | lc.SHORT | lc.FULL) and m == 2:
            # (in binary32 the two orders agree at m = 2, the only multiplier the anchors form sees beyond 1: doubling is exact.
            # What separates them is the rounding of the sum: the rule's width against the sum taken exactly)
            a = int(np.trunc(F32(F32(F32(left) * F32(m)) + F32(F32(right) * F32(m)))))
            split += a != int(np.trunc((float(F32(left)) + float(F32(right))) * m))
        if not flags & lc.FULL:
            lengths.add(lc.ladder_length(W, l))
        over += corridor > lc.cap(W)
        full += bool(flags & lc.FULL)
        d = lc.rung_desc(H, W, l, m)
        if d is not None and m > 1 and H and W:
            builders.add("short" if flags & lc.SHORT else "anchors" if d[3] != 0.0 else "endpoints")
    assert split >= 20 and lengths == {1, 2, 3, 4, 5} and over > 100 and full > 100
    assert builders == {"short", "anchors", "endpoints"}


def test_the_ladder_ends_where_the_loop_ends(built):
    from ngmlr_amd import capi
    W = 999      # refSeqLen 1000: the cap is 2000
    for corridor, want in ((2001, 1), (2000, 1), (1001, 1), (1000, 2), (667, 2), (666, 3), (501, 3), (500, 4), (401, 4), (400, 5), (1, 5), (0, 5)):
        got = [capi.ladder_rung(W, 900, (corridor, 0.0, 0.0, 0), m) is not None for m in range(1, 8)]
        assert got == [m <= want for m in range(1, 8)], (corridor, got)
        assert [capi.ladder_rung(W, 900, (corridor, 0.0, 0.0, lc.FULL), m) is not None for m in range(1, 4)] == [True, False, False]
    # the clamp: a corridor beyond 2 * ref_len is 2 * ref_len
    assert _same_form(capi.ladder_rung(W, 900, (5000, 0.0, 0.0, 0), 1), capi.ladder_rung(W, 900, (2000, 0.0, 0.0, 0), 1))
    # anchors hand over to the endpoints form at rung 3, and at once under realign
    assert capi.ladder_rung(W, 900, (400, 150.0, 160.0, lc.ANCHORS), 2)[3] == 320.0
    assert _same_form(capi.ladder_rung(W, 900, (400, 150.0, 160.0, lc.ANCHORS), 3), capi.ladder_rung(W, 900, (400, 0.0, 0.0, 0), 3))
    assert _same_form(capi.ladder_rung(W, 900, (400, 150.0, 160.0, lc.ANCHORS | lc.REALIGN), 1), capi.ladder_rung(W, 900, (400, 0.0, 0.0, lc.REALIGN), 1))
    assert capi.ladder_rung(W, 900, (400, 0.0, 0.0, lc.REALIGN), 2)[5] == 800 and capi.ladder_rung(W, 900, (400, 0.0, 0.0, 0), 2)[5] == 200


def test_bad_arguments_are_refused(built):
    from ngmlr_amd import capi
    lib = capi.load()
    t = capi.CvxTile()
    t.ref_len, t.qry_len = 100, 90
    form = capi.CvxTile()

    def rc(ladder, m=1, tile=t, out=form):
        l = capi.CvxLadder(*ladder)
        return lib.cvx_ladder_rung(C.byref(tile) if tile is not None else None, C.byref(l), m, C.byref(out) if out is not None else None)
    assert rc((64, 0.0, 0.0, 0)) == 1 and rc((64, 0.0, 0.0, 0), 6) == 0
    assert rc((-1, 0.0, 0.0, 0)) == -3 and rc((64, 0.0, 0.0, 16)) == -3 and rc((64, 0.0, 0.0, 0), 0) == -3
    assert rc((64, float("nan"), 1.0, lc.ANCHORS)) == -3 and rc((64, 1.0, float("inf"), lc.ANCHORS)) == -3 and rc((64, -1.0, 1.0, lc.ANCHORS)) == -3
    assert rc((64, float("nan"), 1.0, 0)) == 1      # read only with ANCHORS
    assert rc((64, 0.0, 0.0, 0), tile=None) == -3 and rc((64, 0.0, 0.0, 0), out=None) == -3
    bad = capi.CvxTile()
    bad.ref_len, bad.qry_len = -1, 5
    assert rc((64, 0.0, 0.0, 0), tile=bad) == -3


def test_the_other_fields_of_the_form_are_left_alone(built):
    from ngmlr_amd import capi
    lib = capi.load()
    t = capi.CvxTile()
    t.ref_len, t.qry_len = 100, 90
    form = capi.CvxTile()
    form.ref_len, form.qry_len, form.row_stride_bytes, form.reserved = 7, 8, 16, 9
    l = capi.CvxLadder(64, 0.0, 0.0, 0)
    assert lib.cvx_ladder_rung(C.byref(t), C.byref(l), 2, C.byref(form)) == 1
    assert (form.ref_len, form.qry_len, form.row_stride_bytes, form.reserved) == (7, 8, 16, 9) and form.corridor_width == 32


GOLDEN = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "ladder_*.npz")))


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p) for p in GOLDEN])
def test_rule_equals_the_recorded_reference(built, path):
    """Every attempt of every computeAlignment call the unmodified reference made on the workload: the corridor it built
    (first row, last row, width) is rung m's form, and the ladder is as long as the rule makes it from the recorded return values."""
    from ngmlr_amd import capi, synth
    z = np.load(path)
    calls, attempts = z["calls"], z["attempts"]
    assert len(calls) > 0 and len(attempts) >= len(calls)
    at = 0
    for c in calls:
        corridor, H, ref_seq_len, realign, full, short, anchors, n_att, read_len_full = (int(c[k]) for k in ("corridor", "read_length", "ref_len", "realign", "full", "short_read", "anchor_length", "n_attempts", "full_read_length"))
        W = ref_seq_len - 1      # the tile's ref_len is strlen(refSeq); computeAlignment's refSeqLen counts one more (:209)
        flags = (lc.ANCHORS if anchors > 0 else 0) | (lc.REALIGN if realign else 0) | (lc.SHORT if short else 0) | (lc.FULL if full else 0)
        ladder = (corridor, float(c["left"]), float(c["right"]), flags)
        mine = attempts[at:at + n_att]
        at += n_att
        resolved = False
        for j, a in enumerate(mine):
            m = j + 1
            assert int(a["multiplier"]) == m and not resolved
            form = capi.ladder_rung(W, H, ladder, m)
            assert form is not None, (ladder, m)
            assert form[5] == int(a["width"]), (ladder, m, form, a)
            off, ln = lc.rung_rows(H, form)
            assert (int(off[0]), int(off[H - 1])) == (int(a["off_first"]), int(a["off_last"])), (ladder, m, form, a)
            resolved = int(a["ret"]) == read_len_full      # validAlignment = cigarLength == fullReadLength (:415)
        # the loop went on exactly while an attempt failed and a further rung existed
        assert resolved or capi.ladder_rung(W, H, ladder, n_att + 1) is None, (ladder, n_att)
