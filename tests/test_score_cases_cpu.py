"""CPU: the case families of tests/score_cases.py on the two scoring oracles.  The C restatement (oracle/score_oracle.c) must equal
the reference's own StrippedSW + ssw.c (oracle/_ref) on every pair -- gaps that pay at every row phase, best paths ending in the
last row and column, an insertion next to a deletion (the adjacency ssw's lazy-F loop forbids), every byte 1 .. 127, the length
limit -- and the families must have the properties they were built for: the closed-form scores, a gapped path that beats the best
ungapped run on every pair that claims one, the same score in both orientations, and pairs in every kernel class they aim at."""
import collections

import numpy as np
import pytest

from tests import score_cases as sc
from tests.test_gpu_score import _oracle_scores_threaded

H_CPU = 4000


def _port(name):
    refs, qrys, metas = sc.family(name)
    return _oracle_scores_threaded(refs, qrys, kind="port"), refs, qrys, metas


@pytest.mark.parametrize("name", list(sc.FAMILIES))
def test_port_equals_reference_on_family(built, name):
    from oracle.pyoracle import have_score_ref
    if not have_score_ref():
        pytest.skip("oracle/_ref/libscore_oracle_ref.so not built")
    port, refs, qrys, metas = _port(name)
    ref = _oracle_scores_threaded(refs, qrys, kind="reference")
    bad = np.nonzero(port != ref)[0]
    assert len(bad) == 0, [(metas[i], float(port[i]), float(ref[i])) for i in bad[:5]]


def test_port_equals_reference_on_volume_pairs(built):
    from oracle.pyoracle import have_score_ref
    if not have_score_ref():
        pytest.skip("oracle/_ref/libscore_oracle_ref.so not built")
    refs, qrys, metas = sc.family_h(n=H_CPU)
    port = _oracle_scores_threaded(refs, qrys, kind="port")
    ref = _oracle_scores_threaded(refs, qrys, kind="reference")
    bad = np.nonzero(port != ref)[0]
    assert len(bad) == 0, [(metas[i], float(port[i]), float(ref[i])) for i in bad[:5]]


@pytest.mark.parametrize("name", list(sc.FAMILIES))
def test_family_properties(built, name):
    """Closed forms, gap-pays on every pair with a floor, orientation symmetry, and the classes the family names."""
    want, refs, qrys, metas = _port(name)
    assert len(refs) == len(qrys) == len(metas) and len(refs) % 2 == 0
    paying = sc.check_properties(want, refs, qrys, metas)
    assert np.array_equal(want[0::2], want[1::2])                # the recurrence is symmetric in the two strings
    for i in range(0, len(refs), 2):
        assert refs[i] == qrys[i + 1] and qrys[i] == refs[i + 1]
        assert metas[i]["orient"] == "qry_short" and metas[i + 1]["orient"] == "ref_short" and len(qrys[i]) <= len(refs[i])
    reached = collections.Counter(m["cls"] for m in metas)
    if name in sc.AIMED:
        assert sc.AIMED[name] <= set(reached), (name, reached)
    if name in ("a", "b", "d"):
        assert paying == len(refs)                               # every pair of these families claims a gap, none left out
        assert set(reached) == sc.AIMED[name], reached
    if name == "a":
        assert len(refs) == 2 * 176
        phases_v = {m["a"] % 16 for m in metas if m["kind"] == "v"}
        assert phases_v == set(range(16))                        # the vertical gap's row: every phase of a lane's 16 rows
        assert {m["kind"] for m in metas} == {"h", "v"}
        margin = min(m["floor"] - max(m["parts"]) for m in metas)
        assert margin >= 40
    if name == "b":
        assert len(refs) == 2 * 130 and {m["j1"] for m in metas} == set(range(65))
    if name == "c":
        for k in sc.WAVE_K:
            assert {m["n"] + 1 for m in metas if m["k"] == k} >= {32 * k + 1, 64 * k - 1, 64 * k}
            assert {m["cls"] for m in metas if m["k"] == k} == {"wave%d" % k}
        assert {len(r) % 64 for r in refs[0::2]} >= {0, 1, 63}
        assert {m["where"] for m in metas} == {"start", "end"}
    if name in ("c_rows", "g"):
        assert all(m["cls"] == ("wave%d" % m["k"] if m["k"] else "rows") for m in metas)
    if name == "c_reg":
        for longest in sc.C_REG_LONGEST:
            grp = [i for i, m in enumerate(metas) if m["group"] == longest and m["orient"] == "qry_short"]
            assert max(len(refs[i]) + 1 for i in grp) == min(len(refs[i]) + 1 for i in grp) == longest
    if name == "d":
        assert {len(m["g"]) for m in metas} == {1, 2} and max(sum(m["g"]) for m in metas) == 4
        assert min(min(len(r), len(q)) for r, q in zip(refs, qrys)) > 1024
    if name == "g":
        assert (want == -1.0).sum() == len(refs) // 2


def test_thin_margin_pairs_sit_on_the_tie(built):
    """Family (a)'s thin cases: the gapped path's a + b - 255 g is within a few points of the best ungapped run (either side)."""
    want, refs, qrys, metas = _port("a_thin")
    for i in range(0, len(refs), 2):
        m = metas[i]
        assert abs(sum(m["parts"]) - 255 * sum(m["g"]) - max(m["parts"])) <= 2
        assert want[i] >= max(m["parts"])
        assert want[i] >= sc.ungapped_best(refs[i], qrys[i])


def test_volume_pairs_cover_every_wave_class(built):
    refs, qrys, metas = sc.family_h(n=H_CPU)
    assert (refs, qrys) == sc.family_h(n=H_CPU)[:2]              # seeded: the same draw every time
    reached = collections.Counter(m["cls"] for m in metas)
    for k in sc.WAVE_K:
        assert reached["wave%d" % k] >= H_CPU // 10, reached
    assert reached["diag"] > 0 and set(reached) <= set(sc.CLASSES)
    want = _oracle_scores_threaded(refs, qrys, kind="port")
    assert (want > 255).sum() >= H_CPU // 20 and (want == 0).sum() > 0
    assert {m["orient"] for m in metas} == {"qry_short", "ref_short"}


def test_expected_class_thresholds():
    assert sc.expected_class(2048, 512) == "diag" and sc.expected_class(2049, 512) == "wave8" and sc.expected_class(2048, 513) == "wave16"
    assert sc.expected_class(512, 2048) == "wave8"               # the diagonal kernel's condition is on the query
    assert sc.expected_class(300, 256, no_diag=True) == "wave4"
    for k in sc.WAVE_K:
        assert sc.expected_class(5000, 64 * k) == "wave%d" % k == sc.expected_class(64 * k, 5000)
        assert sc.expected_class(5000, 64 * k + 1) == ("wave%d" % (2 * k) if k < 16 else "rows")
    assert sc.expected_class(1, 1) == "diag" and sc.expected_class(4000, 1) == "wave1"


def test_ungapped_best_is_kadane_over_diagonals():
    assert sc.ungapped_best(b"", b"ACGT") == 0 and sc.ungapped_best(b"ACGT", b"ACGT") == 4
    assert sc.ungapped_best(b"ACGTACGT", b"ACGTGACGT") == 4      # one extra base: no run longer than a flank
    assert sc.ungapped_best(b"AAAACAAAA", b"AAAAGAAAA") == 7      # 4 - 1 + 4
    assert sc.ungapped_best(b"AAAANAAAA", b"aaaagaaaa") == 8      # N scores 0
    assert sc.ungapped_best(b"TTTT", b"uuuu") == 0 and sc.ungapped_best(b"AAAA", b"UUuu") == 4
