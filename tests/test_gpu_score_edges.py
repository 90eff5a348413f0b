"""GPU (-m gpu): the case families of tests/score_cases.py through the device's scoring kernels, against the reference's own
StrippedSW + ssw.c (ScoreOracle("reference"), oracle/_ref, when built) and the C restatement (ScoreOracle("port")).

cvx_score_submit dispatches per pair (score_diag_kernel, score_wave_kernel<1 | 2 | 4 | 8 | 16>, score_kernel); cvx_score_batch picks one
kernel for the call.  Every family goes through both, as one job each and all shuffled into one job with the 20 000 volume pairs,
so that all seven classes launch from one enqueue and the results travel back through the job's order table.  What a family claims
(closed-form scores, a gapped path that beats every ungapped run) is asserted on the ORACLE's scores; the device must then equal
the oracle on every pair.  Integer scores: bit-exact, no pair excluded."""
import collections
import os

import numpy as np
import pytest

from tests import score_cases as sc
from tests.test_gpu_score import _oracle_scores_threaded

pytestmark = pytest.mark.gpu

NAMES = list(sc.FAMILIES)
_want = {}


def _kinds():
    from oracle.pyoracle import have_score_ref
    return ["port", "reference"] if have_score_ref() else ["port"]


def _oracle(name, kind):
    if (name, kind) not in _want:
        refs, qrys, _ = sc.family(name)
        _want[(name, kind)] = _oracle_scores_threaded(refs, qrys, kind=kind)
    return _want[(name, kind)]


def _equal(got, want, metas, what):
    assert got.dtype == np.float32 and len(got) == len(want)
    bad = np.nonzero(got != want)[0]
    assert np.array_equal(got, want), (what, len(bad), [(metas[i], float(got[i]), float(want[i])) for i in bad[:8]])


def _check_family(got, name, what, idx=None):
    _, _, metas = sc.family(name)
    for kind in _kinds():
        want = _oracle(name, kind)
        if idx is not None:
            _equal(got, want[idx], [metas[i] for i in idx], (name, what, kind))
        else:
            _equal(got, want, metas, (name, what, kind))


@pytest.fixture(scope="module")
def scorer(built):
    from ngmlr_amd.aligner import StrippedSWHip
    sw = StrippedSWHip(device=0)
    yield sw
    sw.close()


@pytest.fixture(scope="module")
def scorer_no_diag(built):
    """A handle of its own that never uses score_diag_kernel: cvx_score_batch then takes score_reg_kernel<5> / <8> / score_kernel by
    the call's longest reference, cvx_score_submit sends the short pairs to the wave kernels."""
    from ngmlr_amd.aligner import StrippedSWHip
    os.environ["CVX_TUNE_SCORE_NO_DIAG"] = "1"
    try:
        sw = StrippedSWHip(device=0)
    finally:
        del os.environ["CVX_TUNE_SCORE_NO_DIAG"]
    yield sw
    sw.close()


def _groups(metas):
    """c_reg: the index lists of the pairs that travel in one cvx_score_batch call (one longest reference, one orientation)."""
    out = collections.OrderedDict()
    for i, m in enumerate(metas):
        out.setdefault((m.get("group"), m["orient"] if "group" in m else None), []).append(i)
    return list(out.values())


@pytest.mark.parametrize("name", NAMES)
def test_family_properties_hold_on_the_oracles(built, name):
    """What the device is compared with has the property the family was built for (on this box's oracles, both kinds)."""
    refs, qrys, metas = sc.family(name)
    for kind in _kinds():
        paying = sc.check_properties(_oracle(name, kind), refs, qrys, metas)
        if name in ("a", "b", "d"):
            assert paying == len(refs)
    if name in sc.AIMED:
        assert sc.AIMED[name] <= {m["cls"] for m in metas}


@pytest.mark.parametrize("name", NAMES)
def test_family_as_one_job(scorer, name):
    refs, qrys, _ = sc.family(name)
    _check_family(scorer.submit_scores(refs, qrys).wait(), name, "submit")


@pytest.mark.parametrize("name", NAMES)
def test_family_through_batch_score(scorer, name):
    refs, qrys, metas = sc.family(name)
    for idx in _groups(metas):
        _check_family(scorer.batch_score([refs[i] for i in idx], [qrys[i] for i in idx]), name, "batch", idx)


@pytest.mark.parametrize("name", ["c", "c_rows", "c_reg", "e", "f"])
def test_family_without_the_diagonal_kernel(scorer_no_diag, name):
    """score_reg_kernel<5> (longest reference 320 with its NUL), <8> (321, 512), score_kernel (513 and above) through
    cvx_score_batch; through cvx_score_submit the pairs the diagonal kernel would take go to the wave kernels."""
    refs, qrys, metas = sc.family(name)
    for idx in _groups(metas):
        _check_family(scorer_no_diag.batch_score([refs[i] for i in idx], [qrys[i] for i in idx]), name, "batch, no diag", idx)
    _check_family(scorer_no_diag.submit_scores(refs, qrys).wait(), name, "submit, no diag")


def test_volume_pairs(scorer):
    """Family (h): 20 000 pairs, every wave class and the diagonal kernel, scores from 0 to above 255; as one job, as five jobs in
    flight, and through cvx_score_batch in calls of 4 096."""
    refs, qrys, metas = sc.family("h")
    n = len(refs)
    reached = collections.Counter(m["cls"] for m in metas)
    for k in sc.WAVE_K:
        assert reached["wave%d" % k] >= n // 10, reached
    assert reached["diag"] > 0
    assert (_oracle("h", "port") > 255).sum() >= n // 20
    whole = scorer.submit_scores(refs, qrys)
    cuts = [0, n // 7, n // 3, n // 2, (4 * n) // 5, n]
    jobs = [scorer.submit_scores(refs[a:b], qrys[a:b]) for a, b in zip(cuts, cuts[1:])]
    _check_family(whole.wait(), "h", "submit")
    _check_family(np.concatenate([j.wait() for j in jobs]), "h", "submit, five jobs in flight")
    got = np.concatenate([scorer.batch_score(refs[lo:lo + 4096], qrys[lo:lo + 4096]) for lo in range(0, n, 4096)])
    _check_family(got, "h", "batch")


def test_all_families_shuffled_into_one_job(scorer):
    """All seven classes from one enqueue; the scores come back in the caller's order."""
    names = NAMES + ["h"]
    refs, qrys, metas, wants = [], [], [], {k: [] for k in _kinds()}
    for name in names:
        r, q, m = sc.family(name)
        refs += r; qrys += q; metas += m
        for kind in wants:
            wants[kind].append(_oracle(name, kind))
    perm = np.random.default_rng(163).permutation(len(refs))
    refs, qrys, metas = [refs[i] for i in perm], [qrys[i] for i in perm], [metas[i] for i in perm]
    assert {m["cls"] for m in metas} == set(sc.CLASSES)
    got = scorer.submit_scores(refs, qrys).wait()
    for kind, parts in wants.items():
        _equal(got, np.concatenate(parts)[perm], metas, ("all families, one job", kind))


def test_small_single_class_jobs(scorer):
    """Jobs of 1, 3, 4 and 5 pairs of one class: four pairs per workgroup, so a last workgroup with one, three, four and one live
    waves; all of them in flight at once."""
    refs, qrys, metas = sc.all_deterministic()
    wants = {kind: np.concatenate([_oracle(name, kind) for name in NAMES]) for kind in _kinds()}
    by_class = collections.defaultdict(list)
    for i, m in enumerate(metas):
        if m["family"] != "g":                         # (the 100 000-character pairs have their own tests)
            by_class[m["cls"]].append(i)
    assert set(by_class) == set(sc.CLASSES)
    rng = np.random.default_rng(167)
    jobs = []
    for cls in sc.CLASSES:
        for n in (1, 3, 4, 5):
            idx = [int(i) for i in rng.choice(by_class[cls], size=n, replace=False)]
            jobs.append((cls, idx, scorer.submit_scores([refs[i] for i in idx], [qrys[i] for i in idx])))
    for cls, idx, job in jobs:
        got = job.wait()
        for kind, want in wants.items():
            _equal(got, want[idx], [metas[i] for i in idx], ("single class", cls, len(idx), kind))
