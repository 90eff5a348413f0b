"""GPU (-m gpu): the chained row-block fill -- the kFillChain form of fill_ring_kernel / fill_ring_twin_kernel (cvx_fill_ring.inc),
planned by plan_chain_tile (cvx_host_logic.h), merged by chain_reduce_kernel -- on the script-written families of
tests/chain_cases.py: a gap run across a block boundary with a known split, a block start on every phase of a direction word
and of a chunk of boundary records, the row above a block cut by the window, equal maxima in two and in many blocks, a last
block of one row.

Every block height (CVX_TUNE_MAX_M=1 with CVX_TUNE_CHAIN_M = 1, 2, 4: 64, 128 and 256 rows, the families written for that
height), the int16-run instantiations, a scalar-twin handle, the ont scoring, and the grouped and the one-wave walk across the
per-block regions of direction words.  Every tile against the port oracle (alignment, raw fill score bits and best cell, valid
or not), the dense ops of every valid tile against the script it was written from, records and ops byte for byte against a
handle without a knob, which takes the same tiles as whole rings.  The families are pinned to what they are for by
tests/test_chain_cases_cpu.py.

A tile with status -1 gave up waiting for a boundary record: a finding, to be read out of the code.

About 280 tiles of at most 600 x 300 cells per form, four of 4 400 x 200 at 64-row blocks; one batch per family."""
import numpy as np
import pytest

from ngmlr_amd import capi
from ngmlr_amd.aligner import ConvexAlignHip, format_alignment
from oracle.pyoracle import COMPARE_KEYS, Oracle, same_alignment
from tests import chain_cases as cc
from tests.twin_cases import TWIN_KEYS

pytestmark = pytest.mark.gpu

CVX_LAUNCH_WHOLE, CVX_LAUNCH_CHAINED = 0, 2
PLAN_DTYPE = np.dtype([("r0", np.int32), ("rend", np.int32), ("need", np.int32), ("flags", np.int32), ("cells", np.uint64), ("active", np.uint64)])

# name -> (N, knobs beside CVX_TUNE_MAX_M=1 / CVX_TUNE_CHAIN_M=N / 64, handle kind, families)
FORMS = {
    "m1": (64, {}, "default", cc.FAMILIES),
    "m2": (128, {}, "default", cc.FAMILIES),
    "m4": (256, {}, "default", cc.FAMILIES),
    "m1 wrap16": (64, {"CVX_TUNE_FORCE_WRAP16": "1"}, "default", cc.FAMILIES),
    "m4 wrap16": (256, {"CVX_TUNE_FORCE_WRAP16": "1"}, "default", cc.FAMILIES),
    "m1 twin": (64, {}, "twin", cc.FAMILIES),
    "m2 twin": (128, {}, "twin", cc.FAMILIES),
    "m1 ont": (64, {}, "ont", cc.FAMILIES),
    "m1 walk 8": (64, {"CVX_TUNE_BT_GROUP": "8"}, "default", ("cross", "brow", "clip")),
    "m1 walk 64": (64, {"CVX_TUNE_BT_GROUP": "64"}, "default", ("cross", "brow", "clip")),
}
# handle kind -> (scoring, scalar twin)
KINDS = {"default": (cc.DEFAULT, False), "twin": (cc.DEFAULT, True), "ont": (cc.ONT, False)}


class Item:
    """one tile of a batch: its case and what the oracle of the handle's kind says"""
    def __init__(self, orc, case, with_script):
        self.case, self.tile = case, case.tile
        self.ops = case.ops if with_script else None
        self.want = orc.align(case.tile)
        self.fwd = orc.last_fwd()
        self.fill_bits = orc.last_fill_score_bits()


_ITEMS, _WHOLE = {}, {}


def _items(built, N, kind):
    """family -> [Item] of families(N) for a handle kind, once per module.  default / twin: the default-scoring cases (the twin
    against the scalar recurrence, which these x-free tiles share with ConvexAlignFast's fill: tests/test_gpu_twin.py); ont: every
    tile under the ont scoring, the script's ops where the case was written for that scoring."""
    if (N, kind) not in _ITEMS:
        sc, twin = KINDS[kind]
        orc = Oracle("port", cc.params(sc))
        orc.set_spec_fill(twin)
        out = {}
        for c in cc.families(N):
            if kind == "ont" or c.scoring is cc.DEFAULT:
                out.setdefault(c.family, []).append(Item(orc, c, c.scoring is sc))
        _ITEMS[(N, kind)] = out
    return _ITEMS[(N, kind)]


def _run(tiles, kind, env):
    """one batch on a fresh handle (the knobs are read when a handle is created)
    -> (alignment dicts, (record bytes, ops) per tile, timing, launches, plan records)"""
    sc, twin = KINDS[kind]
    with pytest.MonkeyPatch.context() as mp:
        for k, v in env.items():
            mp.setenv(k, v)
        al = ConvexAlignHip(device=0, scalar_twin=twin, **sc)
    batch = al.upload(tiles)
    try:
        tm = batch.run()
        launches = batch.launches()
        res, ops = batch.download()
        plan = np.zeros(len(tiles), dtype=PLAN_DTYPE)
        capi.check(al.lib.cvx_batch_plan(batch.b, 0, len(tiles), plan.ctypes.data))
        recs = [(bytes(res[i]), ops[int(res[i].ops_begin):int(res[i].ops_begin) + int(res[i].n_ops)].tolist()) for i in range(len(tiles))]
        got = [format_alignment(al.lib, res[i], ops, tiles[i], scalar_twin=twin) for i in range(len(tiles))]
    finally:
        batch.free()
        al.close()
    return got, recs, tm, launches, plan


def _whole(key, tiles, kind):
    """the records of the same batch on a handle without a knob: whole tiles on rings, once per module"""
    if key not in _WHOLE:
        _, recs, tm, launches, _ = _run(tiles, kind, {})
        assert tm.n_tiles_chained == 0 and {li["kind"] for li in launches} == {CVX_LAUNCH_WHOLE}, (key, launches)
        _WHOLE[key] = recs
    return _WHOLE[key]


def differences(items, got, recs, whole, keys):
    """-> [(tag, first difference)] of a batch: against the oracle, the script and the whole-ring fill"""
    bad = []
    for it, g, (rec, ops), w in zip(items, got, recs, whole):
        want = it.want
        d = None
        if g["status"] == -1:
            d = "status -1: a block gave up waiting for a boundary record"
        elif same_alignment(want, g, keys=keys) is not None:
            d = same_alignment(want, g, keys=keys)
        elif it.fill_bits != 0xBF800000 and g["status"] not in (4, 5):      # (no positive score / never filled: nothing to compare)
            if g["fwd_score_bits"] != it.fill_bits:
                d = "raw fill score %08x, port %08x" % (g["fwd_score_bits"], it.fill_bits)
            elif (g["best_x"], g["best_y"]) != (it.fwd["best_x"], it.fwd["best_y"]):
                d = "best cell (%d, %d), port (%d, %d)" % (g["best_x"], g["best_y"], it.fwd["best_x"], it.fwd["best_y"])
        if d is None and want["ret"] >= 0 and it.ops is not None and ops != it.ops:
            d = "dense ops %r, script %r" % (ops[-6:], it.ops[-6:])
        if d is None and (rec, ops) != w:
            d = "record or ops differ from the whole-ring fill's"
        if d:
            bad.append((it.tile.tag, d))
    return bad


@pytest.mark.parametrize("form", list(FORMS))
def test_every_family_in_every_chained_form(built, form):
    N, knobs, kind, fams = FORMS[form]
    M = N // 64
    env = dict(knobs, CVX_TUNE_MAX_M="1", CVX_TUNE_CHAIN_M=str(M))
    wrap = int(knobs.get("CVX_TUNE_FORCE_WRAP16", "0"))
    keys = TWIN_KEYS if KINDS[kind][1] else COMPARE_KEYS
    items = _items(built, N, kind)
    assert set(items) == set(cc.FAMILIES)
    n_scripts = 0
    for fam in fams:
        its = items[fam]
        tiles = [it.tile for it in its]
        whole = _whole((N, kind, fam), tiles, kind)
        got, recs, tm, launches, plan = _run(tiles, kind, env)
        # the batch ran where it was aimed: every tile as row blocks of N rows, in the instantiation the knobs select
        assert [(li["kind"], li["slots_per_lane"], li["wrap16"], li["n_tiles"]) for li in launches] == [(CVX_LAUNCH_CHAINED, M, wrap, len(tiles))], (fam, launches)
        assert tm.n_tiles_chained == len(tiles), (fam, tm.n_tiles_chained)
        assert sum(li["waves"] for li in launches) == sum((t.H + N - 1) // N for t in tiles)      # (a chained launch reports its row-block tasks)
        if fam == "phase":
            # block 1's first cell behind the tile's first step, from the device's own plan record and the rows as uploaded
            for it, p in zip(its, plan):
                first, _, _ = cc.first_steps(it.tile)
                assert int(first[N] - p["r0"]) % 32 == it.case.info["residue"] and int(first[N] - p["r0"]) == 2 * N + it.case.info["d"], it.tile.tag
        bad = differences(its, got, recs, whole, keys)
        assert not bad, (form, fam, len(bad), bad[:8])
        n_scripts += sum(it.want["ret"] >= 0 and it.ops is not None for it in its)
        if fam == "phase":
            assert sum(it.want["ret"] < 0 and it.fill_bits != 0xBF800000 for it in its) >= 75      # the rejected paths: the raw fill result alone
    assert n_scripts >= (40 if kind == "ont" else 90), n_scripts      # (ont: the cross cases written for that scoring)
