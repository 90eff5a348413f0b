"""GPU (-m gpu): every lanes-per-tile form of the backtrack walk -- backtrack_grp_kernel<4 | 8 | 16 | 32> and the one-wave walk
backtrack_kernel (cvx_kernels.hip), chosen with CVX_TUNE_BT_GROUP -- on the script-written families of tests/walk_cases.py: a gap
at lane 0, 1 and G - 1 of a probe, an insertion that ends on the probe's last lane, a deletion that ends at the edge of a
direction word, sub-runs on every lane, the validPath band met inside a gap follow, rows that wrap in the ring or lie in two
chained row blocks, and waves shared with tiles that are not walked at all.

Every tile against the port oracle (alignment, raw fill score, best cell), the device's dense ops of every valid tile against the
script the tile was written from, and records and ops byte for byte against the 64-lane walk of the same batch.  The families are
pinned to what they are for by tests/test_walk_cases_cpu.py.

About 470 tiles of 80 - 470 rows per form, one batch per family."""
import numpy as np
import pytest

from ngmlr_amd import synth
from ngmlr_amd.aligner import ConvexAlignHip, format_alignment
from oracle.pyoracle import Oracle, same_alignment
from tests import util
from tests import walk_cases as wc

pytestmark = pytest.mark.gpu

FORMS = (4, 8, 16, 32, 64)
FAMILIES = ("lane", "word", "subrun", "band", "ring")
ENV = "CVX_TUNE_BT_GROUP"


@pytest.fixture(scope="module")
def cases():
    return wc.families()


class Item:
    """one tile of a batch: what the oracle says, and the script's ops where the tile was written from one"""
    def __init__(self, orc, tile, ops=None):
        self.tile, self.ops = tile, ops
        self.want = orc.align(tile)
        self.fwd = orc.last_fwd()
        self.fill_bits = orc.last_fill_score_bits()


@pytest.fixture(scope="module")
def mild_oracle(built):
    return Oracle("port", wc.params(wc.MILD))


@pytest.fixture(scope="module")
def batches(cases, port_oracle, mild_oracle):
    return make_batches(cases, port_oracle, mild_oracle)


def make_batches(cases, port_oracle, mild_oracle):
    """name -> (scoring, [Item]): one batch per family, the mild-scoring sub-run cases on their own, the share compositions"""
    out = {}
    for f in FAMILIES:
        out[f] = (wc.DEFAULT, [Item(port_oracle, c.tile, c.ops) for c in cases if c.family == f and c.scoring == wc.DEFAULT])
    out["subrun mild"] = (wc.MILD, [Item(mild_oracle, c.tile, c.ops) for c in cases if c.scoring == wc.MILD])
    assert sum(len(v[1]) for v in out.values()) == len(cases) and len(out["subrun mild"][1]) == 3
    # share: the last wave of a form holds one tile (1, 2 and 17 tiles: 17 = 16 + 1 = 2 * 8 + 1 = 4 * 4 + 1 = 8 * 2 + 1) ...
    lane = out["lane"][1]
    pick = lane[::9][:17]
    for n in (1, 2, 17):
        out["share %d" % n] = (wc.DEFAULT, pick[:n])
    # ... and tiles that are never walked, or end at once, in one wave with valid tiles four times their length
    edge = {t.tag: t for t in util.edge_tiles()}
    odd = [edge["all-mismatch"], wc.empty_tile(), edge["tiny1x40"], edge["tiny1x1"], edge["narrow"]]
    mixed = []
    for k, t in enumerate(odd):
        mixed.append(Item(port_oracle, t))
        long_tile, ops = wc.long_valid(np.random.default_rng([77, k]), max(4 * t.H, 150), "share long %d" % k)
        mixed.append(Item(port_oracle, long_tile, ops))
    assert all(m.want["ret"] >= 0 for m in mixed[1::2]) and sum(m.want["ret"] < 0 for m in mixed[0::2]) >= 4
    out["share mixed"] = (wc.DEFAULT, mixed)
    return out


def _run(tiles, sc, n=None):
    """one batch on a fresh handle (the lanes-per-tile setting is read when a handle is created)
    -> (alignment dicts, (record bytes, ops) per tile) of its first n tiles, the number of tiles that ran as chained row blocks"""
    n = len(tiles) if n is None else n
    al = ConvexAlignHip(device=0, **sc)
    batch = al.upload(tiles)
    try:
        tm = batch.run()
        res, ops = batch.download()
        recs = [(bytes(res[i]), ops[int(res[i].ops_begin):int(res[i].ops_begin) + int(res[i].n_ops)].tolist()) for i in range(n)]
        got = [format_alignment(al.lib, res[i], ops, tiles[i]) for i in range(n)]
    finally:
        batch.free()
        al.close()
    return got, recs, tm.n_tiles_chained


_WAVE = {}


def _wave_walk(key, tiles, sc, n=None):
    """the 64-lane walk's records of a batch, once per module"""
    if key not in _WAVE:
        with pytest.MonkeyPatch.context() as mp:
            mp.setenv(ENV, "64")
            _WAVE[key] = _run(tiles, sc, n)[1]
    return _WAVE[key]


def differences(items, got, recs, wave):
    """-> [(tag, first difference)] of a batch: against the oracle, the script and the 64-lane walk"""
    bad = []
    for it, g, (rec, ops), w in zip(items, got, recs, wave):
        want = it.want
        d = None
        if g["status"] == -1:
            d = "fell outside every device kernel"
        elif same_alignment(want, g) is not None:
            d = same_alignment(want, g)
        elif it.fill_bits != 0xBF800000 and g["status"] not in (4, 5):      # (no positive score / never filled: nothing to compare)
            if g["fwd_score_bits"] != it.fill_bits:
                d = "raw fill score %08x, port %08x" % (g["fwd_score_bits"], it.fill_bits)
            elif (g["best_x"], g["best_y"]) != (it.fwd["best_x"], it.fwd["best_y"]):
                d = "best cell (%d, %d), port (%d, %d)" % (g["best_x"], g["best_y"], it.fwd["best_x"], it.fwd["best_y"])
        if d is None and want["ret"] >= 0 and it.ops is not None and ops != it.ops:
            d = "dense ops %r, script %r" % (ops[-6:], it.ops[-6:])
        if d is None and (rec, ops) != w:
            d = "record or ops differ from the 64-lane walk's"
        if d:
            bad.append((it.tile.tag, d))
    return bad


def _compare(items, got, recs, wave):
    bad = differences(items, got, recs, wave)
    assert not bad, (len(bad), bad[:8])
    return sum(it.want["ret"] >= 0 for it in items)


@pytest.mark.parametrize("G", FORMS)
def test_every_family_in_every_form(built, batches, monkeypatch, G):
    monkeypatch.setenv(ENV, str(G))
    for name, (sc, items) in batches.items():
        tiles = [it.tile for it in items]
        wave = _wave_walk(name, tiles, sc)
        got, recs, n_chained = _run(tiles, sc)
        assert _compare(items, got, recs, wave) > 0, name
        assert n_chained == (2 if name == "ring" else 0), name


def _filler(n=4100):
    rng = np.random.default_rng(404)
    f = [synth.make_tile(rng, int(rng.integers(40, 120)), err=0.1, corridor="linear", ref_pad=60, tag="filler") for _ in range(64)]
    return (f * (n // 64 + 1))[:n]


def test_round_4_rule_bulk_at_8_lanes_and_long_class_at_32(built, batches, monkeypatch):
    """CVX_TUNE_BT_GROUP=-1 with the knobs test's 4 100 filler tiles behind the families: at least 4 096 tiles are walked, the bulk
    at 8 lanes per tile, and every tile with more than three times the batch's mean rows -- all the engineered ones -- in the
    32-lane long class on the side stream (walk_plan, cvx_host_logic.h)."""
    filler = _filler()
    for name, sc in (("default", wc.DEFAULT), ("mild", wc.MILD)):
        items = [it for k, (s, its) in batches.items() if s == sc and not k.startswith("share") for it in its]
        tiles = [it.tile for it in items] + filler
        mean_h = sum(t.H for t in tiles) / len(tiles)
        assert all(it.tile.H > 3 * mean_h for it in items)      # (a filler read is one row: every engineered tile is a long one)
        wave = _wave_walk("filler " + name, tiles, sc, len(items))
        monkeypatch.setenv(ENV, "-1")
        got, recs, _ = _run(tiles, sc, len(items))
        monkeypatch.delenv(ENV)
        assert _compare(items, got, recs, wave) > 0


@pytest.mark.parametrize("G", FORMS)
def test_lane_and_band_against_the_reference(built, cases, ref_oracle, monkeypatch, G):
    """the lane and band families against the reference's own ConvexAlignFast"""
    monkeypatch.setenv(ENV, str(G))
    for f in ("lane", "band"):
        tiles = [c.tile for c in cases if c.family == f]
        if ("ref", f) not in _WAVE:
            _WAVE[("ref", f)] = [ref_oracle.align(t) for t in tiles]
        got, _, _ = _run(tiles, wc.DEFAULT)
        bad = [(t.tag, same_alignment(w, g)) for t, w, g in zip(tiles, _WAVE[("ref", f)], got) if same_alignment(w, g) is not None]
        assert not bad, (len(bad), bad[:8])
        assert any(w["ret"] >= 0 for w in _WAVE[("ref", f)]) and (f != "band" or any(w["ret"] < 0 for w in _WAVE[("ref", f)]))
