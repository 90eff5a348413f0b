"""GPU (-m gpu): a handle in scalar-twin mode (CVX_CREATE_SCALAR_TWIN, ConvexAlignHip(scalar_twin=True)) behaves like the
reference's Convex::ConvexAlign -- what ngmlr --nosse selects -- not like Convex::ConvexAlignFast.

  - tiles without an 'x' in the window: against the port oracle in spec-fill mode (the scalar recurrence; pinned to the
    recorded twin by tests/test_twin_fixtures_cpu.py), every corridor kind, the default and five exotic scorings, the raw
    fill score and best cell of every tile;
  - tiles with 'x' in the window (tests/golden/twin_x.npz): against the recorded twin in every kernel form, and the same tiles
    on a default handle against the recorded ConvexAlignFast -- the switch, not the data, makes the difference;
  - no matrix-size cap in twin mode; the device text stage of a twin handle's job equals the host twin form.
Everything is compared bit-exactly with same_alignment on the key set without cigar_op_count / sv_type (tests/twin_cases.py)."""
import numpy as np
import pytest

from ngmlr_amd import capi, synth
from ngmlr_amd.aligner import ConvexAlignHip, format_alignment
from oracle.pyoracle import DEFAULT_PARAMS, Oracle, same_alignment
from tests import twin_cases, util
from tests.test_gpu_parity import EXOTIC_SCORING
from tests.twin_cases import TWIN_KEYS

pytestmark = pytest.mark.gpu

KINDS = {0: "whole", 1: "gang", 2: "chained", 3: "catch-all"}


def _check_against_port(al, orc, tiles):
    """same_alignment on the twin's keys + the raw fill result (score bits, best cell) of every tile, as tests/test_gpu_parity.py"""
    got = al.batch_align(tiles)
    bad, n_valid = [], 0
    for t, g in zip(tiles, got):
        want = orc.align(t)
        d = same_alignment(want, g, keys=TWIN_KEYS)
        if d is None:
            f, fs = orc.last_fwd(), orc.last_fill_score_bits()
            if fs != 0xBF800000 and g["status"] not in (4, 5):
                if fs != g["fwd_score_bits"]:
                    d = "raw fill score %08x vs %08x" % (g["fwd_score_bits"], fs)
                elif (f["best_x"], f["best_y"]) != (g["best_x"], g["best_y"]):
                    d = "argmax cell"
        assert g["status"] != -1, "tile %s fell outside every device kernel" % t.tag
        if g["ret"] >= 0:
            assert (g["cigar_op_count"], g["sv_type"]) == (capi.NOT_WRITTEN, capi.NOT_WRITTEN), t.tag
        n_valid += want["ret"] >= 0
        if d:
            bad.append((t.tag, t.H, t.W, d))
    assert not bad, bad[:5]
    return n_valid


def _xfree_zoo(seed):
    """every corridor kind, 40-600 read bases, no 'x' in the window"""
    tiles = [t for t in util.tile_zoo(seed=seed, n=72, max_w=620) if b"x" not in t.ref and 40 <= t.H <= 600]
    assert len(tiles) >= 40 and len({t.tag for t in tiles}) == 4
    return tiles


@pytest.mark.parametrize("k", range(len(EXOTIC_SCORING) + 1))
def test_x_free_tiles_equal_the_scalar_recurrence(built, k):
    """k = 0: the default scoring; else the exotic scorings of tests/test_gpu_parity.py, where ConvexAlignFast's SSE path gives
    other results -- a twin handle takes the rings there, never the SSE variant."""
    sc = twin_cases.scoring(DEFAULT_PARAMS) if k == 0 else EXOTIC_SCORING[k - 1]
    params = tuple(sc[n] for n in ("match", "mismatch", "gap_open", "gap_extend", "gap_extend_min", "gap_decay"))
    orc = Oracle("port", params)
    orc.set_spec_fill(True)
    al = ConvexAlignHip(device=0, scalar_twin=True, **sc)
    fixture = [t for _, p, t, _, _ in twin_cases.load("twin_xfree.npz") if p == DEFAULT_PARAMS]
    assert len(fixture) == 32
    tiles = _xfree_zoo(300 + k) + fixture[:12]
    assert _check_against_port(al, orc, tiles) > 30
    batch = al.upload(tiles)
    batch.run()
    kinds = {KINDS[l["kind"]] for l in batch.launches()}
    batch.free()
    al.close()
    assert "whole" in kinds and "gang" not in kinds      # rings, whatever the scoring: its sign structure holds in all six


def test_recorded_scorings_of_the_x_free_fixture(built):
    """the three recorded scorings outside the fast regime: the twin handle against the RECORDED twin"""
    by = {}
    for family, params, t, w, _ in twin_cases.load("twin_xfree.npz"):
        by.setdefault(params, []).append((t, w))
    assert len(by) == 4
    for params, items in by.items():
        al = ConvexAlignHip(device=0, scalar_twin=True, **twin_cases.scoring(params))
        got = al.batch_align([t for t, _ in items])
        al.close()
        bad = [(t.tag, same_alignment(w, g, keys=TWIN_KEYS)) for (t, w), g in zip(items, got)]
        assert not [b for b in bad if b[1]], [b for b in bad if b[1]][:5]


def test_no_matrix_size_cap_in_twin_mode(built, port_oracle):
    """One tile of 2.7 M cells with max_matrix_mb = 1: a default handle reports CVX_TILE_TOO_LARGE
    (src/AlignmentMatrixFast.cpp:45), a twin handle aligns it (AlignmentMatrix::prepare allocates whatever is asked)."""
    rng = np.random.default_rng(8)
    t = synth.make_tile(rng, 1500, err=0.1, corridor="full", tag="full-1500")
    assert t.cells >= 2_000_000
    al = ConvexAlignHip(device=0, max_matrix_mb=1)
    g = al.single_align(t)
    al.close()
    assert g["status"] == 4 and g["ret"] < 0
    port_oracle.set_spec_fill(True)
    try:
        al = ConvexAlignHip(device=0, max_matrix_mb=1, scalar_twin=True)
        assert _check_against_port(al, port_oracle, [t]) == 1
        al.close()
    finally:
        port_oracle.set_spec_fill(False)


FORMS = [{}, {"CVX_TUNE_MIN_M": "1"}, {"CVX_TUNE_MIN_M": "2"}, {"CVX_TUNE_MIN_M": "3"}, {"CVX_TUNE_MIN_M": "4"},
         {"CVX_TUNE_FORCE_WRAP16": "1"}, {"CVX_TUNE_PEN_TABLE": "0"}, {"CVX_TUNE_PEN_TABLE": "1"},
         {"CVX_TUNE_LATE_MIN": "1"},                                       # the exact refill of (nearly) every tile
         {"CVX_TUNE_MAX_M": "1", "CVX_TUNE_CHAIN_M": "2"},                 # corridors past 64 live rows as chained row blocks
         {"CVX_TUNE_MAX_M": "1", "CVX_TUNE_CHAIN_M": "1", "CVX_TUNE_FORCE_WRAP16": "1"},
         {"CVX_TUNE_MAX_M": "2", "CVX_TUNE_CHAIN_M": "4"},                 # 256-row blocks: fill_ring_twin_kernel<4, ., chain>
         {"CVX_TUNE_GANGS": "1"}]                                          # a twin handle ignores the gang knob (cvx_create_ex)


@pytest.mark.parametrize("env", FORMS, ids=lambda e: ",".join("%s=%s" % (k[9:], v) for k, v in e.items()) or "default")
def test_x_fixtures_equal_the_recorded_twin_in_every_kernel_form(built, monkeypatch, env):
    """Every family of tests/golden/twin_x.npz (x prefix / suffix runs of 1, 3, 4, 5, 63, 64, 65 columns, an all-x window, 5 %
    scatter, x against x, upper-case X, x in the corridor's first and last column, full matrices of 300 x 300 for the chained
    blocks, irregular corridors for the catch-all kernel) on a twin handle in the kernel form `env` selects."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    items = twin_cases.load("twin_x.npz")
    tiles = [t for _, _, t, _, _ in items]
    al = ConvexAlignHip(device=0, scalar_twin=True)
    batch = al.upload(tiles)
    tm = batch.run()
    launches = batch.launches()
    got = batch.alignments()
    batch.free()
    al.close()
    bad = []
    for (family, _, t, w, _), g in zip(items, got):
        assert g["status"] != -1, t.tag
        d = same_alignment(w, g, keys=TWIN_KEYS)
        if d:
            bad.append((family, t.tag, d))
    assert not bad, (len(bad), bad[:5])
    kinds = {KINDS[l["kind"]] for l in launches}
    assert "catch-all" in kinds and "gang" not in kinds, kinds          # the irregular family; no gang forms for the twin
    if not env:
        assert "chained" in kinds and "whole" in kinds, kinds           # the 300 x 300 family is chained by itself
        assert {l["slots_per_lane"] for l in launches if KINDS[l["kind"]] == "whole"} >= {1, 2}
    if "CVX_TUNE_MIN_M" in env:
        assert all(l["slots_per_lane"] >= int(env["CVX_TUNE_MIN_M"]) for l in launches if KINDS[l["kind"]] == "whole")
    if "CVX_TUNE_FORCE_WRAP16" in env:
        assert all(l["wrap16"] for l in launches)
    if "CVX_TUNE_LATE_MIN" in env:
        assert tm.n_tiles_redone >= 20, tm.n_tiles_redone
    if "CVX_TUNE_CHAIN_M" in env:
        assert tm.n_tiles_chained >= (20 if env["CVX_TUNE_MAX_M"] == "1" else 4), tm.n_tiles_chained
        assert {l["slots_per_lane"] for l in launches if KINDS[l["kind"]] == "chained"} == {int(env["CVX_TUNE_CHAIN_M"])}
    if "CVX_TUNE_GANGS" in env:
        # the knob bites on a default handle -- the 300 x 300 family becomes gangs of waves there -- and not on the twin's
        assert "chained" in kinds
        al = ConvexAlignHip(device=0)
        batch = al.upload(tiles)
        batch.run()
        default_kinds = {KINDS[l["kind"]] for l in batch.launches()}
        batch.free()
        al.close()
        assert "gang" in default_kinds, default_kinds


def test_the_same_x_fixtures_on_a_default_handle_equal_convex_align_fast(hip_aligner):
    """... and differ from the twin's where the recording says so: the switch, not the data, makes the difference."""
    items = twin_cases.load("twin_x.npz")
    got = hip_aligner.batch_align([t for _, _, t, _, _ in items])
    bad, n_other = [], 0
    for (family, _, t, w, f), g in zip(items, got):
        d = same_alignment(f, g)
        if d:
            bad.append((family, t.tag, d))
        if twin_cases.differs(w, f):
            n_other += same_alignment(w, g, keys=TWIN_KEYS) is not None
    assert not bad, (len(bad), bad[:5])
    assert n_other >= len(items) // 5


def test_device_text_of_a_twin_job_equals_the_host_twin_form(built):
    tiles = [t for name in ("twin_x.npz", "twin_xfree.npz") for _, p, t, _, _ in twin_cases.load(name) if p == DEFAULT_PARAMS]
    al = ConvexAlignHip(device=0, scalar_twin=True)
    job = al.submit(tiles)
    res, ops = job.wait()
    dev = job.text_all()[0]
    n_valid = 0
    for i, t in enumerate(tiles):
        r = capi.CvxResult.from_buffer_copy(res[i].tobytes())
        host = format_alignment(al.lib, r, ops, t, scalar_twin=True)
        d = dev[i]
        for k in ("ret", "score_bits", "position_offset", "qstart", "qend", "nm", "alignment_length", "cigar_op_count", "sv_type",
                  "first_ref", "first_read", "last_ref", "last_read", "nm_count", "cigar_len", "md_len", "cigar", "md"):
            assert host[k] == d[k], (t.tag, k, str(host[k])[:60], str(d[k])[:60])
        assert (d["cigar_op_count"], d["sv_type"]) == (capi.NOT_WRITTEN, capi.NOT_WRITTEN)
        n_valid += host["ret"] >= 0
    job.release()
    al.close()
    assert n_valid >= 90
