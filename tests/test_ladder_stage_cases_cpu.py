"""CPU: the engineered tiles of tests/ladder_stage_cases.py hold what tests/test_gpu_ladder_stages.py relies on -- from the port
oracle (its host text stage gives the profile) and cvx_nm_regions_host alone, no device.  Without this the GPU tests could pass
on tiles that never climb, never have a region or never fail."""
import pytest

from tests import ladder_cases as lc
from tests import ladder_stage_cases as sc


def _with_regions(port_oracle, cases):
    from ngmlr_amd import aligner, capi
    lib = capi.load()
    exp = sc.expectation(cases, lambda t: port_oracle.align(t, want_nm=False)["ret"] >= 0, port_oracle.align)
    for e in exp:
        e["regions"] = []
        if e["port"] is not None and e["port"]["ret"] >= 0:
            reg, _ = aligner.nm_regions_host(e["port"]["nm_per_position"], e["port"]["alignment_length"], lib)
            e["regions"] = [tuple(int(v) for v in r) for r in reg]
    return exp


@pytest.fixture(scope="module")
def expectation(port_oracle):
    return _with_regions(port_oracle, sc.engineered())


def test_tiles_that_climb_carry_regions(expectation):
    assert sum(1 for e in expectation if e["rung"] >= 2 and len(e["regions"]) >= 1) >= 8
    assert sum(1 for e in expectation if e["rung"] >= 3 and e["live"] and e["port"]["ret"] >= 0) >= 2
    assert any(e["rung"] >= 3 and len(e["regions"]) >= 1 for e in expectation)
    # every rung from 1 to 4 reports a tile with regions: the merge takes regions from each of them
    assert {e["rung"] for e in expectation if e["regions"]} >= {1, 2, 3, 4}


def test_a_tile_fails_on_its_last_rung_and_has_no_region(expectation):
    failed = [e for e in expectation if e["live"] and e["port"]["ret"] < 0]
    assert failed and all(not e["regions"] for e in failed)
    assert any(e["rung"] == lc.ladder_length(len(e["ref"]), e["ladder"]) and e["rung"] > 1 for e in failed)


def test_every_builder_is_there(expectation):
    assert any(not e["live"] and len(e["qry"]) == 0 for e in expectation)                       # EMPTY
    assert any(e["ladder"][3] & lc.FULL and e["live"] for e in expectation)
    assert any(e["ladder"][3] & lc.SHORT and e["live"] for e in expectation)
    assert any(e["ladder"][3] == lc.ANCHORS and e["rung"] >= 3 and e["port"]["ret"] >= 0 and e["tiles"][1].desc[3] != 0.0 and e["tiles"][2].desc[3] == 0.0
               for e in expectation)                                                            # anchors form, then the endpoints form at rung 3
    assert any(e["ladder"][3] == lc.ANCHORS and e["rung"] >= 3 and e["regions"] for e in expectation)


def test_a_planted_inversion_lies_on_a_tile_that_climbed(expectation):
    hit = 0
    for e in expectation:
        if e["planted"] is None or e["rung"] < 2:
            continue
        first, last = e["planted"]
        hit += any(r[2] <= last and r[3] >= first and min(r[3], last) - max(r[2], first) >= 100 for r in e["regions"])      # (read coordinates)
    assert hit >= 1
    assert any(e["planted"] is not None and e["rung"] == 1 and e["regions"] for e in expectation)      # ... and one on a tile that did not


def test_read_lengths(expectation):
    assert max(len(e["qry"]) for e in expectation) <= 3000 and sum(1 for e in expectation if len(e["qry"]) >= 600) >= 50


def test_the_grow_tiles_outgrow_their_rungs_arena(port_oracle):
    """all of them climb to the same rung, whose arena holds 9 n + 136 regions (8 n + 64 asked for, cvx_buf.h's growth rule)"""
    exp = _with_regions(port_oracle, sc.grow_tiles())
    n = len(exp)
    assert n == 6 and [e["rung"] for e in exp] == [2] * n
    assert sum(len(e["regions"]) for e in exp) > 9 * n + 136 + 40
    assert all(600 <= len(e["qry"]) <= 3000 for e in exp)


def test_the_straddle_job_climbs_on_both_sides_of_entry_256(port_oracle):
    exp = _with_regions(port_oracle, sc.straddle())
    assert 280 <= len(exp) <= 300
    climbing = [i for i, e in enumerate(exp) if e["rung"] >= 2]
    assert sum(1 for i in climbing if i < 256) >= 20 and sum(1 for i in climbing if i >= 256) >= 5
    assert all(exp[i]["regions"] for i in climbing)
    assert any(exp[i]["rung"] >= 3 for i in climbing if i >= 256)
