"""GPU (-m gpu), in the manner of tests/test_gpu_lifecycle.py: rounds of create, cvx_submit_ladder_ex jobs with a genome on a
handle with all three stage flags -- one job released, one left to cvx_destroy, so the later rungs' batches, their stage arenas
and the merged buffers leave both ways -- then destroy.  Every round computes what the first did, and the device's free memory
after the last round is where the first round left it: a round that kept a handle's memory would show as that handle's size,
measured in the same run (free memory after cvx_destroy minus before it)."""
import ctypes as C

import pytest

from tests import ladder_stage_cases as sc

pytestmark = pytest.mark.gpu

ROUNDS = 3
TAGS = ("bursts-d0", "bursts-d90", "bursts-d150", "inv200-d100", "ep64-d300")      # rungs 1, 2, 3, 2, and one no rung resolves


def _free_bytes():
    hip = C.CDLL("libamdhip64.so")
    free, total = C.c_size_t(), C.c_size_t()
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return int(free.value)


@pytest.fixture(scope="module")
def fixture(built, port_oracle):
    from types import SimpleNamespace
    from ngmlr_amd import capi
    from tests.test_gpu_ladder_stages import _genome_of
    lib = capi.load()
    by_tag = {c[0]: c for c in sc.engineered()}
    cases = sc.expectation([by_tag[t] for t in TAGS], lambda t: port_oracle.align(t, want_nm=False)["ret"] >= 0)
    assert [e["rung"] for e in cases] == [1, 2, 3, 2, 5]
    genome, positions = _genome_of(lib, cases)
    return SimpleNamespace(lib=lib, cases=cases, genome=genome, positions=positions)


def _round(fx):
    from ngmlr_amd.aligner import ConvexAlignHip, Genome
    from tests.test_gpu_ladder_stages import _ladder_answer, _ladder_tiles
    al = ConvexAlignHip(device=0, nm_regions=True, inv_checks=True, job_text=True)
    out = {}
    try:
        g = Genome(al, *fx.genome)
        jobs = [al.submit_ladder_ex(_ladder_tiles(fx.cases), [e["ladder"] for e in fx.cases], genome=g, ref_positions=fx.positions) for _ in range(2)]
        for name, job in zip(("released", "kept"), jobs):
            a = _ladder_answer(job, al)
            out[name] = (a["res_bytes"], a["ops"], a["lad"].tobytes(), a["info"], a["off"].tobytes(), a["reg"].tobytes(), a["open"], a["checks"].tobytes(),
                         a["trecs"], a["toff"].tobytes(), a["traw"])
        jobs[0].release()      # jobs[1] stays: cvx_destroy finds it, and its later rungs' batches, on the handle's live list
        g.free()
        held = _free_bytes()
    finally:
        al.close()
    return out, _free_bytes(), held


def test_rounds_of_ladder_jobs_with_stages_give_their_memory_back(fixture):
    rounds = [_round(fixture) for _ in range(ROUNDS)]
    first = rounds[0][0]
    assert first["released"] == first["kept"]
    for k in range(1, ROUNDS):
        assert rounds[k][0] == first, k
    a = first["kept"]
    assert a[3]["rungs_run"] == 5 and a[3]["tiles"] == [5, 4, 2, 1, 1] and len(a[5]) // 16 >= 30
    # the handle's device memory, as this run measured it, and what is missing after the last round
    handle_bytes = min(after - held for _, after, held in rounds)
    assert handle_bytes > 0
    assert rounds[0][1] - rounds[-1][1] < handle_bytes, (rounds[0][1], rounds[-1][1], handle_bytes)
