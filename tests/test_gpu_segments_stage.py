"""GPU: stage_segments_kernel alone (cvx_stage_segments) against the host restatement (cvx_stage_segments_host) and the rule
written out in Python: an engineered sweep of a few thousand strings in one call and one per call, one 130 000-byte segment that
spans many chunks, and an empty call."""
import numpy as np
import pytest

from tests.segment_cases import engineered_sweep, want_string

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sweep(built):
    from ngmlr_amd import capi
    from ngmlr_amd.aligner import stage_segments_host
    reads, segs, lens = engineered_sweep()
    host = stage_segments_host(capi.load(), reads, segs, lens)
    assert host == [want_string(reads[r], s, n, f) for (r, s, f), n in zip(segs, lens)]
    return reads, segs, lens, host


def test_sweep_in_one_call(hip_aligner, sweep):
    reads, segs, lens, host = sweep
    assert len(segs) > 3000
    got = hip_aligner.stage_segments(reads, segs, lens)
    bad = [(segs[i], lens[i]) for i in range(len(segs)) if got[i] != host[i]]
    assert not bad, (len(bad), bad[:8])


def test_sweep_one_string_per_call(hip_aligner, sweep):
    """every string alone at destination phase 0 (a sample: the calls are what takes the time)"""
    from ngmlr_amd.aligner import KmerIndex
    reads, segs, lens, host = sweep
    block = KmerIndex.make_arena(reads)[:2]
    bad = []
    for i in range(0, len(segs), 23):
        if hip_aligner.stage_segments(block, [segs[i]], [lens[i]]) != [host[i]]:
            bad.append((segs[i], lens[i]))
    assert not bad, (len(bad), bad[:8])


def test_one_long_segment(hip_aligner):
    from ngmlr_amd import capi
    rng = np.random.default_rng(11)
    read = bytes(rng.choice(np.frombuffer(b"ACGTACGTNacgt", dtype=np.uint8), size=130000 + 77))
    segs, lens = [(0, 77, 1), (0, 0, 0), (0, 40, 1), (0, 41, 0)], [130000, 130000, 130000, 130001]
    got = hip_aligner.stage_segments([read], segs, lens)
    assert got == [want_string(read, s, n, f) for (_, s, f), n in zip(segs, lens)]
    assert hip_aligner.stage_kernel_ms(capi.STAGE_SEGMENTS) > 0.0


def test_empty_call_and_errors(hip_aligner):
    from ngmlr_amd import capi
    assert hip_aligner.stage_segments([b"ACGT"], [], []) == []
    assert hip_aligner.stage_segments([b"ACGT"], [(0, 4, 1), (0, 0, 0)], [0, 0]) == [b"", b""]
    for seg, length in (((1, 0, 0), 1), ((0, -1, 0), 1), ((0, 2, 0), 3), ((0, 0, 4), 1)):
        with pytest.raises(capi.CvxError) as e:
            hip_aligner.stage_segments([b"ACGT"], [seg], [length])
        assert e.value.code == -3
    assert hip_aligner.stage_segments([b"ACGT"], [(0, 1, 1)], [3]) == [b"ACG"]      # the handle is still usable


@pytest.mark.parametrize("name", ["read_segments_cases.npz", "read_segments_test_3.npz"])
def test_device_reproduces_the_recorded_reference_calls(hip_aligner, name):
    """every call of the unmodified reference's extractReadSeq in the fixture (tools/make_golden_read_segments.sh), in one device
    call: by the 64-bit hash of its output, flags = (isReverse != revComp)"""
    from tests.segment_cases import hash64, load, segments_of
    z, reads = load(name)
    segs, lens = segments_of(z["calls"])
    got = hip_aligner.stage_segments(reads, segs, lens)
    bad = [i for i, g in enumerate(got) if hash64(g) != int(z["hashes"][i])]
    assert not bad, (len(bad), [tuple(z["calls"][i]) for i in bad[:5]])
