"""CPU: cvx_stage_segments_host against what the UNMODIFIED reference's extractReadSeq returned (reference
src/AlignmentBuffer.cpp:1515-1542), recorded by tools/make_golden_read_segments.sh on test_3, on the split-read workload of
tests/test_gpu_e2e.py (inversions: revComp = true occurs) and on an engineered read set with N, lower case and other printable
bytes (tests/golden/read_segments_*.npz): every recorded call by a 64-bit hash of its output, a seeded sample of each
(isReverse, revComp) combination byte for byte.  The mapping under test: flags = (isReverse != revComp) -- the double complement
under revComp is the forward copy -- confirmed here on the reference's own output, not taken on faith."""
import os

import pytest

from tests.segment_cases import hash64, load, segments_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = ("read_segments_test_3.npz", "read_segments_split.npz", "read_segments_cases.npz")


@pytest.mark.parametrize("name", FIXTURES)
def test_host_restatement_reproduces_every_recorded_call(built, name):
    from ngmlr_amd import capi
    from ngmlr_amd.aligner import stage_segments_host
    z, reads = load(name)
    calls = z["calls"]
    assert len(calls) > 100 and len(reads) >= 1
    segs, lens = segments_of(calls)
    got = stage_segments_host(capi.load(), reads, segs, lens)
    bad = [i for i, g in enumerate(got) if hash64(g) != int(z["hashes"][i])]
    assert not bad, (len(bad), [tuple(calls[i]) for i in bad[:5]])
    so = z["sample_offsets"].astype("int64")
    assert len(z["sample"]) > 0
    for k, i in enumerate(z["sample"]):
        assert got[int(i)] == z["sample_out"][so[k]:so[k + 1]].tobytes(), tuple(calls[int(i)])


def test_every_combination_was_recorded():
    """each of the four (isReverse, revComp) combinations is present, and in the sample: in the engineered set and in test_3, where
    the pipeline's own realign produced them (2 and 6 calls with revComp).  The split-read workload's 307 calls hold both
    strands but no revComp call: its inversions never reached the inverted-rc tile of realign (:1653)."""
    z, _ = load("read_segments_split.npz")
    assert set(int(x) for x in z["calls"][:, 3]) == {0, 1}
    for name in ("read_segments_cases.npz", "read_segments_test_3.npz"):
        z, _ = load(name)
        calls = z["calls"]
        for rev in (0, 1):
            for rc in (0, 1):
                assert int(((calls[:, 3] == rev) & (calls[:, 4] == rc)).sum()) > 0, (name, rev, rc)
                assert any(calls[int(i)][3] == rev and calls[int(i)][4] == rc for i in z["sample"]), (name, rev, rc)
    z, reads = load("read_segments_cases.npz")
    blob = b"".join(reads)
    assert b"N" in blob and b"a" in blob and b"*" in blob
    for name in FIXTURES:
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", name)) < (1 << 20)
