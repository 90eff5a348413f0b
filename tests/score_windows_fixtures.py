"""The fixtures of scoring against the resident genome (tests/golden/score_windows_*.npz, recorded from the unmodified reference by
tools/make_golden_score_windows.sh) in the form the tests use.  A plain module (no pytest fixtures, no device): loaded once per
process and shared by tests/test_score_windows_cpu.py and tests/test_gpu_score_windows.py."""
import functools
import os
from types import SimpleNamespace

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = ("test_3", "test_2", "cases")
CASE_FAILURES = 3      # the last cases of score_windows_cases.npz: position L, L + 5 and the wrapped (uint64) (5 - 20)


def case_sequences():
    """the sequences of the small synthetic genome the engineered windows were recorded on (committed as data)"""
    seqs = []
    for line in open(os.path.join(GOLDEN, "score_windows_cases.fa"), "rb").read().split(b"\n"):
        if line and not line.startswith(b">"):
            seqs.append(line)
    return seqs


@functools.lru_cache(maxsize=None)
def load(name):
    """-> namespace: binref, nibbles, starts (the genome); concat_len; reads (list of bytes); pairs (list of (position, buffer_len,
    read, reverse)); win, qry (the recorded strings); ret, score, reverse, kind (arrays)"""
    from ngmlr_amd import capi
    from ngmlr_amd.aligner import encode_genome
    z = np.load(os.path.join(GOLDEN, "score_windows_%s.npz" % name))
    if name == "cases":
        binref, nibbles, starts = encode_genome(capi.load(), case_sequences())
    else:
        g = np.load(os.path.join(GOLDEN, "decode_%s.npz" % name))
        binref, nibbles, starts = g["binref"], int(g["nibbles"]), g["starts"]
    assert nibbles == int(z["n_nibbles"])
    n = len(z["read"])

    def strings(key):
        blob, off = z[key].tobytes(), z[key + "_off"]
        return [blob[int(off[i]):int(off[i + 1])] for i in range(len(off) - 1)]
    reads = [z["reads"][int(z["read_off"][i]):int(z["read_off"][i + 1])].tobytes() for i in range(len(z["read_off"]) - 1)]
    pairs = list(zip(z["position"].tolist(), z["buffer_len"].tolist(), z["read"].tolist(), z["reverse"].tolist()))
    assert len(pairs) == n
    return SimpleNamespace(name=name, binref=binref, nibbles=nibbles, starts=starts, concat_len=int(z["concat_len"]), reads=reads, pairs=pairs,
                           win=strings("win"), qry=strings("qry"), ret=z["ret"], score=z["score"], reverse=z["reverse"], kind=z["kind"],
                           buffer_len=z["buffer_len"], position=z["position"])
