"""tools/score_windows_rate.py [--calls K] [--genome-mbp M] [--out FILE] -- the scoring call's two data paths, side by side (GPU).

1 024-pair calls (256-base sub-reads, buffer_len 308, half of them on the reverse strand) over a synthetic genome, in one process,
the two forms alternating call by call after a warm-up:
  A  cvx_stage_windows_host + cvx_score_batch: the strings built on the host (the preparation loop of ScoreBuffer::DoRun) and sent
     as strings -- the data path of the string entry, the host preparation timed separately;
  B  cvx_score_windows: (position, buffer_len, read, strand) per pair, the strings written on the device.
Per form: host microseconds per call in front of the scoring entry, whole-call ms, kernel ms (cvx_stage_kernel_ms: all kernels of
the call, and stage_score_windows_kernel alone), bytes over PCIe per call worked out from the shapes -- on one lane and on 16
lanes (16 handles, one thread each, as StrippedSWHip deals ngmlr's workers over its handles)."""
import argparse
import ctypes as C
import json
import os
import sys
import threading
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ngmlr_amd import capi                                                    # noqa: E402
from ngmlr_amd.aligner import Genome, KmerIndex, StrippedSWHip, WINDOW_DTYPE, encode_genome    # noqa: E402

N_PAIRS, READ_LEN, BUFFER_LEN = 1024, 256, 308


def make_call(rng, contig, start, n_reads=128):
    """n_reads sub-reads cut from the genome (5 % substitutions), 8 candidates each, every other one on the reverse strand"""
    cpl = bytes.maketrans(b"ATCG", b"TAGC")
    reads, pairs = [], np.zeros(N_PAIRS, dtype=WINDOW_DTYPE)
    at = rng.integers(1000, len(contig) - 2000, size=n_reads)
    for r in range(n_reads):
        s = np.frombuffer(contig[int(at[r]):int(at[r]) + READ_LEN], dtype=np.uint8).copy()
        hit = rng.random(READ_LEN) < 0.05
        s[hit] = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=int(hit.sum()))
        fwd = s.tobytes()
        reads.append(fwd if r % 2 == 0 else fwd[::-1].translate(cpl))      # a read from the reverse strand is stored reversed
    for i in range(N_PAIRS):
        r = i % n_reads
        own = i < n_reads                                                    # the first candidate of a read is its true place
        loc = int(at[r]) if own else int(rng.integers(1000, len(contig) - 2000))
        pairs[i] = (start + loc - (52 >> 1), BUFFER_LEN, r, (r % 2) if own else int(rng.integers(0, 2)), 0)
    return reads, pairs


class Lane:
    def __init__(self, lib, genome_host, calls):
        self.sw = StrippedSWHip(device=0)
        self.lib, self.h = lib, self.sw._al.h
        self.binref, self.nib, self.starts = genome_host
        self.calls = []
        for reads, pairs in calls:
            arena, offsets, _ = KmerIndex.make_arena(reads)
            self.calls.append((arena, offsets, len(reads), pairs))
        self.out = np.zeros(N_PAIRS * (BUFFER_LEN + READ_LEN + 2) + 64, dtype=np.uint8)
        self.ro, self.qo = np.zeros(N_PAIRS, dtype=np.uint64), np.zeros(N_PAIRS, dtype=np.uint64)
        self.scores = np.zeros(N_PAIRS, dtype=np.float32)
        self.status = np.zeros(N_PAIRS, dtype=np.int32)
        self.rows = {"A": [], "B": []}
        self.used = 0

    def form_a(self, k):
        arena, offsets, n_reads, pairs = self.calls[k % len(self.calls)]
        used = C.c_uint64()
        t0 = time.perf_counter()
        capi.check(self.lib.cvx_stage_windows_host(self.binref.ctypes.data, self.nib, self.starts.ctypes.data, len(self.starts), n_reads, arena.ctypes.data,
                                                   offsets.ctypes.data, N_PAIRS, pairs.ctypes.data, self.out.ctypes.data, len(self.out),
                                                   self.ro.ctypes.data, self.qo.ctypes.data, None, C.byref(used)))
        refs = self.ro + np.uint64(self.out.ctypes.data)
        qrys = self.qo + np.uint64(self.out.ctypes.data)
        t1 = time.perf_counter()
        capi.check(self.lib.cvx_score_batch(self.h, N_PAIRS, refs.ctypes.data_as(C.POINTER(C.c_char_p)), qrys.ctypes.data_as(C.POINTER(C.c_char_p)),
                                            self.scores.ctypes.data))
        t2 = time.perf_counter()
        self.used = int(used.value)
        return (t1 - t0) * 1e6, (t2 - t0) * 1e3, self.sw.kernel_ms(), 0.0

    def form_b(self, k, genome):
        arena, offsets, n_reads, pairs = self.calls[k % len(self.calls)]
        t0 = time.perf_counter()
        capi.check(self.lib.cvx_score_windows(self.h, genome.g, n_reads, arena.ctypes.data, offsets.ctypes.data, N_PAIRS, pairs.ctypes.data,
                                              self.scores.ctypes.data, self.status.ctypes.data))
        t2 = time.perf_counter()
        return 0.0, (t2 - t0) * 1e3, self.sw.kernel_ms(), self.sw.stage_kernel_ms()

    def run(self, genome, n_calls, warmup, check):
        for k in range(-warmup, n_calls):
            a = self.form_a(k)
            sa = self.scores.copy()
            b = self.form_b(k, genome)
            if check:
                assert np.array_equal(sa.view(np.uint32), self.scores.view(np.uint32)) and not self.status.any(), "the two forms disagree"
            if k >= 0:
                self.rows["A"].append(a)
                self.rows["B"].append(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--genome-mbp", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = capi.load()
    rng = np.random.default_rng(12)
    contig = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=a.genome_mbp << 20).tobytes()
    binref, nib, starts = encode_genome(lib, [contig])
    calls = [make_call(rng, contig, int(starts[0])) for _ in range(8)]
    lines = ["score_windows_rate: %d-pair calls, %d-base sub-reads, buffer_len %d, genome %d Mbp, %d calls per lane and form after %d warm-up calls" % (
        N_PAIRS, READ_LEN, BUFFER_LEN, a.genome_mbp, a.calls, a.warmup)]
    result = {}
    for n_lanes in (1, 16):
        lanes = [Lane(lib, (binref, nib, starts), calls) for _ in range(n_lanes)]
        genome = Genome(lanes[0].sw._al, binref, nib, starts)
        t0 = time.perf_counter()
        ths = [threading.Thread(target=ln.run, args=(genome, a.calls, a.warmup, i == 0)) for i, ln in enumerate(lanes)]
        for t in ths:
            t.start()
        for t in ths:
            t.join()
        wall = time.perf_counter() - t0
        read_bytes = int(lanes[0].calls[0][1][-1])
        pcie = {"A": (lanes[0].used + 255) // 256 * 256 + N_PAIRS * 32 + N_PAIRS * 4, "B": (read_bytes + 255) // 256 * 256 + N_PAIRS * 56 + N_PAIRS * 4}
        for form in ("A", "B"):
            rows = np.array([r for ln in lanes for r in ln.rows[form]])
            med, lo, hi = np.median(rows, axis=0), np.percentile(rows, 10, axis=0), np.percentile(rows, 90, axis=0)
            result["%s_%d" % (form, n_lanes)] = dict(host_us=med[0], call_ms=med[1], kernel_ms=med[2], stage_kernel_ms=med[3], pcie_bytes=pcie[form])
            lines.append("%2d lane(s) form %s: host %7.1f us (10-90 %%: %.1f-%.1f), whole call %.3f ms (%.3f-%.3f), kernels %.3f ms (%.3f-%.3f), "
                         "of them the stage kernel %.4f ms, %d bytes over PCIe per call" % (
                             n_lanes, form, med[0], lo[0], hi[0], med[1], lo[1], hi[1], med[2], lo[2], hi[2], med[3], pcie[form]))
        lines.append("%2d lane(s): both forms of %d calls each in %.2f s wall" % (n_lanes, a.calls * n_lanes, wall))
        genome.free()
        for ln in lanes:
            ln.sw.close()
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
