"""tools/search_score_rate.py [--genome-mbp 2,512] [--reads 806] [--calls K] [--out FILE] -- a CS batch's two device calls against
the one that replaces them (GPU).

One call of `--reads` 256-base sub-reads (806: what a CS thread's batch of ten 20 kb reads splits into) over a synthetic genome of
2 Mbp (the pipeline's test size) and of 512 Mbp (a table that leaves every cache), on ONE handle in one process, the two forms
alternating call by call after a warm-up:
  A  cvx_search_batch_arena, then the pairs built on the host from the lists, then cvx_score_windows: two device calls, the
     reads uploaded twice, 56 bytes per pair up;
  B  cvx_search_score_arena: one call.
Per form: wall per batch (host clock around calls that end in a wait), the host time between A's two calls, kernel ms by stage
(cvx_stage_kernel_ms: search; stage + score of A; plan + stage + score of B), bytes over PCIe each way worked out from the shapes.
The scores of the two forms are compared bit for bit on every call."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ngmlr_amd import capi, synth                                             # noqa: E402
from ngmlr_amd.aligner import CANDIDATE_DTYPE, ConvexAlignHip, Genome, KmerIndex, WINDOW_DTYPE, encode_genome    # noqa: E402

K, SKIP, BIN_SHIFT, BUFFER_LEN, LEAD, MAX_CMRS = 13, 2, 4, 308, 20, 1000


def build(lib, mbp):
    contigs = synth.big_reference(mbp << 20, n_contigs=8 if mbp >= 64 else 2, families=24 if mbp >= 64 else 2, microsats=600 if mbp >= 64 else 10)
    binref, nib, starts = encode_genome(lib, [c.tobytes() for c in contigs])
    lens = np.array([len(c) for c in contigs], dtype=np.uint64)
    idx = np.zeros(((1 << (2 * K)) + 2) * 5, dtype=np.uint8)
    locs = np.zeros(int(lens.sum()) // (SKIP + 1) + 64, dtype=np.uint32)
    nl = C.c_uint64()
    capi.check(lib.cvx_index_build_device(0, binref.ctypes.data, nib, starts.ctypes.data, lens.ctypes.data, len(lens), K, SKIP, BIN_SHIFT,
                                          idx.ctypes.data, locs.ctypes.data, len(locs), C.byref(nl), 0))
    return contigs, binref, nib, starts, idx.view(np.dtype([("tab", "<u4"), ("rc", "i1")])), locs[:nl.value]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome-mbp", default="2,512")
    ap.add_argument("--reads", type=int, default=806)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = capi.load()
    lines, result = [], {}
    for mbp in [int(x) for x in a.genome_mbp.split(",")]:
        contigs, binref, nib, starts, idx, locs = build(lib, mbp)
        al = ConvexAlignHip(device=0)
        genome = Genome(al, binref, nib, starts)
        ix = KmerIndex(al, K, idx, locs, 0)
        batches = []
        for b in range(8):
            arena, offsets, _ = KmerIndex.make_arena(synth.sample_subreads(contigs, a.reads, seed=100 + b))
            batches.append((arena, offsets))
        del contigs
        n = a.reads
        cap = 1 << 18
        ncand, begin = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.uint64)
        cands = np.zeros(cap, dtype=CANDIDATE_DTYPE)
        mh, ms = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.int32)
        sw_a, st_a = np.zeros(cap, dtype=np.float32), np.zeros(cap, dtype=np.int32)
        sw_b, st_b = np.zeros(cap, dtype=np.float32), np.zeros(cap, dtype=np.int32)
        used = C.c_uint64()
        rows = {"A": [], "B": []}
        pcie = {}

        def form_a(arena, offsets):
            t0 = time.perf_counter()
            capi.check(lib.cvx_search_batch_arena(al.h, ix.ix, n, arena.ctypes.data, offsets.ctypes.data, 0.8, 0.0, BIN_SHIFT, 0, ncand.ctypes.data, begin.ctypes.data,
                                                  cands.ctypes.data, cap, C.byref(used), mh.ctypes.data, ms.ctypes.data))
            t1 = time.perf_counter()
            search_ms = al.stage_kernel_ms(capi.STAGE_SEARCH)
            u = int(used.value)
            # the host's part between the calls: one pair per candidate of every list below max_cmrs (vectorised: the C++ binding's loop is cheaper still)
            owner = np.repeat(np.arange(n), np.maximum(ncand, 0))
            keep = ncand[owner] < MAX_CMRS
            tab = np.zeros(int(keep.sum()), dtype=WINDOW_DTYPE)
            tab["position"] = cands["location"][:u][keep] - np.uint64(LEAD)
            tab["buffer_len"], tab["read"], tab["reverse"] = BUFFER_LEN, owner[keep], cands["reverse"][:u][keep]
            t2 = time.perf_counter()
            sw_a[:u] = -1.0
            sc, st = np.zeros(len(tab), dtype=np.float32), np.zeros(len(tab), dtype=np.int32)
            capi.check(lib.cvx_score_windows(al.h, genome.g, n, arena.ctypes.data, offsets.ctypes.data, len(tab), tab.ctypes.data, sc.ctypes.data, st.ctypes.data))
            t3 = time.perf_counter()
            sw_a[:u][keep] = sc
            read_bytes = int(offsets[-1] - offsets[0])
            pcie["A"] = (2 * read_bytes + n * 12 + len(tab) * 56, u * 16 + n * 12 + len(tab) * 4)
            return u, ((t3 - t0) * 1e3, (t2 - t1) * 1e3, search_ms, al.stage_kernel_ms(capi.STAGE_SCORE))

        def form_b(arena, offsets):
            t0 = time.perf_counter()
            capi.check(lib.cvx_search_score_arena(al.h, ix.ix, genome.g, n, arena.ctypes.data, offsets.ctypes.data, 0.8, 0.0, BIN_SHIFT, 0, BUFFER_LEN, LEAD, MAX_CMRS,
                                                  ncand.ctypes.data, begin.ctypes.data, cands.ctypes.data, cap, C.byref(used), mh.ctypes.data, ms.ctypes.data,
                                                  sw_b.ctypes.data, st_b.ctypes.data))
            t1 = time.perf_counter()
            u = int(used.value)
            read_bytes = int(offsets[-1] - offsets[0])
            pcie["B"] = (read_bytes + n * 12 + (n + 1) * 8, u * 16 + n * 12 + u * 8)
            return u, ((t1 - t0) * 1e3, 0.0, al.stage_kernel_ms(capi.STAGE_SEARCH), al.stage_kernel_ms(capi.STAGE_SEARCH_SCORE))

        n_cands = 0
        for k in range(-a.warmup, a.calls):
            arena, offsets = batches[k % len(batches)]
            order = (form_a, form_b) if k % 2 == 0 else (form_b, form_a)      # which form goes first alternates too
            got = {}
            for f in order:
                got[f.__name__] = f(arena, offsets)
            ua, ra = got["form_a"]
            ub, rb = got["form_b"]
            assert ua == ub and np.array_equal(sw_a[:ua].view(np.uint32), sw_b[:ub].view(np.uint32)), "the two forms disagree"
            n_cands = ua
            if k >= 0:
                rows["A"].append(ra)
                rows["B"].append(rb)
        lines.append("search_score_rate: %d sub-reads of 256 bases per call (%d candidates in the last), genome %d Mbp (%d locations in the table), buffer_len %d, "
                     "%d calls per form after %d warm-up calls, one handle" % (n, n_cands, mbp, len(locs), BUFFER_LEN, a.calls, a.warmup))
        for form in ("A", "B"):
            r = np.array(rows[form])
            med, lo, hi = np.median(r, axis=0), np.percentile(r, 10, axis=0), np.percentile(r, 90, axis=0)
            result["%s_%d" % (form, mbp)] = dict(call_ms=med[0], host_between_ms=med[1], search_kernel_ms=med[2], score_kernel_ms=med[3], pcie_up=pcie[form][0], pcie_down=pcie[form][1])
            lines.append("  %4d Mbp form %s: wall %.3f ms per batch (10-90 %%: %.3f-%.3f), host between the calls %.3f ms, search kernels %.3f ms (%.3f-%.3f), "
                         "%s kernels %.3f ms (%.3f-%.3f), PCIe %d B up / %d B down" % (
                             mbp, form, med[0], lo[0], hi[0], med[1], med[2], lo[2], hi[2], "stage + score" if form == "A" else "plan + stage + score",
                             med[3], lo[3], hi[3], pcie[form][0], pcie[form][1]))
        ix.free()
        genome.free()
        al.close()
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
