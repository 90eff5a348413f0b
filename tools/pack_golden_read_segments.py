#!/usr/bin/env python
"""Packs what tools/make_golden_read_segments.sh recorded at the end of the reference's five-argument extractReadSeq into
tests/golden/read_segments_*.npz, and writes the engineered inputs the recorder answers.

  --cases-in READS.txt OUT.reads OUT.cases   the committed engineered reads (one per line) as the hook reads them (int32 length +
                                             bytes each) and a seeded list of `read start len isReverse revComp`
  --pack DUMP OUT.npz                        each distinct read once (`reads`, `read_offsets`), every call's arguments
                                             (`calls`: read, start, len, isReverse, revComp) plus a 64-bit hash of its output
                                             (`hashes`: blake2b-8), and the full output of a seeded sample of each of the four
                                             (isReverse, revComp) combinations (`sample`, `sample_out`, `sample_offsets`).  A dump
                                             whose reads do not fit 1 MB keeps a seeded subset of its reads -- those with revComp
                                             calls first -- and all of their calls.  Prints the count per combination.
"""
import hashlib
import struct
import sys

import numpy as np

BUDGET = 900_000      # bytes of the .npz (a committed file stays under 1 MiB)
SAMPLE = 24           # full outputs per combination


def hash64(b: bytes) -> int:
    return int.from_bytes(hashlib.blake2b(b, digest_size=8).digest(), "little")


def cases_in(reads_txt, out_reads, out_cases):
    reads = [l.rstrip(b"\n") for l in open(reads_txt, "rb") if l.strip()]
    with open(out_reads, "wb") as f:
        for r in reads:
            f.write(struct.pack("<i", len(r)) + r)
    rng = np.random.default_rng(15)
    with open(out_cases, "w") as f:
        for ri, r in enumerate(reads):
            L = len(r)
            lens = sorted(set([1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, L] + [int(x) for x in rng.integers(1, L + 1, size=6)]))
            for ln in lens:
                if ln > L:
                    continue
                for start in sorted(set([0, L - ln] + [int(x) for x in rng.integers(0, L - ln + 1, size=2)])):
                    for rev in (0, 1):
                        for rc in (0, 1):
                            f.write("%d %d %d %d %d\n" % (ri, start, ln, rev, rc))


def parse(dump):
    b = open(dump, "rb").read()
    at, recs = 0, []
    while at < len(b):
        (ln,) = struct.unpack_from("<i", b, at); at += 4
        seq = b[at:at + ln]; at += ln
        start, slen, rev, rc, ol = struct.unpack_from("<5i", b, at); at += 20
        out = b[at:at + ol]; at += ol
        recs.append((seq, start, slen, rev, rc, out))
    return recs


def pack(dump, out_npz):
    recs = parse(dump)
    index, reads = {}, []
    for seq, *_ in recs:
        if seq not in index:
            index[seq] = len(reads)
            reads.append(seq)
    rng = np.random.default_rng(29)
    has_rc = set(index[r[0]] for r in recs if r[4])
    order = sorted(range(len(reads)), key=lambda i: (i not in has_rc, rng.random()))
    keep = len(reads)
    while True:
        chosen = sorted(order[:keep])
        remap = {old: new for new, old in enumerate(chosen)}
        calls = [(remap[index[s]], st, ln, rev, rc, out) for s, st, ln, rev, rc, out in recs if index[s] in remap]
        arena = b"".join(reads[i] for i in chosen)
        offsets = np.concatenate([[0], np.cumsum([len(reads[i]) for i in chosen])]).astype(np.uint64)
        tab = np.array([c[:5] for c in calls], dtype=np.int32).reshape(-1, 5)
        hashes = np.array([hash64(c[5]) for c in calls], dtype=np.uint64)
        sample = []
        for rev in (0, 1):
            for rc in (0, 1):
                idx = [i for i, c in enumerate(calls) if c[3] == rev and c[4] == rc]
                sample += sorted(int(x) for x in rng.choice(idx, size=min(SAMPLE, len(idx)), replace=False)) if idx else []
        sout = b"".join(calls[i][5] for i in sample)
        soff = np.concatenate([[0], np.cumsum([len(calls[i][5]) for i in sample])]).astype(np.uint64)
        np.savez_compressed(out_npz, reads=np.frombuffer(arena, dtype=np.uint8), read_offsets=offsets, calls=tab, hashes=hashes,
                            sample=np.array(sample, dtype=np.int32), sample_out=np.frombuffer(sout, dtype=np.uint8), sample_offsets=soff)
        import os
        size = os.path.getsize(out_npz)
        if size <= BUDGET or keep <= 1:
            break
        keep = max(1, int(keep * min(0.9, BUDGET / size)))
    counts = {(rev, rc): int(((tab[:, 3] == rev) & (tab[:, 4] == rc)).sum()) for rev in (0, 1) for rc in (0, 1)}
    print("%s: %d of %d reads, %d of %d calls, %d bytes; (isReverse, revComp) counts: %s" % (out_npz, len(chosen), len(reads), len(calls), len(recs), size, counts))


if __name__ == "__main__":
    if sys.argv[1] == "--cases-in":
        cases_in(*sys.argv[2:5])
    elif sys.argv[1] == "--pack":
        pack(*sys.argv[2:4])
    else:
        sys.exit(__doc__)
