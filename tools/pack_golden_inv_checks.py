"""tools/pack_golden_inv_checks.py DUMP OUT.npz [--synth-genome SEED LENGTH FASTA] -- the call records the recorder hook of
tools/make_golden_inv_checks.sh wrote at the ends of the reference's checkForSV, as arrays (tests/golden/inv_checks_*.npz), and
the counts per outcome.  Identical calls are stored once.  --synth-genome: the workload's reference is
synth.random_ref(default_rng(SEED), LENGTH) (tools/e2e_rates.py write_sv_workload); its seed, length and the SHA-1 of its bases
are stored in place of a FASTA, after checking them against the one the run used."""
import hashlib
import sys

import numpy as np

REC = np.dtype([("on_ref_start", "<i8"), ("mid_ref", "<u8"), ("mid_read", "<u8"), ("position_offset", "<i4"), ("inv_len", "<i4"),
                ("read_len", "<i4"), ("outcome", "<i4"), ("ref_chars", "<i4"), ("n_read", "<i4"), ("read", "S128"),
                ("score_fwd", "<f4"), ("score_rev", "<f4")])
OUTCOMES = {0: "scoring block ran", 1: "inversion too short", 2: "no read part"}


def main():
    dump, out = sys.argv[1], sys.argv[2]
    assert REC.itemsize == 184
    raw = np.fromfile(dump, dtype=REC)
    recs = np.unique(raw) if len(raw) else raw
    assert all(int(r["n_read"]) in (0, 100) for r in recs), "a read part is 100 characters or none"
    extra = {}
    if "--synth-genome" in sys.argv:
        k = sys.argv.index("--synth-genome")
        seed, length, fasta = int(sys.argv[k + 1]), int(sys.argv[k + 2]), sys.argv[k + 3]
        from ngmlr_amd import synth
        ref = synth.random_ref(np.random.default_rng(seed), length).tobytes()
        used = "".join(line.strip() for line in open(fasta) if not line.startswith(">")).encode()
        assert ref == used, "the workload's reference is not random_ref(default_rng(seed), length)"
        extra = {"genome_seed": np.int64(seed), "genome_len": np.int64(length), "genome_sha1": np.frombuffer(hashlib.sha1(ref).digest(), dtype=np.uint8)}
    reads = np.zeros((len(recs), 100), dtype=np.uint8)
    for i, r in enumerate(recs):
        b = bytes(r["read"])
        reads[i, :len(b)] = np.frombuffer(b, dtype=np.uint8)[:100]
    np.savez_compressed(out, n=np.int64(len(recs)), calls_recorded=np.int64(len(raw)), on_ref_start=recs["on_ref_start"], mid_ref=recs["mid_ref"],
                        mid_read=recs["mid_read"], position_offset=recs["position_offset"], inv_len=recs["inv_len"], read_len=recs["read_len"],
                        outcome=recs["outcome"], ref_chars=recs["ref_chars"], n_read=recs["n_read"], read=reads,
                        score_fwd=recs["score_fwd"], score_rev=recs["score_rev"], **extra)
    print("%s: %d calls recorded, %d distinct" % (out, len(raw), len(recs)))
    for o, name in OUTCOMES.items():
        sel = recs[recs["outcome"] == o]
        line = "  %-20s %d" % (name, len(sel))
        if o == 0 and len(sel):
            line += "  (window empty: %d, score_rev > score_fwd: %d, window of %d..%d characters)" % (
                int((sel["ref_chars"] == 0).sum()), int((sel["score_rev"] > sel["score_fwd"]).sum()), int(sel["ref_chars"].min()), int(sel["ref_chars"].max()))
        print(line)


if __name__ == "__main__":
    main()
