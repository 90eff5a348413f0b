"""tools/pack_golden_ladder.py DUMP OUT.npz -- the call and attempt lines the recorder hook of tools/make_golden_ladder.sh wrote in
the reference's computeAlignment, as arrays (tests/golden/ladder_*.npz): `calls` (one per computeAlignment call that reached the
retry loop) and `attempts` (its attempts, in order, n_attempts per call).  Identical ladders are stored once.  Prints how many
ladders of each length the recording holds, and how many ended valid."""
import sys

import numpy as np

CALL = np.dtype([("corridor", "<i4"), ("read_length", "<i4"), ("ref_len", "<i4"), ("realign", "<i4"), ("full", "<i4"), ("short_read", "<i4"),
                 ("anchor_length", "<i4"), ("full_read_length", "<i4"), ("have_lr", "<i4"), ("left", "<f4"), ("right", "<f4"), ("n_attempts", "<i4")])
ATTEMPT = np.dtype([("multiplier", "<i4"), ("height", "<i4"), ("off_first", "<i4"), ("off_last", "<i4"), ("width", "<i4"), ("ret", "<i4")])


def main():
    dump, out = sys.argv[1], sys.argv[2]
    ladders = {}
    pending = []
    for line in open(dump):
        f = line.split()
        if f[0] == "A":
            pending.append(tuple(int(x) for x in f[1:7]))
        else:
            assert f[0] == "C" and len(f) == 12
            left, right = float.fromhex(f[10]), float.fromhex(f[11])
            assert float(np.float32(left)) == left and float(np.float32(right)) == right      # binary32 values, printed exactly
            call = tuple(int(x) for x in f[1:10]) + (left, right, len(pending))
            assert all(a[1] == call[1] for a in pending), "corridorHeight is the read's length"
            ladders.setdefault((call, tuple(pending)), 0)
            ladders[(call, tuple(pending))] += 1
            pending = []
    assert not pending, "attempt lines without their call line"
    keys = sorted(ladders)
    calls = np.array([k[0] for k in keys], dtype=CALL) if keys else np.zeros(0, CALL)
    attempts = np.array([a for k in keys for a in k[1]], dtype=ATTEMPT) if keys else np.zeros(0, ATTEMPT)
    np.savez_compressed(out, calls=calls, attempts=attempts, times_seen=np.array([ladders[k] for k in keys], dtype=np.int64))
    by_len = {}
    at = 0
    for c in calls:
        n = int(c["n_attempts"])
        ok = n > 0 and int(attempts[at + n - 1]["ret"]) == int(c["full_read_length"])
        by_len.setdefault(n, [0, 0])
        by_len[n][0] += 1
        by_len[n][1] += ok
        at += n
    print("%s: %d distinct ladders (%d calls), %d attempts" % (out, len(calls), sum(ladders.values()), len(attempts)))
    for n in sorted(by_len):
        print("  length %d: %d ladders, %d of them ended valid" % (n, by_len[n][0], by_len[n][1]))
    kinds = {"full": int((calls["full"] != 0).sum()), "short": int((calls["short_read"] != 0).sum()), "realign": int((calls["realign"] != 0).sum()),
             "anchors": int(((calls["anchor_length"] > 0) & (calls["realign"] == 0) & (calls["full"] == 0) & (calls["short_read"] == 0)).sum()),
             "corridor > 2 * ref_len": int((calls["corridor"] > 2 * calls["ref_len"]).sum())}
    print("  " + ", ".join("%s: %d" % kv for kv in kinds.items()))


if __name__ == "__main__":
    main()
