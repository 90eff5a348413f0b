#!/bin/bash
# tools/make_golden_twin.sh -- record the scalar twin's fixtures from the UNMODIFIED reference sources.
#
# Compiles the reference's own Convex::ConvexAlign (src/ConvexAlign.cpp + src/AlignmentMatrix.cpp plus the one
# `_config` global, by path, behind tools/ref_recorder/twin_wrap.cpp) into oracle/_ref/libcvx_oracle_twin.so
# (git-ignored), then runs tools/pack_golden_twin.py, which writes data only: tests/golden/twin_xfree.npz and
# tests/golden/twin_x.npz (inputs, the twin's outputs and, per tile, ConvexAlignFast's outputs on the same input).
# Then the end-to-end fixtures of --nosse: the reference's ngmlr is built twice in a temporary copy, unmodified and with its one
# `new Convex::ConvexAlign(...)` (src/AlignmentBuffer.h:346) wrapped in tools/ref_recorder/recording_aligner.h (a pure pass-through
# decorator), and run with --nosse on its own test data: tests/golden/test_2.nosse.sam, test_4.nosse.sam and
# test_3.nosse.sorted.sam.gz hold the SAM records of the UNMODIFIED binary (the recording build must print the same), and
# tests/golden/nosse_calls.txt how many SingleAlign calls each run made and how many of their windows carry an 'x'.
# Nothing is written to the reference tree; no reference source enters this repository.
#
#   REF=<reference>/src tools/make_golden_twin.sh            build the library and record again
#   REF=<reference>/src tools/make_golden_twin.sh --lib      build the library only (the fixture-honesty test re-runs it)
set -euo pipefail
HERE="$(cd "$(dirname "$0")" && pwd)"
REPO="$(dirname "$HERE")"
REF="${REF:-/root/reference/src}"
CXX="${CXX:-g++}"
[ -f "$REF/ConvexAlign.cpp" ] || { echo "reference sources not present at $REF" >&2; exit 1; }
mkdir -p "$REPO/oracle/_ref"
"$CXX" -O2 -g -std=c++11 -pthread -fPIC -shared -w -I"$REF" -I"$REPO/oracle" \
	-o "$REPO/oracle/_ref/libcvx_oracle_twin.so" \
	"$HERE/ref_recorder/twin_wrap.cpp" "$REF/ConvexAlign.cpp" "$REF/AlignmentMatrix.cpp"
echo "built oracle/_ref/libcvx_oracle_twin.so"
[ "${1:-}" = "--lib" ] && exit 0
# the ConvexAlignFast side of every tile comes from the checker the oracle's own recipe builds
[ -f "$REPO/oracle/_ref/libcvx_oracle_ref.so" ] || make -s -C "$REPO/oracle" ref
python3 "$HERE/pack_golden_twin.py" "$REPO/oracle/_ref/libcvx_oracle_twin.so" "$REPO/oracle/_ref/libcvx_oracle_ref.so" "$REPO/tests/golden"

# ---- ngmlr --nosse end to end (needs cmake and zlib, like tools/make_golden.sh)
REFROOT="$(dirname "$REF")"
WORK="$(mktemp -d /tmp/ngmlr_twin_rec.XXXXXX)"
for v in plain rec; do cp -r "$REFROOT" "$WORK/$v"; done
cp "$HERE/ref_recorder/recording_aligner.h" "$WORK/rec/src/"
python3 - "$WORK/rec/src/AlignmentBuffer.h" <<'PY'
import sys, re
p = sys.argv[1]
s = open(p).read()
s = s.replace('#include "ConvexAlignFast.h"', '#include "ConvexAlignFast.h"\n#include "recording_aligner.h"', 1)
pat = re.compile(r'aligner = new Convex::ConvexAlign\((.*?)\);', re.S)
assert len(pat.findall(s)) == 1, "construction site of the --nosse branch not found"
s = pat.sub(lambda m: 'aligner = new RecordingAligner(new Convex::ConvexAlign(' + m.group(1) + '));', s)
open(p, 'w').write(s)
PY
for v in plain rec; do
  ( mkdir -p "$WORK/$v/build" && cd "$WORK/$v/build" && cmake .. -DCMAKE_POLICY_VERSION_MINIMUM=3.5 -DCMAKE_BUILD_TYPE=RELWITHDEBINFO > "$WORK/$v.cmake.log" 2>&1 && make -j8 > "$WORK/$v.make.log" 2>&1 ) &
done
wait
D="$REFROOT/test/data"
python3 - "$D/test_3/read.fa.gz" "$WORK/test_3.fq" <<'PY'
import sys, gzip
name = None; seq = []
out = open(sys.argv[2], 'w')
def flush():
    if name is not None:
        s = ''.join(seq)
        out.write('@%s\n%s\n+\n%s\n' % (name, s, 'I' * len(s)))
for line in gzip.open(sys.argv[1], 'rt'):
    line = line.rstrip()
    if line.startswith('>'):
        flush(); name = line[1:]; seq = []
    else:
        seq.append(line)
flush(); out.close()
PY
run() { # name, args...
  local name=$1; shift
  for v in plain rec; do
    local BIN=$(ls "$WORK/$v"/bin/ngmlr-*/ngmlr)
    CVX_RECORD="$WORK/$name.rec" "$BIN" --skip-write --nosse "$@" 2> "$WORK/$name.$v.log" | grep -v '^@' | LC_ALL=C sort > "$WORK/$name.$v.sam"
  done
  cmp "$WORK/$name.plain.sam" "$WORK/$name.rec.sam"      # the decorator changes nothing
  echo "$name: $(wc -l < "$WORK/$name.plain.sam") SAM records under --nosse"
}
run test_2 -t 1 -r "$D/test_2/ref_chr21_20kb.fa" -q "$D/test_2/reads_100_2200bp.fa"
run test_4 -x pacbio -t 1 -r "$D/test_4/reference.fasta.gz" -q "$D/test_4/read.fa.gz"
run test_3 -x pacbio -t 1 -R 0.01 -r "$D/test_3/reference.fasta.gz" -q "$WORK/test_3.fq"
cp "$WORK/test_2.plain.sam" "$REPO/tests/golden/test_2.nosse.sam"
cp "$WORK/test_4.plain.sam" "$REPO/tests/golden/test_4.nosse.sam"
gzip -9 -n -c "$WORK/test_3.plain.sam" > "$REPO/tests/golden/test_3.nosse.sorted.sam.gz"
python3 - "$HERE" "$WORK" "$REPO/tests/golden/nosse_calls.txt" <<'PY'
import os, sys
sys.path.insert(0, sys.argv[1])
import pack_golden
with open(sys.argv[3], 'w') as out:
    out.write("# ngmlr --nosse on the reference's test data: SingleAlign calls of the run, and how many of their reference windows carry an 'x'\n")
    for name in ('test_2', 'test_3', 'test_4'):
        recs = pack_golden.read_records(os.path.join(sys.argv[2], name + '.rec'))
        out.write("%s %d %d\n" % (name, len(recs), sum(b'x' in r['ref'] for r in recs)))
print(open(sys.argv[3]).read())
PY
rm -rf "$WORK"
