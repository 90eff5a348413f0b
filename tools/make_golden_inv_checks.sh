#!/bin/bash
# tools/make_golden_inv_checks.sh -- harvest the fixtures of the inversion checks (cvx_inv_checks*, CVX_CREATE_INV_CHECKS) from the
# UNMODIFIED reference pipeline, in the manner of tools/make_golden_read_segments.sh.
#
# A fresh /tmp copy of /root/reference gets a pass-through recorder hook of our own at the three ends of
# AlignmentBuffer::checkForSV (src/AlignmentBuffer.cpp:1158-1235), switched on by an environment variable: per call
# interval->onRefStart, align->PositionOffset, both midpoints, inversionLength, strlen(fullReadSeq), the 100 read characters the
# scoring block was given (or none), both scores, strlen of the decoded window, and which end the call took (0: the scoring block
# ran, 1: inversion too short, 2: no read part).  No window string is stored: the genome is the FASTA under tests/golden/e2e
# (test_3) or the generated reference of the split-read workload (tools/e2e_rates.py write_sv_workload, seed and length recorded).
# ngmlr maps its own test_3 reads and the split-read workload of tests/test_gpu_e2e.py with -t 1;
# tools/pack_golden_inv_checks.py turns the dumps into tests/golden/inv_checks_*.npz and prints the counts per outcome.
# Nothing is written to /root/reference; no reference source enters this repository.  Needs /root/reference, cmake, zlib.
set -euo pipefail
HERE="$(cd "$(dirname "$0")" && pwd)"
REPO="$(dirname "$HERE")"
WORK="$(mktemp -d /tmp/ngmlr_ic.XXXXXX)"
cp -r /root/reference "$WORK/src_tree"
T="$WORK/src_tree"
python3 - "$T/src" <<'PY'
import sys
src = sys.argv[1]
p = src + '/AlignmentBuffer.cpp'
s = open(p).read()
assert s.count('#include "AlignmentBuffer.h"') == 1
s = s.replace('#include "AlignmentBuffer.h"', '''#include "AlignmentBuffer.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
/* recorder hook (tools/make_golden_inv_checks.sh), not part of the reference */
static void cvx_record_check(int outcome, Interval const * interval, Align const * align, char const * fullReadSeq, unsigned long long midRef,
		unsigned long long midRead, int inversionLength, char const * readSeq, char const * refSeq, float scoreFwd, float scoreRev) {
	char const * path = getenv("CVX_RECORD_CHECKS");
	if (path == 0) return;
	FILE * f = fopen(path, "ab");
	long long onRefStart = (long long) interval->onRefStart;
	int a[5] = { align->PositionOffset, inversionLength, (int) strlen(fullReadSeq), outcome, refSeq ? (int) strlen(refSeq) : -1 };
	int nread = readSeq ? (int) strlen(readSeq) : 0;
	char buf[128];
	memset(buf, 0, sizeof(buf));
	if (nread > 0) memcpy(buf, readSeq, (size_t) (nread < 128 ? nread : 128));
	fwrite(&onRefStart, 8, 1, f); fwrite(&midRef, 8, 1, f); fwrite(&midRead, 8, 1, f); fwrite(a, 4, 5, f); fwrite(&nread, 4, 1, f);
	fwrite(buf, 1, 128, f); fwrite(&scoreFwd, 4, 1, f); fwrite(&scoreRev, 4, 1, f);
	fclose(f);
}
''', 1)
ran = '\t\t\tif ((scoreRev / scoreFwd) > Config.getInvScoreRatio() && scoreRev > minScore) {\n'
assert s.count(ran) == 1
s = s.replace(ran, '\t\t\tcvx_record_check(0, interval, align, fullReadSeq, inversionMidpointOnRef, inversionMidpointOnRead, inversionLength, readSeq, refSeq, scoreFwd, scoreRev);   /* recorder hook */\n' + ran, 1)
noread = '\t\t\tverbose(0, true, "Skipping alignment. Readpart not long enough.");\n'
assert s.count(noread) == 1
s = s.replace(noread, noread + '\t\t\tcvx_record_check(2, interval, align, fullReadSeq, inversionMidpointOnRef, inversionMidpointOnRead, inversionLength, 0, refSeq, 0.0f, 0.0f);   /* recorder hook */\n', 1)
short = '\t} else {\n\t\tif(pacbioDebug) {\n\t\t\tLog.Message("Inversion too short!");\n'
assert s.count(short) == 1
s = s.replace(short, '\t} else {\n\t\tcvx_record_check(1, interval, align, fullReadSeq, inversionMidpointOnRef, inversionMidpointOnRead, inversionLength, 0, 0, 0.0f, 0.0f);   /* recorder hook */\n\t\tif(pacbioDebug) {\n\t\t\tLog.Message("Inversion too short!");\n', 1)
open(p, 'w').write(s)
PY
mkdir -p "$T/build" && cd "$T/build"
cmake .. -DCMAKE_POLICY_VERSION_MINIMUM=3.5 -DCMAKE_BUILD_TYPE=RELWITHDEBINFO > "$WORK/cmake.log" 2>&1
make -j16 > "$WORK/make.log" 2>&1 || { tail -30 "$WORK/make.log"; exit 1; }
BIN=$(ls "$T"/bin/ngmlr-*/ngmlr)
D="$T/test/data"
cd "$WORK"
CVX_RECORD_CHECKS="$WORK/test_3.chk" "$BIN" --skip-write -x pacbio -t 1 -R 0.01 --no-progress -r "$D/test_3/reference.fasta.gz" -q "$REPO/tests/golden/e2e/test_3_reads.fq.gz" > "$WORK/test_3.sam" 2> "$WORK/test_3.log" || true
touch "$WORK/test_3.chk"
echo "test_3: $(stat -c %s "$WORK/test_3.chk") bytes of call records"
# the split-read workload of tests/test_gpu_e2e.py::test_split_reads_with_structural_variants
SV_SEED=77
SV_LEN=3000000
PYTHONPATH="$REPO" python3 -c "import sys; sys.path.insert(0, '$REPO/tools'); import e2e_rates; e2e_rates.write_sv_workload('$WORK/sv_ref.fa', '$WORK/sv_reads.fq', 160, seed=$SV_SEED, L=$SV_LEN)"
CVX_RECORD_CHECKS="$WORK/sv.chk" "$BIN" --skip-write -x ont -t 1 -R 0.01 --no-progress -r "$WORK/sv_ref.fa" -q "$WORK/sv_reads.fq" > "$WORK/sv.sam" 2> "$WORK/sv.log" || true
touch "$WORK/sv.chk"
echo "split reads: $(stat -c %s "$WORK/sv.chk") bytes of call records"
PYTHONPATH="$REPO" python3 "$HERE/pack_golden_inv_checks.py" "$WORK/test_3.chk" "$REPO/tests/golden/inv_checks_test_3.npz"
PYTHONPATH="$REPO" python3 "$HERE/pack_golden_inv_checks.py" "$WORK/sv.chk" "$REPO/tests/golden/inv_checks_split.npz" --synth-genome $SV_SEED $SV_LEN "$WORK/sv_ref.fa"
if [ "${KEEP_WORK:-}" = "" ]; then rm -rf "$WORK"; else echo "kept $WORK"; fi
