#!/bin/bash
# tools/make_golden_ladder.sh -- harvest the fixtures of the corridor retry ladder (cvx_ladder_rung, cvx_submit_ladder) from the
# UNMODIFIED reference pipeline, in the manner of tools/make_golden_inv_checks.sh.
#
# A fresh /tmp copy of /root/reference gets a pass-through recorder hook of our own in AlignmentBuffer::computeAlignment
# (src/AlignmentBuffer.cpp:226-425) and in getCorridorEndpointsWithAnchors (:129-197), switched on by an environment variable:
# per call `corridor` as passed (before the clamp at :266), readLength, refSeqLen, realign, fullAlignment, shortRead,
# interval->anchorLength, fullReadLength and the builder's corridorLeft / corridorRight after :178-182, before the multiplier;
# per attempt the multiplier, corridorLines[0].offset, corridorLines[H - 1].offset, the width and SingleAlign's return value.
# No sequence is stored.  ngmlr maps its own test_3 reads and the split-read workload of tests/test_gpu_e2e.py with -t 1;
# tools/pack_golden_ladder.py turns the dumps into tests/golden/ladder_*.npz and prints how many ladders of each length they hold.
# Nothing is written to /root/reference; no reference source enters this repository.  Needs /root/reference, cmake, zlib.
set -euo pipefail
HERE="$(cd "$(dirname "$0")" && pwd)"
REPO="$(dirname "$HERE")"
WORK="$(mktemp -d /tmp/ngmlr_ld.XXXXXX)"
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
/* recorder hook (tools/make_golden_ladder.sh), not part of the reference */
static float cvx_rec_left = 0.0f, cvx_rec_right = 0.0f;
static int cvx_rec_have_lr = 0;
static void cvx_record_line(char const * line) {
	char const * path = getenv("CVX_RECORD_LADDER");
	if (path == 0) return;
	FILE * f = fopen(path, "a");
	fputs(line, f);
	fclose(f);
}
''', 1)
mul = '\tcorridorLeft = corridorLeft * corridorMultiplier;\n'
assert s.count(mul) == 1
s = s.replace(mul, '\tif (!cvx_rec_have_lr) { cvx_rec_left = corridorLeft; cvx_rec_right = corridorRight; cvx_rec_have_lr = 1; }   /* recorder hook */\n' + mul, 1)
clamp = '\t\t\tint const maxCorridorSize = refSeqLen * 2;\n'
assert s.count(clamp) == 1
s = s.replace(clamp, '\t\t\tint const cvx_rec_corridor = corridor; cvx_rec_have_lr = 0; cvx_rec_left = cvx_rec_right = 0.0f;   /* recorder hook */\n' + clamp, 1)
att = '\t\t\t\talignmentId += 1;\n'
assert s.count(att) == 1
s = s.replace(att, '''\t\t\t\t{   /* recorder hook */
\t\t\t\t\tchar cvx_line[256];
\t\t\t\t\tsnprintf(cvx_line, sizeof(cvx_line), "A %d %d %d %d %d %d\\n", corridorMultiplier, corridorHeight, corridorHeight > 0 ? corridorLines[0].offset : 0,
\t\t\t\t\t\t\tcorridorHeight > 0 ? corridorLines[corridorHeight - 1].offset : 0, corridorHeight > 0 ? corridorLines[0].length : 0, cigarLength);
\t\t\t\t\tcvx_record_line(cvx_line);
\t\t\t\t}
''' + att, 1)
end = '\t\t\tdelete[] refSeq;\n\t\t\trefSeq = 0;\n\n\t\t\t#ifdef TEST_ALIGNER\n'
assert s.count(end) == 1
s = s.replace(end, '''\t\t\t{   /* recorder hook */
\t\t\t\tchar cvx_line[320];
\t\t\t\tsnprintf(cvx_line, sizeof(cvx_line), "C %d %d %d %d %d %d %d %d %d %a %a\\n", cvx_rec_corridor, (int) readLength, refSeqLen, (int) realign, (int) fullAlignment,
\t\t\t\t\t\t(int) shortRead, (int) interval->anchorLength, fullReadLength, cvx_rec_have_lr, (double) cvx_rec_left, (double) cvx_rec_right);
\t\t\t\tcvx_record_line(cvx_line);
\t\t\t}
''' + end, 1)
open(p, 'w').write(s)
PY
mkdir -p "$T/build" && cd "$T/build"
cmake .. -DCMAKE_POLICY_VERSION_MINIMUM=3.5 -DCMAKE_BUILD_TYPE=RELWITHDEBINFO > "$WORK/cmake.log" 2>&1
make -j16 > "$WORK/make.log" 2>&1 || { tail -30 "$WORK/make.log"; exit 1; }
BIN=$(ls "$T"/bin/ngmlr-*/ngmlr)
D="$T/test/data"
cd "$WORK"
CVX_RECORD_LADDER="$WORK/test_3.lad" "$BIN" --skip-write -x pacbio -t 1 -R 0.01 --no-progress -r "$D/test_3/reference.fasta.gz" -q "$REPO/tests/golden/e2e/test_3_reads.fq.gz" > "$WORK/test_3.sam" 2> "$WORK/test_3.log" || true
touch "$WORK/test_3.lad"
echo "test_3: $(wc -l < "$WORK/test_3.lad") lines of call and attempt records"
# the split-read workload of tests/test_gpu_e2e.py::test_split_reads_with_structural_variants
SV_SEED=77
SV_LEN=3000000
PYTHONPATH="$REPO" python3 -c "import sys; sys.path.insert(0, '$REPO/tools'); import e2e_rates; e2e_rates.write_sv_workload('$WORK/sv_ref.fa', '$WORK/sv_reads.fq', 160, seed=$SV_SEED, L=$SV_LEN)"
CVX_RECORD_LADDER="$WORK/sv.lad" "$BIN" --skip-write -x ont -t 1 -R 0.01 --no-progress -r "$WORK/sv_ref.fa" -q "$WORK/sv_reads.fq" > "$WORK/sv.sam" 2> "$WORK/sv.log" || true
touch "$WORK/sv.lad"
echo "split reads: $(wc -l < "$WORK/sv.lad") lines of call and attempt records"
PYTHONPATH="$REPO" python3 "$HERE/pack_golden_ladder.py" "$WORK/test_3.lad" "$REPO/tests/golden/ladder_test_3.npz"
PYTHONPATH="$REPO" python3 "$HERE/pack_golden_ladder.py" "$WORK/sv.lad" "$REPO/tests/golden/ladder_split.npz"
if [ "${KEEP_WORK:-}" = "" ]; then rm -rf "$WORK"; else echo "kept $WORK"; fi
