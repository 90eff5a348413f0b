#!/bin/bash
# tools/make_golden_read_segments.sh -- harvest the fixtures of alignment queries taken as segments of a read block
# (cvx_submit_segments, cvx_stage_segments*) from the UNMODIFIED reference pipeline, in the manner of
# tools/make_golden_score_windows.sh.
#
# A fresh /tmp copy of /root/reference gets a pass-through recorder hook of our own at the end of the five-argument
# AlignmentBuffer::extractReadSeq (src/AlignmentBuffer.cpp:1515-1542), switched on by environment variables: per call the read's
# Seq and length, onReadStart, readSeqLen, isReverse, revComp and the string the function returns.  Given a file of engineered reads
# (N, lower case, other printable bytes) and a list of (read, start, len, isReverse, revComp), the first call of the function also
# answers that list with the reference's own function, on MappedRead objects the hook fills itself (no parser in between).
# ngmlr then maps its own test_3 reads (their FASTQ form, tests/golden/e2e: FASTA + reverse strand crashes the reference) and the split-read workload of tests/test_gpu_e2e.py (tools/e2e_rates.py: inversions, so
# revComp = true occurs) with -t 1; tools/pack_golden_read_segments.py turns the dumps into tests/golden/read_segments_*.npz.
# Nothing is written to /root/reference; no reference source enters this repository.  Needs /root/reference, cmake, zlib.
set -euo pipefail
HERE="$(cd "$(dirname "$0")" && pwd)"
REPO="$(dirname "$HERE")"
WORK="$(mktemp -d /tmp/ngmlr_rs.XXXXXX)"
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
/* recorder hook (tools/make_golden_read_segments.sh), not part of the reference */
static bool cvx_cases_active = false;
static void cvx_record_seg(MappedRead * read, int onReadStart, int readSeqLen, bool isReverse, bool revComp, char const * out) {
	char const * path = getenv(cvx_cases_active ? "CVX_RECORD_SEG_CASES_OUT" : "CVX_RECORD_SEG");
	if (path == 0) return;
	FILE * f = fopen(path, "ab");
	int len = read->length, a[4] = { onReadStart, readSeqLen, isReverse ? 1 : 0, revComp ? 1 : 0 }, ol = (int) strlen(out);
	fwrite(&len, 4, 1, f); fwrite(read->Seq, 1, (size_t) len, f); fwrite(a, 4, 4, f); fwrite(&ol, 4, 1, f); fwrite(out, 1, (size_t) ol, f);
	fclose(f);
}
''', 1)
head = '\t// > 500000 very basic check for overflows (this is terrible)\n'
assert s.count(head) == 1
s = s.replace(head, '''	{   /* recorder hook: the engineered list, answered by this very function, once */
		static bool cvx_cases_done = false;
		if (!cvx_cases_done && getenv("CVX_RECORD_SEG_READS") && getenv("CVX_RECORD_SEG_CASES_IN") && getenv("CVX_RECORD_SEG_CASES_OUT")) {
			cvx_cases_done = true;
			std::vector<MappedRead *> cvx_reads;
			FILE * rf = fopen(getenv("CVX_RECORD_SEG_READS"), "rb");
			int rl = 0;
			while (fread(&rl, 4, 1, rf) == 1) {
				MappedRead * r = new MappedRead(0, rl + 16);
				r->Seq = new char[rl + 16];
				memset(r->Seq, 0, rl + 16);
				if (fread(r->Seq, 1, (size_t) rl, rf) != (size_t) rl) break;
				r->length = rl;
				cvx_reads.push_back(r);
			}
			fclose(rf);
			FILE * ci = fopen(getenv("CVX_RECORD_SEG_CASES_IN"), "r");
			int cr, cs, cl, cv, cc;
			cvx_cases_active = true;
			while (fscanf(ci, "%d %d %d %d %d", &cr, &cs, &cl, &cv, &cc) == 5) (void) extractReadSeq(cl, cs, cv != 0, cvx_reads[cr], cc != 0);
			cvx_cases_active = false;
			fclose(ci);
		}
		cvx_cases_done = true;
	}
''' + head, 1)
for ret, var in (('\t\treturn tmp;\n', 'tmp'), ('\t\treturn readSeq;\n', 'readSeq')):
    assert s.count(ret) == 1
    s = s.replace(ret, '\t\tcvx_record_seg(read, onReadStart, readSeqLen, isReverse, revComp, %s.get());   /* recorder hook */\n' % var + ret, 1)
open(p, 'w').write(s)
PY
mkdir -p "$T/build" && cd "$T/build"
cmake .. -DCMAKE_POLICY_VERSION_MINIMUM=3.5 -DCMAKE_BUILD_TYPE=RELWITHDEBINFO > "$WORK/cmake.log" 2>&1
make -j16 > "$WORK/make.log" 2>&1 || { tail -30 "$WORK/make.log"; exit 1; }
BIN=$(ls "$T"/bin/ngmlr-*/ngmlr)
D="$T/test/data"
cd "$WORK"
# the engineered reads (committed as data) and the list the hook answers: written by the packer
python3 "$HERE/pack_golden_read_segments.py" --cases-in "$REPO/tests/golden/read_segments_cases.txt" "$WORK/cases.reads" "$WORK/cases.txt"
CVX_RECORD_SEG="$WORK/test_3.seg" CVX_RECORD_SEG_READS="$WORK/cases.reads" CVX_RECORD_SEG_CASES_IN="$WORK/cases.txt" CVX_RECORD_SEG_CASES_OUT="$WORK/cases.seg" \
	"$BIN" --skip-write -x pacbio -t 1 -R 0.01 --no-progress -r "$D/test_3/reference.fasta.gz" -q "$REPO/tests/golden/e2e/test_3_reads.fq.gz" > "$WORK/test_3.sam" 2> "$WORK/test_3.log" || true
echo "test_3: $(stat -c %s "$WORK/test_3.seg") bytes of call records, cases: $(stat -c %s "$WORK/cases.seg") bytes"
# the split-read workload of tests/test_gpu_e2e.py::test_split_reads_with_structural_variants
PYTHONPATH="$REPO" python3 -c "import sys; sys.path.insert(0, '$REPO/tools'); import e2e_rates; e2e_rates.write_sv_workload('$WORK/sv_ref.fa', '$WORK/sv_reads.fq', 160, seed=77)"
CVX_RECORD_SEG="$WORK/sv.seg" "$BIN" --skip-write -x ont -t 1 -R 0.01 --no-progress -r "$WORK/sv_ref.fa" -q "$WORK/sv_reads.fq" > "$WORK/sv.sam" 2> "$WORK/sv.log" || true
echo "split reads: $(stat -c %s "$WORK/sv.seg") bytes of call records"
python3 "$HERE/pack_golden_read_segments.py" --pack "$WORK/test_3.seg" "$REPO/tests/golden/read_segments_test_3.npz"
python3 "$HERE/pack_golden_read_segments.py" --pack "$WORK/sv.seg" "$REPO/tests/golden/read_segments_split.npz"
python3 "$HERE/pack_golden_read_segments.py" --pack "$WORK/cases.seg" "$REPO/tests/golden/read_segments_cases.npz"
if [ "${KEEP_WORK:-}" = "" ]; then rm -rf "$WORK"; else echo "kept $WORK"; fi
