#!/bin/bash
# tools/make_golden_score_windows.sh -- harvest the fixtures of scoring against the resident genome (cvx_score_windows*) from the
# UNMODIFIED reference pipeline, in the manner of tools/make_golden_cs.sh.
#
# A fresh /tmp copy of /root/reference gets pass-through recorder hooks, switched on by environment variables:
#   ScoreBuffer::DoRun (src/ScoreBuffer.cpp:124)          behind BatchScore, per pair: the read's forward Seq and length, the
#   ScoreBuffer::scoreShortRead (src/ScoreBuffer.cpp:267)  location and its strand, the position and buffer length handed to
#                                                          DecodeRefSequence, what that call returns (asked again into a buffer of
#                                                          the hook's own: the function only reads the genome), the two strings
#                                                          that were scored and the score; GetConcatRefLen() with every record
#   _SequenceProvider::Init (src/SequenceProvider.cpp:424) at its end: binRef and its nibble count, and -- given a list of
#                                                          (position, buffer_len) -- what DecodeRefSequence returns and writes
#                                                          for each of them
# ngmlr then maps its own test_3 and test_2 reads with -t 1 and one read over a small synthetic genome (three sequences of 37, 64
# and 1 001 bases, written here and committed beside the fixtures as data); tools/pack_golden_score_windows.py turns the dumps
# into tests/golden/score_windows_{test_3,test_2,cases}.npz.  Nothing is written to /root/reference; no reference source
# enters this repository.  Needs /root/reference, cmake, zlib.
set -euo pipefail
HERE="$(cd "$(dirname "$0")" && pwd)"
REPO="$(dirname "$HERE")"
WORK="$(mktemp -d /tmp/ngmlr_sw.XXXXXX)"
cp -r /root/reference "$WORK/src_tree"
T="$WORK/src_tree"
python3 - "$T/src" <<'PY'
import sys
src = sys.argv[1]
p = src + '/ScoreBuffer.cpp'
s = open(p).read()
s = s.replace('#include "ScoreBuffer.h"', '''#include "ScoreBuffer.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
/* recorder hook (tools/make_golden_score_windows.sh), not part of the reference */
static void cvx_record_pair(int kind, MappedRead * read, SequenceLocation loc, uloc position, uloc bufferLength, char const * ref, char const * qry, float score) {
	char const * path = getenv("CVX_RECORD_SW");
	if (path == 0) return;
	FILE * f = fopen(path, "ab");
	char * tmp = new char[bufferLength + 16];
	memset(tmp, 0, bufferLength + 16);
	int ret = SequenceProvider.DecodeRefSequence(tmp, 0, position, bufferLength) ? 1 : 0;
	delete[] tmp;
	unsigned long long l = loc.m_Location, pos = position, bl = bufferLength, cl = SequenceProvider.GetConcatRefLen();
	int len = read->length, rev = loc.isReverse() ? 1 : 0;
	int wl = (int) strnlen(ref, bufferLength), ql = (int) strlen(qry);
	fwrite(&kind, 4, 1, f); fwrite(&len, 4, 1, f); fwrite(read->Seq, 1, (size_t) len, f);
	fwrite(&l, 8, 1, f); fwrite(&rev, 4, 1, f); fwrite(&pos, 8, 1, f); fwrite(&bl, 8, 1, f); fwrite(&cl, 8, 1, f); fwrite(&ret, 4, 1, f);
	fwrite(&wl, 4, 1, f); fwrite(ref, 1, (size_t) wl, f); fwrite(&ql, 4, 1, f); fwrite(qry, 1, (size_t) ql, f); fwrite(&score, 4, 1, f);
	fclose(f);
}
''', 1)
anchor = '\t\tint res = aligner->BatchScore(0, iScores, m_RefBuffer, m_QryBuffer, m_ScoreBuffer, 0);\n'
assert s.count(anchor) == 1
s = s.replace(anchor, anchor + '''\t\tfor (int cvx_i = 0; cvx_i < iScores; ++cvx_i) {   /* recorder hook */
			SequenceLocation cvx_loc = scores[cvx_i].read->Scores[scores[cvx_i].scoreId].Location;
			cvx_record_pair(0, scores[cvx_i].read, cvx_loc, cvx_loc.m_Location - (corridor >> 1), refMaxLen, m_RefBuffer[cvx_i], m_QryBuffer[cvx_i], m_ScoreBuffer[cvx_i]);
		}
''')
anchor = '\t\taligner->SingleScore(0, corridor, refSeq, qrySeq, score, 0);\n'
assert s.count(anchor) == 1
s = s.replace(anchor, anchor + '\t\tcvx_record_pair(1, read, read->Scores[i].Location, read->Scores[i].Location.m_Location - (corridor >> 1), read->length + corridor, refSeq, qrySeq, score);   /* recorder hook */\n')
open(p, 'w').write(s)
p = src + '/SequenceProvider.cpp'
s = open(p).read()
anchor = '\trefStartPos[j] = refStartPos[j - 1] + SequenceProvider.GetRefLen(refCount - 1) + 1000;\n'
assert s.count(anchor) == 1
s = s.replace(anchor, anchor + '''\tif (getenv("CVX_RECORD_BINREF")) {   /* recorder hook (tools/make_golden_score_windows.sh), not part of the reference */
		FILE * bf = fopen(getenv("CVX_RECORD_BINREF"), "wb");
		unsigned long long nn = binRefIndex, cl = GetConcatRefLen();
		fwrite(&nn, 8, 1, bf); fwrite(&cl, 8, 1, bf); fwrite(binRef, 1, (size_t) (nn / 2), bf);
		fclose(bf);
	}
	if (getenv("CVX_RECORD_CASES_IN") && getenv("CVX_RECORD_CASES_OUT")) {   /* recorder hook */
		FILE * ci = fopen(getenv("CVX_RECORD_CASES_IN"), "r");
		FILE * co = fopen(getenv("CVX_RECORD_CASES_OUT"), "wb");
		unsigned long long cpos; int clen;
		while (fscanf(ci, "%llu %d", &cpos, &clen) == 2) {
			char * cbuf = new char[clen + 16];
			memset(cbuf, 0, clen + 16);
			int cret = DecodeRefSequence(cbuf, 0, cpos, clen) ? 1 : 0;
			fwrite(&cpos, 8, 1, co); fwrite(&clen, 4, 1, co); fwrite(&cret, 4, 1, co); fwrite(cbuf, 1, (size_t) clen + 16, co);
			delete[] cbuf;
		}
		fclose(ci); fclose(co);
	}
''')
open(p, 'w').write(s)
PY
mkdir -p "$T/build" && cd "$T/build"
cmake .. -DCMAKE_POLICY_VERSION_MINIMUM=3.5 -DCMAKE_BUILD_TYPE=RELWITHDEBINFO > "$WORK/cmake.log" 2>&1
make -j16 > "$WORK/make.log" 2>&1 || { tail -30 "$WORK/make.log"; exit 1; }
BIN=$(ls "$T"/bin/ngmlr-*/ngmlr)
D="$T/test/data"
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
CVX_RECORD_SW="$WORK/test_3.sw" CVX_RECORD_BINREF="$WORK/test_3.binref" "$BIN" --skip-write -x pacbio -t 1 -R 0.01 --no-progress \
	-r "$D/test_3/reference.fasta.gz" -q "$WORK/test_3.fq" > "$WORK/test_3.sam" 2> "$WORK/test_3.log" || true
echo "test_3: $(stat -c %s "$WORK/test_3.sw") bytes of pair records"
cp "$D/test_2/ref_chr21_20kb.fa" "$WORK/test_2.fa"
CVX_RECORD_SW="$WORK/test_2.sw" CVX_RECORD_BINREF="$WORK/test_2.binref" "$BIN" --skip-write -x pacbio -t 1 --no-progress \
	-r "$WORK/test_2.fa" -q "$D/test_2/reads_100_2200bp.fa" > "$WORK/test_2.sam" 2> "$WORK/test_2.log" || true
echo "test_2: $(stat -c %s "$WORK/test_2.sw") bytes of pair records"
# the engineered windows: the genome and the list are written by the packer (--cases-in), answered by the hook in Init
python3 "$HERE/pack_golden_score_windows.py" --cases-in "$REPO/tests/golden/score_windows_cases.fa" "$WORK/cases.txt" "$WORK/cases.fq"
cp "$REPO/tests/golden/score_windows_cases.fa" "$WORK/cases.fa"      # (ngmlr writes its caches beside the reference)
CVX_RECORD_BINREF="$WORK/cases.binref" CVX_RECORD_CASES_IN="$WORK/cases.txt" CVX_RECORD_CASES_OUT="$WORK/cases.out" "$BIN" --skip-write -x pacbio -t 1 --no-progress \
	-r "$WORK/cases.fa" -q "$WORK/cases.fq" > "$WORK/cases.sam" 2> "$WORK/cases.log" || true
echo "cases: $(stat -c %s "$WORK/cases.out") bytes of decoded windows"
python3 "$HERE/pack_golden_score_windows.py" --pairs "$WORK/test_3.sw" "$WORK/test_3.binref" "$REPO/tests/golden/decode_test_3.npz" 1600 "$REPO/tests/golden/score_windows_test_3.npz"
python3 "$HERE/pack_golden_score_windows.py" --pairs "$WORK/test_2.sw" "$WORK/test_2.binref" "$REPO/tests/golden/decode_test_2.npz" 1600 "$REPO/tests/golden/score_windows_test_2.npz"
python3 "$HERE/pack_golden_score_windows.py" --cases "$WORK/cases.out" "$WORK/cases.binref" "$REPO/tests/golden/score_windows_cases.fa" "$REPO/tests/golden/score_windows_cases.npz"
if [ "${KEEP_WORK:-}" = "" ]; then rm -rf "$WORK"; else echo "kept $WORK"; fi
