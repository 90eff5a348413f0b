/*
 * ladder_cpu_aligner.h -- test-only IAlignment for oracle/_ref/ngmlr_ladder_cpu (tools/build_ngmlr_hip.sh): the reference's own
 * Convex::ConvexAlignFast behind Convex::LadderAligner, no GPU, the way regions_cpu_aligner.h stands in for the regions.
 * ladder_binding.inc finds the interface with dynamic_cast and hands computeAlignment's retry loop over as one request;
 * SingleLadder climbs it here with the rule the device runs -- cvx_ladder_rung's form of rung m, its rows written out with the
 * expression of include/cvx_align.h (offset[y] = (int) (((float) y - d) / k - right), one width; cvx_corridor_rows would ask a
 * device for the same rows), inner.SingleAlign on them -- and stops at the first attempt that does not return -1.  So the
 * insertion, the left / right fill, the acceptance rule and the counters run inside ngmlr on a machine without a device
 * (tests/test_ladder_binding_cpu.py: SAM identical to the unmodified reference).
 *
 * CVX_DEVICE_LADDER=0: SingleLadder answers false and the reference's loop runs.  CVX_LADDER_DUMP=<file>: one line per call is
 * appended -- corridor, flags, the bits of left and right, ref_len, qry_len, fullReadLength (which the binding announces through
 * CVX_LADDER_CALL_CONTEXT, the aligner's interface does not carry it) and the attempts made -- which the test holds against the
 * calls recorded from the unmodified reference (tests/golden/ladder_*.npz).  Compiled only inside ngmlr's tree.
 */
#ifndef LADDER_CPU_ALIGNER_H
#define LADDER_CPU_ALIGNER_H

#include <mutex>
#include <vector>

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

/* (ConvexAlignFast.h comes from AlignmentBuffer.h right in front of this header; its include guard does not survive a second inclusion) */
#include "convex_align_hip.h"

#define CVX_LADDER_CALL_CONTEXT(fullReadLength) Convex::LadderCpuAligner::CallContext(fullReadLength)

namespace Convex {

class LadderCpuAligner: public IAlignment, public LadderAligner {
	struct Book {
		std::mutex mtx;
		bool on;
		char const * dump;
		long calls, climbed, unresolved;
		Book() : on(true), dump(getenv("CVX_LADDER_DUMP")), calls(0), climbed(0), unresolved(0) {
			char const * e = getenv("CVX_DEVICE_LADDER");
			if (e && atoi(e) == 0) on = false;
		}
		~Book() { fprintf(stderr, "LadderCpuAligner: %ld ladder requests, %ld with attempts >= 2, %ld reported a failed last rung (CVX_DEVICE_LADDER=0 turns that off)\n", calls, climbed, unresolved); }
	};
	static Book & book() { static Book b; return b; }
	static int & fullReadLengthOfCall() { static thread_local int v = -1; return v; }
	ConvexAlignFast inner;
public:
	LadderCpuAligner(int const stdOutMode, float const match, float const mismatch, float const gapOpen, float const gapExtend,
			float const gapExtendMin, float const gapDecay) : inner(stdOutMode, match, mismatch, gapOpen, gapExtend, gapExtendMin, gapDecay) { (void) book(); }
	static void CallContext(int const fullReadLength) { fullReadLengthOfCall() = fullReadLength; }
	virtual int GetScoreBatchSize() const { return inner.GetScoreBatchSize(); }
	virtual int GetAlignBatchSize() const { return inner.GetAlignBatchSize(); }
	virtual int BatchScore(int const mode, int const batchSize, char const * const * const refSeqList, char const * const * const qrySeqList,
			float * const results, void * extData) { return inner.BatchScore(mode, batchSize, refSeqList, qrySeqList, results, extData); }
	virtual int BatchAlign(int const mode, int const batchSize, char const * const * const refSeqList, char const * const * const qrySeqList,
			Align * const results, void * extData) { return inner.BatchAlign(mode, batchSize, refSeqList, qrySeqList, results, extData); }
	virtual int SingleAlign(int const mode, int const corridor, char const * const refSeq, char const * const qrySeq, Align & result, void * extData) {
		return inner.SingleAlign(mode, corridor, refSeq, qrySeq, result, extData);
	}
	virtual int SingleAlign(int const mode, CorridorLine * corridor, int const corridorHeight, char const * const refSeq, char const * const qrySeq,
			Align & result, int const externalQStart, int const externalQEnd, void * extData) {
		return inner.SingleAlign(mode, corridor, corridorHeight, refSeq, qrySeq, result, externalQStart, externalQEnd, extData);
	}
	virtual bool SingleLadder(char const * refSeq, char const * qrySeq, Align & result, int const externalQStart, int const externalQEnd,
			cvx_ladder const & ladder, int & ret, int & rung, int & attempts, int & width) {
		Book & bk = book();
		if (!bk.on) return false;
		cvx_tile t;
		memset(&t, 0, sizeof(t));
		t.ref_len = (int32_t) strlen(refSeq); t.qry_len = (int32_t) strlen(qrySeq);
		int const H = t.qry_len;
		int const readId = result.svType;      /* the binding stored it there once; the loop stores it before every attempt (src/AlignmentBuffer.cpp:362) */
		std::vector<CorridorLine> lines((size_t) (H > 0 ? H : 1));
		ret = -1; rung = attempts = width = 0;
		for (int m = 1;; ++m) {
			cvx_tile form;
			memset(&form, 0, sizeof(form));
			int const rc = cvx_ladder_rung(&t, &ladder, m, &form);
			if (rc < 0) { fprintf(stderr, "LadderCpuAligner: %s\n", cvx_last_error()); throw 1; }
			if (rc == 0) break;
			for (int y = 0; y < H; ++y) {
				lines[(size_t) y].offset = form.corridor_kind == CVX_CORRIDOR_CONST ? form.corridor_offset : (int) (((float) y - form.corridor_d) / form.corridor_k - form.corridor_right);
				lines[(size_t) y].length = form.corridor_width;
				lines[(size_t) y].offsetInMatrix = 0;
			}
			rung = attempts = m;
			width = form.corridor_width;
			result.svType = readId;
			ret = inner.SingleAlign(0, lines.data(), H, refSeq, qrySeq, result, externalQStart, externalQEnd, 0);
			if (ret != -1) break;
		}
		std::lock_guard<std::mutex> lk(bk.mtx);
		bk.calls += 1;
		if (attempts >= 2) bk.climbed += 1;
		if (ret < 0) bk.unresolved += 1;
		if (bk.dump) {
			uint32_t lb, rb;
			memcpy(&lb, &ladder.left, 4); memcpy(&rb, &ladder.right, 4);
			if (FILE * f = fopen(bk.dump, "a")) {
				fprintf(f, "%d %d %08x %08x %d %d %d %d\n", ladder.corridor, ladder.flags, lb, rb, t.ref_len, t.qry_len, fullReadLengthOfCall(), attempts);
				fclose(f);
			}
		}
		return true;
	}
};

}  // namespace Convex

#endif
