/*
 * regions_cpu_aligner.h -- test-only IAlignment for oracle/_ref/ngmlr_regions_cpu (tools/build_ngmlr_hip.sh): the reference's own
 * Convex::ConvexAlignFast behind the request / note exchange of nm_regions_note.h, no GPU.  A call whose Align::nmPerPosition
 * holds a request (nm_regions_alloc_binding.inc) lets the CPU aligner write its profile into a buffer of the wrapper's, turns
 * that profile into a note with cvx_nm_regions_host and hands the note back, so that both insertion sites and the note run
 * inside ngmlr on a machine without a device (tests/test_regions_binding_cpu.py: SAM identical to the unmodified reference).
 *
 * It also checks what the device finder assumes about the reference: the rows from an accepted alignment's entry
 * count to alignmentLength are zeros, because an accepted alignment is always the first profile written into its buffer.  The
 * wrapper's buffer therefore stands for the reference's: allocated as the reference allocates it when a request arrives and kept
 * over the invalid attempts into the same Align; once a valid profile was written the rows go back and the book keeps the entry
 * count, against which a second valid profile into the same Align (which then holds the first one's note) is judged.  Counted
 * and printed when the process ends: calls that found a row in [entries, min(alignmentLength, buffer rows)) that is not zero,
 * calls that wrote a second valid profile into one buffer, and calls whose alignmentLength exceeds the buffer (the reference's
 * own scan then reads past it).  Compiled only inside ngmlr's tree.
 */
#ifndef REGIONS_CPU_ALIGNER_H
#define REGIONS_CPU_ALIGNER_H

#include <map>
#include <mutex>
#include <vector>

/* (ConvexAlignFast.h comes from AlignmentBuffer.h right in front of this header; its include guard does not survive a second inclusion) */
#include "convex_align_hip.h"
#include "nm_regions_note.h"

namespace Convex {

class RegionsCpuAligner: public IAlignment {
	struct Buffer { PositionNM * rows; int length; int validWrites; int entries; };      /* rows: 0 once a valid profile was written (entries of it kept) */
	struct Book {
		std::mutex mtx;
		std::map<void const *, Buffer> buffers;      /* by the caller's buffer: what the reference would hold in its place */
		long notes, regions, profiles, tailViolations, rewritten, tooLong;
		Book() : notes(0), regions(0), profiles(0), tailViolations(0), rewritten(0), tooLong(0) {}
		~Book() {
			for (std::map<void const *, Buffer>::iterator it = buffers.begin(); it != buffers.end(); ++it) delete[] it->second.rows;
			fprintf(stderr, "RegionsCpuAligner: %ld calls answered with a note (%ld regions), %ld with their profile; violations: %ld profiles with a "
					"row past their entries that is not zero, %ld buffers written twice, %ld alignments longer than their buffer\n",
					notes, regions, profiles, tailViolations, rewritten, tooLong);
			long na = 0, nr = 0, np = 0;
			DeviceRegions::Stats(na, nr, np);
			fprintf(stderr, "RegionsCpuAligner: %ld alignments handed detectMisalignment %ld regions from their note, %ld their profile (CVX_DEVICE_REGIONS=0 turns that off)\n", na, nr, np);
		}
	};
	static Book & book() { static Book b; return b; }
	ConvexAlignFast inner;
public:
	RegionsCpuAligner(int const stdOutMode, float const match, float const mismatch, float const gapOpen, float const gapExtend,
			float const gapExtendMin, float const gapDecay) : inner(stdOutMode, match, mismatch, gapOpen, gapExtend, gapExtendMin, gapDecay) { (void) book(); }
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
		Book & bk = book();
		bool const request = NmRegionsNote::IsRequest(result.nmPerPosition, result.nmPerPostionLength);
		if (!request && !NmRegionsNote::Wanted(result.nmPerPosition, result.nmPerPostionLength)) {
			{ std::lock_guard<std::mutex> lk(bk.mtx); bk.profiles += 1; }
			return inner.SingleAlign(mode, corridor, corridorHeight, refSeq, qrySeq, result, externalQStart, externalQEnd, extData);
		}
		PositionNM * const callers = result.nmPerPosition;
		int const callersLength = result.nmPerPostionLength;
		Buffer mine;
		{
			std::lock_guard<std::mutex> lk(bk.mtx);
			std::map<void const *, Buffer>::iterator it = bk.buffers.find(callers);
			if (it == bk.buffers.end() || request || it->second.rows == 0) {
				/* a request nobody has answered (a new Align, or one whose earlier attempts were invalid and wrote nothing): the buffer
				 * the reference allocates at src/AlignmentBuffer.cpp:277-278.  (An entry under this address with a request in the buffer
				 * is a freed Align's.)  An Align that holds a note already had a valid profile: the wrapper kept only its entry count --
				 * a second valid one is counted as a violation below, with the rows the first would have left behind it. */
				mine.validWrites = 0; mine.entries = 0;
				if (it != bk.buffers.end()) {
					if (!request) { mine.validWrites = it->second.validWrites; mine.entries = it->second.entries; }
					delete[] it->second.rows;
					bk.buffers.erase(it);
				}
				mine.length = (corridorHeight + 1) * 2;
				mine.rows = new PositionNM[mine.length];
			} else {
				mine = it->second;      /* a retry after invalid attempts into the same buffer, whatever it holds */
				bk.buffers.erase(it);
			}
		}
		result.nmPerPosition = mine.rows;
		result.nmPerPostionLength = mine.length;
		int ret = -1;
		try {
			ret = inner.SingleAlign(mode, corridor, corridorHeight, refSeq, qrySeq, result, externalQStart, externalQEnd, extData);
		} catch (...) {
			delete[] result.nmPerPosition;
			result.nmPerPosition = callers; result.nmPerPostionLength = callersLength;
			throw;
		}
		mine.rows = result.nmPerPosition;            /* (addPosition may have replaced it) */
		mine.length = result.nmPerPostionLength;
		result.nmPerPosition = callers;
		result.nmPerPostionLength = callersLength;
		long tail = 0, twice = 0, tooLong = 0, found = 0;
		if (ret >= 0) {
			/* an entry has both positions >= 1 (addPosition, src/ConvexAlignFast.cpp:76-98) and entries are written from row 0 on */
			int entries = 0;
			while (entries < mine.length && mine.rows[entries].refPosition >= 1 && mine.rows[entries].readPosition >= 1) ++entries;
			int const scanned = result.alignmentLength < mine.length ? result.alignmentLength : mine.length;
			if (mine.validWrites > 0) twice = 1;
			if (result.alignmentLength > mine.length) tooLong = 1;
			for (int i = entries; i < scanned; ++i) if (mine.rows[i].refPosition != 0 || mine.rows[i].readPosition != 0 || mine.rows[i].nm != 0) { tail = 1; break; }
			if (mine.validWrites > 0 && mine.entries > entries && entries < scanned) tail = 1;      /* the earlier profile's rows would lie behind this one's */
			mine.validWrites += 1;
			/* the note: what the reference's finder makes of the rows it would scan, stale ones included */
			int64_t n = 0;
			if (cvx_nm_regions_host((int32_t const *) mine.rows, scanned, result.alignmentLength, 0, 0, &n, 0) != CVX_OK) throw 1;
			std::vector<cvx_nm_region> regions((size_t) n + 1);
			if (n > 0 && cvx_nm_regions_host((int32_t const *) mine.rows, scanned, result.alignmentLength, regions.data(), n, &n, 0) != CVX_OK) throw 1;
			NmRegionsNote::Put(result.nmPerPosition, result.nmPerPostionLength, reinterpret_cast<NmRegionsNote::Region const *>(regions.data()), (int) n);
			found = (long) n;
		}
		{
			std::lock_guard<std::mutex> lk(bk.mtx);
			/* (the caller's buffer may have been replaced by Put: the book goes by the one the Align holds now) */
			std::map<void const *, Buffer>::iterator old = bk.buffers.find(result.nmPerPosition);
			if (old != bk.buffers.end()) { delete[] old->second.rows; bk.buffers.erase(old); }
			if (ret >= 0) {      /* an answered Align: its 240 kB go back, the book keeps the count */
				int n = 0;
				while (n < mine.length && mine.rows[n].refPosition >= 1 && mine.rows[n].readPosition >= 1) ++n;
				if (n > mine.entries) mine.entries = n;
				delete[] mine.rows;
				mine.rows = 0; mine.length = 0;
			}
			bk.buffers[result.nmPerPosition] = mine;
			if (ret >= 0) { bk.notes += 1; bk.regions += found; }
			bk.tailViolations += tail; bk.rewritten += twice; bk.tooLong += tooLong;
		}
		return ret;
	}
};

}  // namespace Convex

#endif
