/*
 * nm_regions_note.h -- regions instead of a profile, in the buffer the profile would have gone to.
 *
 * Align::nmPerPosition has one reader: the peak finder at the top of AlignmentBuffer::detectMisalignment (reference
 * src/AlignmentBuffer.cpp:1316-1395), which reduces some ten thousand rows to four or five regions.  A job of a
 * CVX_CREATE_NM_REGIONS handle brings those regions back with its results (cvx_job_regions), so a caller that wants nothing
 * else says so IN the buffer, and the aligner answers in it -- the idiom of the read-segment placeholder (DeviceReads,
 * convex_align_hip.h): nothing is kept per thread or fiber, a buffer is recognised by its content alone.
 *
 *   request   row 0 = (kMagicRef, kMagicRead, kRequest): "the caller wants regions, not a profile".
 *   note      row 0 = (kMagicRef, kMagicRead, -1 - n), then n regions of four ints each, packed from row 1 on:
 *             what ConvexAlignHip::Finish writes over a request after a valid alignment.
 *   checks    row 0 = (kMagicRef, kMagicRead, kChecksBase - n), then the n regions as in a note and behind them n check records
 *   note      of 16 bytes each, in the same order (Check: the layout of cvx_inv_check): what Finish writes when the job brought
 *             the inversion checks of its regions (Convex::DeviceInvChecks, convex_align_hip.h).  A regions-only header lies in
 *             [-1 - INT32_MAX / 8, -1], a checks header in [kChecksBase - INT32_MAX / 8, kChecksBase], the request is INT32_MIN:
 *             the third int alone tells the three apart, and IsNote never takes a checks note (nor IsChecksNote a note).
 *
 * A row of a profile is (refPosition, readPosition, nm) with both positions >= 1 and 0 <= nm <= 32 (addPosition,
 * src/ConvexAlignFast.cpp:76-98), a fresh buffer is zeros: neither has a negative first row, so neither is ever taken for a
 * request or a note of either form.  Rows are three ints (PositionNM, src/IAlignment.h:16-21); this header knows neither that type nor
 * HIP nor the library's own headers.
 */
#ifndef NM_REGIONS_NOTE_H
#define NM_REGIONS_NOTE_H

#include <stdint.h>
#include <string.h>

namespace Convex {

struct NmRegionsNote {
	struct Region { int32_t refStart, refStop, readStart, readStop; };      /* startInv, stopInv, startInvRead, stopInvRead: the layout of cvx_nm_region */
	static int32_t const kMagicRef = -0x4E4D5247;       /* "NMRG", negated */
	static int32_t const kMagicRead = -0x4E4F5445;      /* "NOTE", negated */
	static int32_t const kRequest = INT32_MIN;
	struct Check { float scoreFwd, scoreRev; int32_t status, windowChars; };      /* the layout of cvx_inv_check */
	static int32_t const kChecksBase = -0x40000000;

	/* rows (12 bytes each) a note of n regions takes: the header and 4 n ints */
	static int RowsFor(int n) { return 1 + (4 * n + 2) / 3; }
	/* rows a checks note of n regions takes: the header, 4 n ints of regions and 4 n ints of check records */
	static int RowsForChecks(int n) { return 1 + (8 * n + 2) / 3; }
	/* rows: the buffer (capRows >= 1 rows of three ints) */
	static void Request(void * rows) {
		int32_t const head[3] = { kMagicRef, kMagicRead, kRequest };
		memcpy(rows, head, sizeof(head));
	}
	static bool IsRequest(void const * rows, int capRows) {
		int32_t head[3];
		if (rows == 0 || capRows < 1) return false;
		memcpy(head, rows, sizeof(head));
		return head[0] == kMagicRef && head[1] == kMagicRead && head[2] == kRequest;
	}
	/* true: the buffer holds a note (whole: a header whose regions would not fit the buffer is not one); n = its regions */
	static bool IsNote(void const * rows, int capRows, int & n) {
		int32_t head[3];
		if (rows == 0 || capRows < 1) return false;
		memcpy(head, rows, sizeof(head));
		if (head[0] != kMagicRef || head[1] != kMagicRead || head[2] >= 0 || head[2] == kRequest) return false;
		int64_t const count = -1 - (int64_t) head[2];
		if (count > (int64_t) (INT32_MAX / 8) || RowsFor((int) count) > capRows) return false;
		n = (int) count;
		return true;
	}
	/* true: the buffer holds a checks note (whole, as for IsNote); n = its regions, each with a check record */
	static bool IsChecksNote(void const * rows, int capRows, int & n) {
		int32_t head[3];
		if (rows == 0 || capRows < 1) return false;
		memcpy(head, rows, sizeof(head));
		if (head[0] != kMagicRef || head[1] != kMagicRead || head[2] > kChecksBase || head[2] == kRequest) return false;
		int64_t const count = (int64_t) kChecksBase - (int64_t) head[2];
		if (count > (int64_t) (INT32_MAX / 8) || RowsForChecks((int) count) > capRows) return false;
		n = (int) count;
		return true;
	}
	/* a request, or the note (of either form) an earlier alignment into the same buffer left: either way the caller wants regions */
	static bool Wanted(void const * rows, int capRows) {
		int n = 0;
		return IsRequest(rows, capRows) || IsNote(rows, capRows, n) || IsChecksNote(rows, capRows, n);
	}
	/* false (nothing written): the buffer is too small, the caller grows it to RowsFor(n) rows and writes again */
	static bool Write(void * rows, int capRows, Region const * regions, int n) {
		if (rows == 0 || n < 0 || RowsFor(n) > capRows) return false;
		int32_t const head[3] = { kMagicRef, kMagicRead, -1 - n };
		memcpy(rows, head, sizeof(head));
		if (n > 0) memcpy((char *) rows + sizeof(head), regions, (size_t) n * sizeof(Region));
		return true;
	}
	/* the checks note: as Write, with checks[i] the record of regions[i] */
	static bool WriteChecks(void * rows, int capRows, Region const * regions, Check const * checks, int n) {
		if (rows == 0 || n < 0 || n > INT32_MAX / 8 || RowsForChecks(n) > capRows || (n > 0 && (regions == 0 || checks == 0))) return false;
		int32_t const head[3] = { kMagicRef, kMagicRead, kChecksBase - n };
		memcpy(rows, head, sizeof(head));
		if (n > 0) {
			memcpy((char *) rows + sizeof(head), regions, (size_t) n * sizeof(Region));
			memcpy((char *) rows + sizeof(head) + (size_t) n * sizeof(Region), checks, (size_t) n * sizeof(Check));
		}
		return true;
	}
	/* the check record of region i of a checks note of n regions (IsChecksNote said so); its regions are read with At */
	static Check CheckAt(void const * rows, int n, int i) {
		Check c;
		memcpy(&c, (char const *) rows + 3 * sizeof(int32_t) + (size_t) n * sizeof(Region) + (size_t) i * sizeof(Check), sizeof(c));
		return c;
	}
	/* region i of a note of either form (IsNote / IsChecksNote said so); copied out: the rows are aligned for ints, not for anything wider */
	static Region At(void const * rows, int i) {
		Region r;
		memcpy(&r, (char const *) rows + 3 * sizeof(int32_t) + (size_t) i * sizeof(Region), sizeof(r));
		return r;
	}
	/* what a path without regions does to a request or a stale note before it writes a profile: the rows it held are zeros
	 * again, as new PositionNM[] left them */
	static void Clear(void * rows, int capRows) {
		int n = 0;
		if (IsNote(rows, capRows, n)) memset(rows, 0, (size_t) RowsFor(n) * 3 * sizeof(int32_t));
		else if (IsChecksNote(rows, capRows, n)) memset(rows, 0, (size_t) RowsForChecks(n) * 3 * sizeof(int32_t));
		else if (IsRequest(rows, capRows)) memset(rows, 0, 3 * sizeof(int32_t));
	}
	/* What an aligner does with the buffer once it has a VALID alignment (an invalid one touches nothing: the request stays for
	 * the caller's retry).  true: the caller wants regions and the aligner has them -- no profile is written, Put follows.
	 * false: a profile is written as always; a request or stale note was cleared first, so that none is ever left where a
	 * profile is expected (an alignment may have no entry at all). */
	static bool Begin(void * rows, int capRows, bool haveRegions) {
		if (!Wanted(rows, capRows)) return false;
		if (haveRegions) return true;
		Clear(rows, capRows);
		return false;
	}
	/* The same moment on a path WITHOUT regions (a plain handle, the device text stage): true when the buffer held a request or a
	 * stale note.  The caller allocated a small buffer because it asked for regions; what reads the profile scans alignmentLength
	 * rows of it, so the buffer becomes the one the caller would have allocated had it not asked -- 2 * (readLength + 1) zeroed rows
	 * (src/AlignmentBuffer.cpp:277-278) -- before the profile is written, and CoverScan follows once alignmentLength is known. */
	template <typename Row>
	static bool BeginProfile(Row * & rows, int & capRows, int readLength) {
		static_assert(sizeof(Row) == 3 * sizeof(int32_t), "a profile row is three ints");
		if (!Wanted(rows, capRows)) return false;
		int const need = 2 * (readLength + 1);
		if (capRows < need) {
			delete[] rows;
			rows = new Row[need];
			capRows = need;
		} else {
			Clear(rows, capRows);
		}
		return true;
	}
	/* after the profile of `entries` rows was written into a buffer BeginProfile prepared: never fewer rows than the alignmentLength
	 * its reader scans -- the entries kept, zeros behind them */
	template <typename Row>
	static void CoverScan(Row * & rows, int & capRows, int entries, int alignmentLength) {
		if (alignmentLength <= capRows) return;
		Row * const grown = new Row[alignmentLength];
		int const keep = entries < capRows ? entries : capRows;
		if (keep > 0) memcpy((void *) grown, (void const *) rows, (size_t) keep * sizeof(Row));
		delete[] rows;
		rows = grown;
		capRows = alignmentLength;
	}
	/* the note into the caller's buffer, grown when it is too small the way addPosition grows it (delete[] / new Row[], the
	 * capacity doubled until it fits); Row: the caller's 12-byte row type, PositionNM */
	template <typename Row>
	static void Put(Row * & rows, int & capRows, Region const * regions, int n) {
		static_assert(sizeof(Row) == 3 * sizeof(int32_t), "a profile row is three ints");
		int const need = RowsFor(n);
		if (need > capRows) {
			int cap = capRows > 0 ? capRows : 64;
			while (cap < need) cap *= 2;
			delete[] rows;
			rows = new Row[cap];
			capRows = cap;
		}
		(void) Write(rows, capRows, regions, n);
	}
	/* the checks note into the caller's buffer, grown by Put's rule */
	template <typename Row>
	static void PutChecks(Row * & rows, int & capRows, Region const * regions, Check const * checks, int n) {
		static_assert(sizeof(Row) == 3 * sizeof(int32_t), "a profile row is three ints");
		int const need = RowsForChecks(n);
		if (need > capRows) {
			int cap = capRows > 0 ? capRows : 64;
			while (cap < need) cap *= 2;
			delete[] rows;
			rows = new Row[cap];
			capRows = cap;
		}
		(void) WriteChecks(rows, capRows, regions, checks, n);
	}
};

}  // namespace Convex

#endif
