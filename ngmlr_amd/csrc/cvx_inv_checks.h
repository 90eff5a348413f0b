/*
 * cvx_inv_checks.h -- the inversion check of one low-identity region: what AlignmentBuffer::checkForSV (reference
 * src/AlignmentBuffer.cpp:1158-1235) does with every region the peak finder of detectMisalignment hands it (:1360-1366), up to
 * the two scores its decision reads (:1217-1227).  A window of the genome around the region's midpoint on the reference,
 * decoded by DecodeRefSequence (the window rule of cvx_score_windows.h), against the 100 read bases around the midpoint on the
 * read and against their reverse complement (computeReverseSeq / cplBase, :1117-1141), both with StrippedSW::SingleScore.
 *
 * inv_check_plan is the one statement of everything but the scores; inv_checks_kernel (cvx_inv_checks.hip) calls it on the
 * device, inv_checks_host below on the host.  Free of HIP but for the launch declaration -- a plain C++ compiler sees the rest
 * (cvx_inv_checks_host needs no device).  Kept apart from cvx_types.h / cvx_launch.h, whose bytes name the fill / search kernel
 * families (Makefile FILL_ID / SEARCH_ID).
 */
#ifndef CVX_INV_CHECKS_H
#define CVX_INV_CHECKS_H

#include <stdint.h>

#include "cvx_score_windows.h"

namespace cvx {

struct InvCheck {         /* same layout as cvx_inv_check (include/cvx_align.h) */
	float score_fwd, score_rev;
	int32_t status;
	int32_t window_chars;
};

static const int kInvReadHalf = 50;       /* readCheckLength (:1164) */
static const int kInvRefHalf = 250;       /* refCheckLength (:1167) */
static const int kInvMinLen = 10;         /* minInversionLength (:1170) */
static const int kInvQry = 2 * kInvReadHalf;
static const int kInvMaxSeqLen = 100000;  /* maxSeqLen (src/StrippedSW.h:88): a string of that many bytes, NUL included, scores -1.0f */

struct InvCheckPlan {
	int32_t status;        /* CVX_CHECK_* */
	int32_t mid_read;      /* the read part is qry[mid_read - 50 .. mid_read + 50) (status SCORED or NO_WINDOW) */
	uint64_t position;     /* first nibble of the window */
	int32_t n_plain;       /* leading characters of the window that are nibbles of the genome; the rest are 'x' */
	int32_t window_chars;  /* strlen of the window; 0 where none is scored or none decodes */
	int32_t buffer_len;    /* DecodeRefSequence's buffer length: inversionLength + 500 (status SCORED) */
};

/* Region (ref_start, ref_stop, read_start, read_stop) of a tile whose read has H characters, whose window starts at P
 * (interval->onRefStart) and whose alignment starts O characters into it (Align::PositionOffset); L = GetConcatRefLen().
 * The midpoints and the length in int arithmetic, as at :1360-1362 (two's complement where the reference would overflow); the
 * window's position in uint64 arithmetic, as at :1179. */
CVX_HOST_DEVICE inline InvCheckPlan inv_check_plan(int32_t ref_start, int32_t ref_stop, int32_t read_start, int32_t read_stop,
		int32_t H, uint64_t P, int32_t O, uint64_t L) {
	InvCheckPlan p = {CVX_CHECK_TOO_SHORT, 0, 0, 0, 0, 0};
	const int32_t mid_ref = (int32_t) ((uint32_t) ref_start + (uint32_t) ref_stop) / 2;
	const int32_t mid_read = (int32_t) ((uint32_t) read_start + (uint32_t) read_stop) / 2;
	const int32_t diff = (int32_t) ((uint32_t) ref_stop - (uint32_t) ref_start);
	const int32_t inv_len = diff < 0 ? (int32_t) (0u - (uint32_t) diff) : diff;
	if (!(inv_len > kInvMinLen)) return p;      /* (INT_MIN stays negative: too short) */
	p.mid_read = mid_read;
	if (!(kInvReadHalf <= mid_read && (int64_t) mid_read + kInvReadHalf < (int64_t) H)) { p.status = CVX_CHECK_NO_READ; return p; }
	if (inv_len > 0x7fffffff - 2 * kInvRefHalf) { p.status = CVX_CHECK_NO_WINDOW; return p; }      /* (no buffer of that length exists) */
	p.position = P + (uint64_t) (int64_t) O + (uint64_t) (int64_t) mid_ref - (uint64_t) kInvRefHalf - (uint64_t) (inv_len / 2);
	const ScoreWinShape s = score_window_shape(p.position, inv_len + 2 * kInvRefHalf, L);
	if (s.failed) { p.status = CVX_CHECK_NO_WINDOW; return p; }
	p.status = CVX_CHECK_SCORED;
	p.buffer_len = inv_len + 2 * kInvRefHalf;
	p.n_plain = s.n_plain;
	p.window_chars = s.ref_chars;
	return p;
}

/* nt_table (src/StrippedSW.cpp:111-116) */
CVX_HOST_DEVICE inline int inv_nt_code(int c) {
	c |= 0x20;
	return (c == 'a' || c == 'u') ? 0 : c == 'c' ? 1 : c == 'g' ? 2 : c == 't' ? 3 : 4;
}

/* StrippedSW::SingleScore on the host, cell by cell: both strings with their NUL, +1 / -1 with zeros for code 4, gap open and
 * extension 255 (the semantics derived in oracle/score_oracle.c and restated in front of cvx_score.hip).  No diagonal argument
 * here: the full recurrence, two rows. */
inline float inv_single_score_host(const uint8_t *ref, size_t ref_chars, const uint8_t *qry, size_t qry_chars) {
	const size_t R = ref_chars + 1, Q = qry_chars + 1;
	if (R >= (size_t) kInvMaxSeqLen || Q >= (size_t) kInvMaxSeqLen) return -1.0f;
	std::vector<int32_t> prev(R, 0), cur(R, 0);
	std::vector<uint8_t> rc(R);
	for (size_t j = 0; j < R; ++j) rc[j] = (uint8_t) inv_nt_code(j < ref_chars ? ref[j] : 0);
	int32_t best = 0;
	for (size_t i = 0; i < Q; ++i) {
		const int qc = inv_nt_code(i < qry_chars ? qry[i] : 0);
		for (size_t j = 0; j < R; ++j) {
			const int s = (qc == 4 || rc[j] == 4) ? 0 : (qc == (int) rc[j] ? 1 : -1);
			int32_t h = (j > 0 ? prev[j - 1] : 0) + s;
			h = std::max(h, prev[j] - 255);
			if (j > 0) h = std::max(h, cur[j - 1] - 255);
			h = std::max(h, 0);
			cur[j] = h;
			best = std::max(best, h);
		}
		prev.swap(cur);
	}
	return (float) best;
}

/* one region on the host: the window through score_window_decode_host (DecodeRefSequence statement by statement), the read part
 * and its reverse complement as the reference builds them, the scorer above */
inline InvCheck inv_check_host(const uint8_t *bin_ref, uint64_t L, const uint8_t *qry, int32_t H, uint64_t P, int32_t O,
		int32_t ref_start, int32_t ref_stop, int32_t read_start, int32_t read_stop) {
	const InvCheckPlan p = inv_check_plan(ref_start, ref_stop, read_start, read_stop, H, P, O, L);
	InvCheck c = {0.0f, 0.0f, p.status, 0};
	if (p.status != CVX_CHECK_SCORED && p.status != CVX_CHECK_NO_WINDOW) return c;
	std::vector<uint8_t> win;
	size_t win_chars = 0;
	if (p.status == CVX_CHECK_SCORED) {
		if (score_window_decode_host(bin_ref, L, p.position, p.buffer_len, win)) win_chars = strlen((const char *) win.data());
	}
	uint8_t fwd[kInvQry], rev[kInvQry];
	memcpy(fwd, qry + (p.mid_read - kInvReadHalf), (size_t) kInvQry);
	for (int k = 0; k < kInvQry; ++k) rev[kInvQry - 1 - k] = score_window_cpl(fwd[k]);      /* cplBase is cpl: A<->T, C<->G, else unchanged */
	c.window_chars = (int32_t) win_chars;
	c.score_fwd = inv_single_score_host(win.data(), win_chars, fwd, (size_t) kInvQry);
	c.score_rev = inv_single_score_host(win.data(), win_chars, rev, (size_t) kInvQry);
	return c;
}

}  // namespace cvx

#endif
