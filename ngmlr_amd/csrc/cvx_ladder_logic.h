/*
 * cvx_ladder_logic.h -- the corridor retry ladder of AlignmentBuffer::computeAlignment (reference
 * src/AlignmentBuffer.cpp:259-425) as plain functions compiled for the device and for the host, free of HIP calls, so that
 * ladder_next_kernel (cvx_ladder.hip), cvx_ladder_rung (cvx_corridor.cpp), cvx_submit_ladder (cvx_rt_ladder.cpp) and the CPU suite
 * (tests/test_ladder_logic_cpu.py, through cvx_ladder_rung) run one rule.
 *
 * An attempt that is not valid rebuilds the corridor at multiplier 2, 3, ... and aligns again:
 *   rung m exists while  min(corridor, 2 * refSeqLen) * m <= 2 * refSeqLen  and fewer than 5 attempts have run (:259-266, :292-294;
 *   fullAlignment: 1 attempt);
 *   refSeqLen is computeAlignment's: onRefStop - onRefStart + 1 (:209), the decoded string's length PLUS ONE -- a tile's ref_len
 *   is that string's length (strlen(refSeq), what the builders' k is computed from, :112, :135), so refSeqLen = ref_len + 1 in
 *   the cap and in getCorridorFull's argument (:310).  The recordings of the unmodified reference pin this
 *   (tests/golden/ladder_*.npz);
 *   its corridor is what the reference's builder writes at multiplier m, as the closed form the device evaluates (RowSrc):
 *     FULL                          getCorridorFull(refSeqLen = ref_len + 1)   :101-102  constant rows
 *     SHORT                         getCorridorLinear(corridor * m)            :78-79    k = 1, d = width / 2 (integer)
 *     ANCHORS && !REALIGN && m < 3  getCorridorEndpointsWithAnchors(m)         :184-191  left * m, right * m, width = (int) (left' + right')
 *     otherwise                     getCorridorEndpoints(corridor * m, realign) :110-123  width = corridor * m / (realign ? 1 : 4)
 * in the reference's own types: int arithmetic where it has ints, binary32 operations each rounded on its own (the host
 * files are compiled with -ffp-contract=off; the device takes __fmul_rn / __fadd_rn / __fdiv_rn), the (int) conversions C
 * truncation, getCorridorFull's 20 % in double.
 *
 * A tile whose slope k = qry_len * 1.0f / ref_len is not a positive finite number (an empty read or an empty window, which the
 * reference never aligns) has no affine form the device accepts; it gets constant rows (offset 0) of the rule's width -- the
 * tile is CVX_TILE_EMPTY whatever its rows say.
 */
#ifndef CVX_LADDER_LOGIC_H
#define CVX_LADDER_LOGIC_H

#include <stdint.h>

#include "cvx_align.h"
#include "cvx_types.h"

#if defined(__HIPCC__)
#define CVX_LHD __host__ __device__ inline
#else
#define CVX_LHD inline
#endif

namespace cvx {

static const int kLadderMaxRungs = 5;      /* retryCount (:259) */
static const int32_t kLadderFlags = CVX_LADDER_ANCHORS | CVX_LADDER_REALIGN | CVX_LADDER_SHORT | CVX_LADDER_FULL;

/* binary32 operations that round once, wherever they are compiled */
CVX_LHD float ladder_mul(const float a, const float b) {
#if defined(__HIP_DEVICE_COMPILE__)
	return __fmul_rn(a, b);
#else
	return a * b;
#endif
}
CVX_LHD float ladder_add(const float a, const float b) {
#if defined(__HIP_DEVICE_COMPILE__)
	return __fadd_rn(a, b);
#else
	return a + b;
#endif
}
CVX_LHD float ladder_div(const float a, const float b) {
#if defined(__HIP_DEVICE_COMPILE__)
	return __fdiv_rn(a, b);
#else
	return a / b;
#endif
}

/* arguments for which every int and every float -> int conversion below is defined: what cvx_ladder_rung and cvx_submit_ladder
 * accept (the kernel sees checked records only) */
CVX_LHD bool ladder_args_ok(const cvx_ladder &l, const int32_t ref_len, const int32_t qry_len) {
	if (l.corridor < 0 || (l.flags & ~kLadderFlags) != 0 || ref_len < 0 || ref_len > (1 << 29) || qry_len < 0) return false;
	if (l.flags & CVX_LADDER_ANCHORS) {
		if (!(l.left >= 0.0f && l.left <= 1.0e8f) || !(l.right >= 0.0f && l.right <= 1.0e8f)) return false;      /* (also refuses NaN) */
	}
	return true;
}

/* attempts computeAlignment allows the tile at most */
CVX_LHD int ladder_attempts(const int32_t flags) { return (flags & CVX_LADDER_FULL) ? 1 : kLadderMaxRungs; }

/* maxCorridorSize = refSeqLen * 2 (:265) with refSeqLen = ref_len + 1 (see the head of this file); 64 bits: it need not fit an int here */
CVX_LHD int64_t ladder_cap(const int32_t ref_len) { return 2 * ((int64_t) ref_len + 1); }

/* corridor = std::min(corridor, maxCorridorSize) (:266) */
CVX_LHD int64_t ladder_corridor(const int32_t corridor, const int32_t ref_len) {
	const int64_t cap = ladder_cap(ref_len);
	return (int64_t) corridor < cap ? (int64_t) corridor : cap;
}

/* does rung m (1-based) exist? */
CVX_LHD bool ladder_rung_exists(const int32_t corridor, const int32_t flags, const int32_t ref_len, const int32_t m) {
	if (m < 1 || m > ladder_attempts(flags)) return false;
	return ladder_corridor(corridor, ref_len) * (int64_t) m <= ladder_cap(ref_len);
}

/* rungs the tile can climb at most: the largest m that exists (they exist from 1 up to it) */
CVX_LHD int ladder_length(const int32_t corridor, const int32_t flags, const int32_t ref_len) {
	int m = 0;
	while (ladder_rung_exists(corridor, flags, ref_len, m + 1)) ++m;
	return m;
}

/* The corridor of rung m as the record the kernels read (RowSrc: fmt, width, off0, k, d, right; src_off unused).  The caller has
 * checked that the rung exists and that the arguments are in range (ladder_args_ok: every int below then fits). */
CVX_LHD void ladder_form(const int32_t corridor, const float left, const float right, const int32_t flags, const int32_t ref_len,
		const int32_t qry_len, const int32_t m, RowSrc &f) {
	f.src_off = 0; f.off0 = 0; f.width = 0; f.fmt = kRowsAffine;
	f.k = 0.0f; f.d = 0.0f; f.right = 0.0f;
	if (flags & CVX_LADDER_FULL) {
		f.fmt = kRowsConst;
		const int32_t w = ref_len + 1;      /* refSeqLen */
		f.off0 = (int32_t) ((double) w * -0.2);
		f.width = w + (int32_t) ((double) w * 0.2);
		return;
	}
	const int32_t cm = (int32_t) (ladder_corridor(corridor, ref_len) * (int64_t) m);      /* corridor * corridorMultiplier */
	if (flags & CVX_LADDER_SHORT) {
		f.width = cm;
		f.k = 1.0f;
		f.d = (float) (cm / 2);
		return;
	}
	f.k = ladder_div(ladder_mul((float) qry_len, 1.0f), (float) ref_len);
	if ((flags & CVX_LADDER_ANCHORS) && !(flags & CVX_LADDER_REALIGN) && m < 3) {
		const float l = ladder_mul(left, (float) m);
		const float r = ladder_mul(right, (float) m);
		f.width = (int32_t) ladder_add(l, r);
		f.right = r;
	} else {
		f.width = cm / ((flags & CVX_LADDER_REALIGN) ? 1 : 4);
		f.d = ladder_div((float) f.width, 2.0f);
	}
	if (!(f.k > 0.0f && f.k < 3.0e38f)) {      /* no slope: constant rows, see the head of this file */
		f.fmt = kRowsConst;
		f.k = 0.0f; f.d = 0.0f; f.right = 0.0f;
	}
}

/* what a rung's status means for the tile: 0 resolved (or stopped: CVX_TILE_UNSUPPORTED stays loud), 1 the reference's -1 */
CVX_LHD bool ladder_status_climbs(const int32_t status) { return status != CVX_TILE_OK && status != CVX_TILE_UNSUPPORTED; }

/* does the tile go on to rung m + 1 after rung m ended with `status`? */
CVX_LHD bool ladder_climbs(const int32_t corridor, const int32_t flags, const int32_t ref_len, const int32_t m, const int32_t status) {
	return ladder_status_climbs(status) && ladder_rung_exists(corridor, flags, ref_len, m + 1);
}

}  // namespace cvx

#endif
