/*
 * cvx_score_wave.hip -- sub-read scoring of pairs whose shorter side fits in one wave's registers: ngmlr's interval check
 * (reference src/AlignmentBuffer.cpp:2515-2548, a read piece under 1 000 bases against a reference span of up to many kb)
 * and its inversion check (:1158-1235, 100 bases against inversionLength + 500).  Same semantics as cvx_score.hip (header
 * comment there, derivation in oracle/score_oracle.c): strings with their NUL, A/C/G/T(U) = 0..3 and anything else 4,
 * +1 / -1 with 0 for code 4, gaps 255 per base, H = max(0, diag + s, up - 255, left - 255), score = max H, -1 when a
 * length (NUL included) is >= 100 000.
 *
 * The recurrence is symmetric in the two strings, so the SHORTER one (S characters, S <= 64 K) lies along the rows and
 * stays in registers while the longer one (L characters) streams past as an anti-diagonal wavefront:
 *   - lane l owns rows lK .. lK + K - 1 (K = 1, 2, 4, 8, 16): their current H and a per-row score table;
 *   - at step t lane l updates column t - l of its K rows, top to bottom;
 *   - what the row below needs from the lane above -- that lane's bottom-row H of this column, and the column's
 *     character -- moves down one lane per step by DPP wave_shr:1; the lane above's previous value is the diagonal of
 *     the lane's top row, kept in a register.  Lane 0 takes row -1 = 0 and feeds the long string's characters, which
 *     arrive 64 at a time (one coalesced byte per lane, fetched a chunk ahead) and leave that register by v_readlane.
 *   - no masks: a column before a lane's start or past the end carries code 4 (score 0), and with s = 0 the recurrence
 *     only ever moves values that already exist (H <= max of the cells it reads), so rows of code 4 below the short
 *     side, columns of code 4 around the long side and the initial zeros never change the maximum.  The loop runs
 *     L + (S - 1) / K steps: until the last lane that owns a real row has seen the last column.
 * Exact int32 arithmetic (every H is in [0, 1025]).  Per cell: v_bfe (score + 1 from the row's table, indexed by the
 * column's code), v_add3 (diag + that - 1), a max of up and left, the -255, a max3 with the zero, and the best-so-far max.  Per step besides: two DPP moves, a v_readlane and two selects on lane 0.
 *
 * One wave per pair, four pairs per workgroup, no LDS, no scratch, no global memory inside the 64-step inner loop.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cvx_score_wave.h"

namespace cvx {

namespace {

__device__ __forceinline__ int wave_code(int c) {
	c |= 0x20;                       /* case-insensitive; U/u map to 0 like A (src/StrippedSW.cpp:111-116) */
	return (c == 'a' || c == 'u') ? 0 : c == 'c' ? 1 : c == 'g' ? 2 : c == 't' ? 3 : 4;
}

/* lane i <- lane i - 1 (DPP wave_shr:1, GFX9 DPP_WF_SR1 = 0x138); lane 0 gets 0 */
__device__ __forceinline__ int shr1(int v) {
	return __builtin_amdgcn_update_dpp(0, v, 0x138, 0xf, 0xf, true);
}

}  // namespace

template <int K>
__global__ void __launch_bounds__(256)
score_wave_kernel(const uint8_t *seq, const ScorePair *pairs, float *out, int n) {
	const int lane = threadIdx.x & 63;
	const int p = blockIdx.x * 4 + (threadIdx.x >> 6);
	if (p >= n) return;                                  /* wave-uniform */
	const ScorePair pr = pairs[p];
	/* the pair is the wave's: its lengths and offsets in SGPRs, so that the step loop is counted on the scalar unit */
	const int R = __builtin_amdgcn_readfirstlane(pr.ref_len), Q = __builtin_amdgcn_readfirstlane(pr.qry_len);
	if (R >= 100000 || Q >= 100000) {                    /* maxSeqLen, src/StrippedSW.h:88 */
		if (lane == 0) out[p] = -1.0f;
		return;
	}
	const bool qry_short = Q <= R;
	const uint64_t off_s = qry_short ? pr.qry_off : pr.ref_off, off_l = qry_short ? pr.ref_off : pr.qry_off;
	const uint8_t *sh = seq + (((uint64_t) (uint32_t) __builtin_amdgcn_readfirstlane((int) (off_s >> 32)) << 32) | (uint32_t) __builtin_amdgcn_readfirstlane((int) off_s));
	const uint8_t *lg = seq + (((uint64_t) (uint32_t) __builtin_amdgcn_readfirstlane((int) (off_l >> 32)) << 32) | (uint32_t) __builtin_amdgcn_readfirstlane((int) off_l));
	const int S = qry_short ? Q : R;                     /* <= 64 K (host), >= 1 (the NUL) */
	const int L = qry_short ? R : Q;

	/* per row: 2-bit fields (score + 1) indexed by 2 * column code -- bits 2c..2c+1 for c = 0..4 */
	uint32_t tbl[K];
	int h[K];
#pragma unroll
	for (int k = 0; k < K; ++k) {
		const int r = lane * K + k;
		const int c = r < S ? wave_code(sh[r]) : 4;
		tbl[k] = c == 4 ? 0x155u : (0x100u | (2u << (2 * c)));
		h[k] = 0;
	}
	const int steps = L + (S - 1) / K;
	int top_prev = 0;        /* H[lK - 1][column - 1]: the diagonal of the lane's top row */
	int send_h = 0;          /* H[lK + K - 1][column]: handed to the lane below */
	int send_c = 8;          /* 2 * code of the lane's column: handed to the lane below */
	int best = 0;
	int next = lane < L ? 2 * wave_code(lg[lane]) : 8;
	for (int base = 0; base < steps; base += 64) {
		const int chunk = next;                          /* lane j: 2 * code of column base + j (8 past the end) */
		const int j = base + 64 + lane;
		next = j < L ? 2 * wave_code(lg[j]) : 8;
		const int m = min(64, steps - base);
		for (int s = 0; s < m; ++s) {
			const int feed = __builtin_amdgcn_readlane(chunk, s);
			int up = shr1(send_h);
			int cs = shr1(send_c);
			if (lane == 0) { up = 0; cs = feed; }
			int dg = top_prev;
			top_prev = up;
#pragma unroll
			for (int k = 0; k < K; ++k) {
				const int t = (int) ((tbl[k] >> cs) & 3u);   /* s + 1 */
				const int left = h[k];
				const int v = max(max(dg + t - 1, max(up, left) - 255), 0);
				dg = left;
				up = v;
				h[k] = v;
				best = max(best, v);
			}
			send_h = h[K - 1];
			send_c = cs;
		}
	}
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1) best = max(best, __shfl_xor(best, d, 64));
	if (lane == 0) out[p] = (float) best;
}

hipError_t launch_score_wave(const uint8_t *seq, const ScorePair *pairs, float *out, int n, int rows, hipStream_t st) {
	if (n <= 0) return hipSuccess;
	const dim3 grid((n + 3) / 4), block(256);
	switch (rows) {
	case 1: hipLaunchKernelGGL(score_wave_kernel<1>, grid, block, 0, st, seq, pairs, out, n); break;
	case 2: hipLaunchKernelGGL(score_wave_kernel<2>, grid, block, 0, st, seq, pairs, out, n); break;
	case 4: hipLaunchKernelGGL(score_wave_kernel<4>, grid, block, 0, st, seq, pairs, out, n); break;
	case 8: hipLaunchKernelGGL(score_wave_kernel<8>, grid, block, 0, st, seq, pairs, out, n); break;
	case 16: hipLaunchKernelGGL(score_wave_kernel<16>, grid, block, 0, st, seq, pairs, out, n); break;
	default: return hipErrorInvalidValue;
	}
	return hipGetLastError();
}

}  // namespace cvx
