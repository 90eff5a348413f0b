/*
 * cvx_inv_checks.hip -- the inversion checks of a job's low-identity regions scored on the device (gfx950): per region what
 * AlignmentBuffer::checkForSV (reference src/AlignmentBuffer.cpp:1158-1235) computes before it decides -- the window of the
 * genome around the region's midpoint against the 100 read bases around the midpoint on the read, and against their reverse
 * complement, both with StrippedSW::SingleScore.  The rule (outcomes, positions, the window's shape) is inv_check_plan in
 * cvx_inv_checks.h; this file adds the scores.
 *
 * The query is 100 bases, so no DP row is kept: a gap costs 255 and the shorter string has 101 bytes, hence (the argument in
 * front of score_diag_kernel, cvx_score.hip: min(Q, R) <= 511) no gapped path beats the best ungapped one, for a window of any
 * length -- the score is the maximum over all diagonals of the best contiguous run, h = max(0, h + s).  Every lane walks its
 * own diagonal.  A character outside the window, the NUL behind either string, an 'x' and an N all have code 4, which scores 0
 * against everything: h keeps its value and the maximum does not move, so the kernel treats all of them alike and only the
 * window's n_plain leading characters -- nibbles of the genome -- are ever looked up.
 *
 * The window never exists as a string: a chunk of it is decoded from the resident 4-bit genome straight into LDS as codes,
 * kInvDiags diagonals at a time with the kInvQry - 1 columns more that their last rows reach, so consecutive chunks overlap
 * by the query's length and the window's own length bounds nothing but the number of chunks.  The 100 query codes of both strands
 * sit in LDS for the whole region, and both strands are scored in the same pass over a chunk.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cvx_inv_checks_dev.h"

namespace cvx {

namespace {

const int kInvDiags = 2048;                  /* diagonals of one chunk: 32 trips of the wave */
const int kInvLead = 128;                    /* the first chunk starts at diagonal -kInvLead: the diagonals -(kInvQry - 1) .. -1 start left of the window */
const int kInvCols = kInvDiags + 128;        /* window columns of one chunk in LDS: a diagonal's last row lies kInvQry - 1 columns right of its first */
static_assert(kInvLead >= kInvQry - 1 && kInvCols >= kInvDiags + kInvQry - 1 && kInvDiags % 64 == 0, "chunk geometry");

/* nibble of the genome -> nt_table code of the character dec4 gives it: A T G C N -> 0 3 2 1 4, '?' -> 4 */
__device__ __forceinline__ int nibble_code(const unsigned v) {
	return v == 0u ? 0 : v == 1u ? 3 : v == 2u ? 2 : v == 3u ? 1 : 4;
}

}  // namespace

__global__ void __launch_bounds__(256)
inv_checks_kernel(const InvCheckArgs a) {
	__shared__ uint8_t s_r[4][kInvCols];
	__shared__ uint16_t s_q[4][128];         /* row i: forward code | reverse-complement code << 8 */
	__shared__ int s_chunks[4];
	/* one WAVE per region, four regions per workgroup, as the neighbouring kernels do it; the region is wave-uniform */
	const int lane = (int) (threadIdx.x & 63u), w = (int) (threadIdx.x >> 6);
	const unsigned long long r = (unsigned long long) blockIdx.x * 4ull + (unsigned long long) w;
	unsigned long long total = a.off[a.n_tiles];
	if (total > a.cap) total = a.cap;
	const bool live = r < total;
	InvCheckPlan p = {CVX_CHECK_TOO_SHORT, 0, 0, 0, 0, 0};
	int n_chunks = 0;
	bool too_long = false;
	if (live) {
		/* the region's tile: the last one whose first region is not behind r (off[0] = 0, tiles without regions repeat an offset) */
		int lo = 0, hi = a.n_tiles - 1;
		while (lo < hi) {
			const int mid = (lo + hi + 1) >> 1;
			if (a.off[mid] <= r) lo = mid; else hi = mid - 1;
		}
		const NmRegion g = a.regions[r];
		const TileIn ti = a.tin[lo];
		p = inv_check_plan(g.ref_start, g.ref_stop, g.read_start, g.read_stop, ti.H, a.win[lo].position, a.rec[lo].ref_position, a.L);
		if (p.status == CVX_CHECK_SCORED) {
			too_long = p.window_chars + 1 >= kInvMaxSeqLen;
			if (!too_long && p.n_plain > 0) n_chunks = (p.n_plain + kInvLead + kInvDiags - 1) / kInvDiags;
		}
		if (n_chunks > 0) {
			/* the read part is inside the tile's query: 50 <= mid_read and mid_read + 50 < H */
			const uint8_t *q = a.seq + ti.qry_off + (unsigned) (p.mid_read - kInvReadHalf);
			for (int k = lane; k < kInvQry; k += 64) {
				const int cf = q[k], cr = q[kInvQry - 1 - k];
				int rv = inv_nt_code(cr);
				if (cr == 'A' || cr == 'C' || cr == 'G' || cr == 'T') rv = 3 - rv;      /* cplBase: the four upper-case letters, nothing else */
				s_q[w][k] = (uint16_t) (inv_nt_code(cf) | (rv << 8));
			}
		}
	}
	if (lane == 0) s_chunks[w] = n_chunks;
	__syncthreads();
	const int max_chunks = max(max(s_chunks[0], s_chunks[1]), max(s_chunks[2], s_chunks[3]));      /* (uniform over the workgroup: its barriers) */
	int best_f = 0, best_r = 0;
	for (int c = 0; c < max_chunks; ++c) {
		const int d0 = c * kInvDiags - kInvLead;     /* first diagonal of the chunk = the window column s_r[w][0] stands for */
		if (c > 0) __syncthreads();                  /* the previous chunk has been read */
		if (c < n_chunks) {
			for (int x = lane; x < kInvCols; x += 64) {
				const int col = d0 + x;
				int code = 4;
				if (col >= 0 && col < p.n_plain) {
					const unsigned long long at = p.position + (unsigned long long) col;      /* <= L: a nibble of the genome (cvx_score_stage.hip) */
					const unsigned b = a.bin[at >> 1];
					code = nibble_code((at & 1ull) ? (b & 0xFu) : (b >> 4));
				}
				s_r[w][x] = (uint8_t) code;
			}
		}
		__syncthreads();
		if (c < n_chunks) {
			for (int b0 = 0; b0 < kInvDiags && d0 + b0 < p.n_plain; b0 += 64) {
				const uint8_t *rp = &s_r[w][b0 + lane];      /* this lane's diagonal d0 + b0 + lane: row i meets column rp[i] */
				int hf = 0, hr = 0;
#pragma unroll 4
				for (int i = 0; i < kInvQry; ++i) {
					const int q = s_q[w][i];
					const int qf = q & 0xFF, qr = q >> 8;
					const int rc = rp[i];
					const int sf = (qf == 4 || rc == 4) ? 0 : (qf == rc ? 1 : -1);
					const int sr = (qr == 4 || rc == 4) ? 0 : (qr == rc ? 1 : -1);
					hf = max(hf + sf, 0);
					hr = max(hr + sr, 0);
					best_f = max(best_f, hf);
					best_r = max(best_r, hr);
				}
			}
		}
	}
	if (!live) return;
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1) {
		best_f = max(best_f, __shfl_xor(best_f, d, 64));
		best_r = max(best_r, __shfl_xor(best_r, d, 64));
	}
	if (lane == 0) {
		InvCheck out;
		out.score_fwd = too_long ? -1.0f : (float) best_f;
		out.score_rev = too_long ? -1.0f : (float) best_r;
		out.status = p.status;
		out.window_chars = p.status == CVX_CHECK_SCORED ? p.window_chars : 0;
		a.checks[r] = out;
	}
}

hipError_t launch_inv_checks(const InvCheckArgs &a, unsigned long long max_regions, hipStream_t st) {
	if (max_regions == 0 || a.n_tiles <= 0) return hipSuccess;
	hipLaunchKernelGGL(inv_checks_kernel, dim3((unsigned) ((max_regions + 3) / 4)), dim3(256), 0, st, a);
	return hipGetLastError();
}

}  // namespace cvx
