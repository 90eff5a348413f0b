/*
 * cvx_ladder.hip -- the step between two rungs of a ladder job (gfx950; cvx_submit_ladder, include/cvx_align.h): behind a
 * rung's result records, on the job's stream, ladder_next_kernel reads every live tile's status, decides with the shared
 * rule (cvx_ladder_logic.h: the retry loop of AlignmentBuffer::computeAlignment, reference src/AlignmentBuffer.cpp:259-425)
 * and writes the next rung's corridor and tile records, compacted in the finished rung's order, with the list of the job
 * tiles they belong to and their count.  A climbing tile keeps the sequence offsets of rung 1: nothing of its sequences moves.
 * A job submitted with a genome on a handle that scores inversion checks also gets every climbing tile's window descriptor
 * gathered beside its tile record (inv_checks_kernel indexes them by the rung's own tile index); no window is decoded again.
 *
 * One workgroup for the whole rung: the list is an ordered compaction of a few thousand 4-byte decisions, a block scan per
 * 256 tiles, microseconds beside the fills on either side of it.  The kernel neither waits nor polls: the rung it reads is
 * final by stream order.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cvx_ladder.h"
#include "cvx_ladder_logic.h"

namespace cvx {

static const int kLadderBlock = 256;

__global__ void __launch_bounds__(kLadderBlock)
ladder_next_kernel(const LadderNextArgs a) {
	__shared__ int32_t s_scan[kLadderBlock];
	__shared__ int32_t s_base;
	const int tid = (int) threadIdx.x;
	if (tid == 0) s_base = 0;
	__syncthreads();
	for (int j0 = 0; j0 < a.n_prev; j0 += kLadderBlock) {
		const int j = j0 + tid;
		int32_t tile = -1, climbs = 0;
		cvx_ladder l;
		TileIn ti;
		if (j < a.n_prev) {
			tile = a.prev_idx ? a.prev_idx[j] : j;
			l = a.lad[tile];
			ti = a.tin0[tile];
			climbs = ladder_climbs(l.corridor, l.flags, ti.W, a.m, a.res[j].status) ? 1 : 0;
		}
		/* inclusive scan of the block's decisions (Hillis-Steele over LDS: 8 rounds) */
		s_scan[tid] = climbs;
		__syncthreads();
		for (int d = 1; d < kLadderBlock; d <<= 1) {
			const int32_t add = tid >= d ? s_scan[tid - d] : 0;
			__syncthreads();
			s_scan[tid] += add;
			__syncthreads();
		}
		const int32_t base = s_base;
		if (climbs) {
			const int32_t at = base + s_scan[tid] - 1;      /* < n_prev: one entry per climbing tile of the n_prev read */
			RowSrc f;
			ladder_form(l.corridor, l.left, l.right, l.flags, ti.W, ti.H, a.m + 1, f);
			a.rsrc[at] = f;
			ti.row_off = 0;      /* closed forms own no rows */
			ti.reserved = 0;
			a.tin[at] = ti;
			a.head[1 + at] = tile;
			if (a.win0) a.win[at] = a.win0[tile];      /* the tile's window descriptor, for the rung's inversion checks */
		}
		__syncthreads();
		if (tid == kLadderBlock - 1) s_base = base + s_scan[tid];
		__syncthreads();
	}
	const int32_t count = s_base;
	if (tid == 0) a.head[0] = count;
	for (int at = count + tid; at < a.n_prev; at += kLadderBlock) {
		RowSrc f;
		f.src_off = 0; f.off0 = 0; f.width = 0; f.fmt = kRowsConst;
		f.k = 0.0f; f.d = 0.0f; f.right = 0.0f;
		TileIn ti;
		ti.ref_off = 0; ti.qry_off = 0; ti.W = 0; ti.H = 0; ti.row_off = 0; ti.reserved = 0;
		a.rsrc[at] = f;
		a.tin[at] = ti;
		a.head[1 + at] = -1;
		if (a.win0) {
			WindowDesc w;
			w.position = 0; w.dst_off = 0; w.n_chars = 0;
			a.win[at] = w;
		}
	}
}

hipError_t launch_ladder_next(const LadderNextArgs &a, hipStream_t st) {
	if (a.n_prev <= 0) return hipSuccess;
	hipLaunchKernelGGL(ladder_next_kernel, dim3(1), dim3(kLadderBlock), 0, st, a);
	return hipGetLastError();
}

}  // namespace cvx
