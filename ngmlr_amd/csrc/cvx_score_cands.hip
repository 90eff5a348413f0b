/*
 * cvx_score_cands.hip -- the scoring call of a batch planned on the device (gfx950): from the candidate search's dense list to
 * one ScoreWinDesc per candidate, so that stage_score_windows_kernel and score_diag_kernel can run behind the search without the
 * lists visiting the host (cvx_search_score_arena).  The device counterpart of score_windows_plan (cvx_score_windows.h) for the
 * one shape ngmlr's CS feed has: every window with the same buffer_len, every pair in the diagonal class, which is what lets
 * every candidate own a slot of fixed size instead of an offset that depends on the candidates in front of it.
 *
 * One thread per candidate.  The candidate's read is the last one whose list begins at or in front of it (reads without a list
 * share their begin with the next read that has one and lie in front of it), found by binary search over begin[]: those
 * ceil(log2(n_reads + 1)) loads are the only dependent chain; begin[] of a call is a few KB and stays in cache.  No LDS.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cvx_score_cands.h"

namespace cvx {

__global__ void __launch_bounds__(256)
plan_candidate_windows_kernel(const SearchCandidate * __restrict__ cand, const uint64_t * __restrict__ begin, const int32_t * __restrict__ n_cand,
		const uint64_t * __restrict__ read_off, const int32_t * __restrict__ read_len, int n_reads, uint64_t need, uint64_t L,
		int32_t buffer_len, int32_t window_lead, int32_t max_cmrs, CandWinSlots slots,
		ScoreWinDesc * __restrict__ desc, int32_t * __restrict__ status) {
	const uint64_t q = (uint64_t) blockIdx.x * 256u + threadIdx.x;
	if (q >= need) return;
	/* begin[lo] <= q < begin[hi] throughout: begin[0] = 0, begin[n_reads] = need */
	int lo = 0, hi = n_reads;
	while (hi - lo > 1) {
		const int mid = (int) (((unsigned) lo + (unsigned) hi) >> 1);
		if (begin[mid] <= q) lo = mid; else hi = mid;
	}
	const int i = lo;
	const SearchCandidate c = cand[q];
	ScoreWinDesc d;
	/* loc.m_Location - (corridor >> 1), src/ScoreBuffer.cpp:111: unsigned, a location inside the lead wraps to the far end */
	d.position = c.location - (uint64_t) (int64_t) window_lead;
	const ScoreWinShape s = score_window_shape(d.position, buffer_len, L);
	const int32_t st = n_cand[i] >= max_cmrs ? (int32_t) kCandListDropped : s.failed ? (int32_t) kCandNoWindow : (int32_t) kCandScored;
	const bool scored = st == kCandScored;
	/* a candidate that is not scored keeps its slot and gets two empty strings: the kernels behind run over all slots alike */
	d.n_plain = scored ? s.n_plain : 0;
	d.ref_chars = scored ? s.ref_chars : 0;
	d.read_off = read_off[i];
	d.read_len = scored ? read_len[i] : 0;
	d.reverse = c.reverse != 0;
	d.ref_off = q * slots.stride_ref;
	d.qry_off = slots.base_qry + q * slots.stride_qry;
	d.scratch_off = 0;
	desc[q] = d;
	status[q] = st;
}

hipError_t launch_plan_candidate_windows(const SearchCandidate *cand, const uint64_t *begin, const int32_t *n_cand, const uint64_t *read_off,
		const int32_t *read_len, int n_reads, uint64_t need, uint64_t L, int32_t buffer_len, int32_t window_lead, int32_t max_cmrs,
		CandWinSlots slots, ScoreWinDesc *desc, int32_t *status, hipStream_t st) {
	if (need == 0 || n_reads <= 0) return hipSuccess;
	hipLaunchKernelGGL(plan_candidate_windows_kernel, dim3((unsigned) ((need + 255) / 256)), dim3(256), 0, st, cand, begin, n_cand, read_off, read_len,
			n_reads, need, L, buffer_len, window_lead, max_cmrs, slots, desc, status);
	return hipGetLastError();
}

}  // namespace cvx
