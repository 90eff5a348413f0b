/*
 * cvx_score_cands.h -- launch of plan_candidate_windows_kernel (cvx_score_cands.hip) and the slot layout of a fused call
 * (cvx_search_score_arena): the sequence arena as need fixed-size window slots followed by need fixed-size query slots.  Kept
 * apart from cvx_launch.h for the reason cvx_score_stage.h is.
 */
#ifndef CVX_SCORE_CANDS_H
#define CVX_SCORE_CANDS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cvx_launch.h"
#include "cvx_score_windows.h"

namespace cvx {

/* status[q] of a candidate, in the order they are decided */
enum { kCandScored = 0, kCandNoWindow = 1 /* DecodeRefSequence returns false */, kCandListDropped = 2 /* n_cand >= max_cmrs: no AllocScores, src/CS.cpp:264-266 */ };

/* Where candidate q's strings lie in the sequence arena.  Every window of a call has the same buffer_len, so a slot of
 * align16(buffer_len + 1) bytes holds any of them with its NUL (ref_chars <= buffer_len: the odd position's leading character,
 * len + 1 from the genome, `end` behind it); a query slot holds the longest read of the call with its NUL.  Slots begin on 16
 * bytes, which is stage_score_windows_kernel's whole-piece path. */
struct CandWinSlots {
	uint64_t stride_ref, stride_qry, base_qry, seq_bytes;
};
inline uint64_t cand_windows_align16(uint64_t x) { return (x + 15ull) & ~15ull; }
inline CandWinSlots cand_windows_slots(int32_t buffer_len, uint64_t max_read_bytes /* NUL included */, uint64_t need) {
	CandWinSlots s;
	s.stride_ref = cand_windows_align16((uint64_t) buffer_len + 1);
	s.stride_qry = cand_windows_align16(max_read_bytes);
	s.base_qry = need * s.stride_ref;
	s.seq_bytes = need * (s.stride_ref + s.stride_qry);
	return s;
}

/* One ScoreWinDesc and one status per entry of the search's dense candidate list cand[0 .. need): begin has n_reads + 1 entries
 * (begin[n_reads] = need), n_cand may be negative (a read the ladder gave up on: no entries); read_off / read_len are the search's
 * own read block; L = score_windows_concat_len(n_nibbles). */
hipError_t launch_plan_candidate_windows(const SearchCandidate *cand, const uint64_t *begin, const int32_t *n_cand, const uint64_t *read_off,
		const int32_t *read_len, int n_reads, uint64_t need, uint64_t L, int32_t buffer_len, int32_t window_lead, int32_t max_cmrs,
		CandWinSlots slots, ScoreWinDesc *desc, int32_t *status, hipStream_t st);

}  // namespace cvx

#endif
