/*
 * cvx_score_stage.h -- launch of stage_score_windows_kernel (cvx_score_stage.hip).  Kept apart from cvx_launch.h, whose hash
 * names the fill / search kernel families (Makefile FILL_ID / SEARCH_ID).
 */
#ifndef CVX_SCORE_STAGE_H
#define CVX_SCORE_STAGE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cvx_launch.h"
#include "cvx_score_windows.h"

namespace cvx {

/* For every slot of desc[0 .. n): the window and its NUL, the query and its NUL into seq at the slot's offsets, and pairs[slot]
 * for the scoring kernels.  bin: the resident genome (cvx_genome_upload: at least 64 bytes of allocation behind its last byte);
 * reads: the call's read block. */
hipError_t launch_stage_score_windows(const uint8_t *bin, const uint8_t *reads, const ScoreWinDesc *desc, int n,
		uint8_t *seq, ScorePair *pairs, hipStream_t st);

}  // namespace cvx

#endif
