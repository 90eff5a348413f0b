/*
 * cvx_ladder.h -- launch of ladder_next_kernel (cvx_ladder.hip).  Kept apart from cvx_launch.h, whose hash names the
 * fill / search kernel families (Makefile FILL_ID / SEARCH_ID).
 */
#ifndef CVX_LADDER_H
#define CVX_LADDER_H

#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "cvx_align.h"
#include "cvx_types.h"

namespace cvx {

struct LadderNextArgs {
	const ResultRec *res;      /* the finished rung's result records, n_prev of them */
	const int32_t *prev_idx;   /* job tile of each of them; NULL: rung 1, record j is tile j */
	const TileIn *tin0;        /* rung 1's tile records, by job tile: sequence offsets, W, H */
	const cvx_ladder *lad;     /* by job tile */
	int32_t n_prev;
	int32_t m;                 /* the rung that has finished (1-based); the records written are rung m + 1's */
	const WindowDesc *win0;    /* rung 1's window descriptors, by job tile; NULL: the job's rungs run no inversion checks */
	/* out, each with room for n_prev entries: the climbing tiles in the finished rung's order, then empty tiles (H = W = 0)
	 * up to n_prev, so that a plan launch over all n_prev entries reads defined records */
	RowSrc *rsrc;
	TileIn *tin;
	int32_t *head;             /* head[0] = tiles that climb, head[1 + j] = job tile of entry j (j < head[0]) */
	WindowDesc *win;           /* with win0: the window descriptor of entry j's job tile (zeros behind the climbing tiles) */
};
hipError_t launch_ladder_next(const LadderNextArgs &a, hipStream_t st);

}  // namespace cvx

#endif
