/*
 * cvx_qry_stage.h -- launch of stage_segments_kernel (cvx_qry_stage.hip).  Kept apart from cvx_launch.h, whose hash names the
 * fill / search kernel families (Makefile FILL_ID / SEARCH_ID).
 */
#ifndef CVX_QRY_STAGE_H
#define CVX_QRY_STAGE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cvx_segments.h"

namespace cvx {

/* For every chunk of chunks[0 .. n_chunks): its share of string desc[chunk.seg] into seq, [dst_off, dst_off + len) of a string
 * and not a byte more.  reads: the call's read block; seq: aligned to 16 bytes or more. */
hipError_t launch_stage_segments(const uint8_t *reads, const SegDesc *desc, const SegChunk *chunks, int n_chunks, uint8_t *seq, hipStream_t st);

}  // namespace cvx

#endif
