/*
 * cvx_job_text.h -- the device text stage of a job that brings its CIGAR / MD strings back with its results (a CVX_CREATE_JOB_TEXT
 * handle; text_kernel<false>, text_scan_kernel and text_bounded_kernel in cvx_text.hip).  Kept apart from cvx_types.h /
 * cvx_launch.h, whose bytes name the fill / search kernel families (Makefile FILL_ID / SEARCH_ID).
 */
#ifndef CVX_JOB_TEXT_H
#define CVX_JOB_TEXT_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cvx_launch.h"
#include "cvx_job_text_logic.h"

namespace cvx {

/* pass 1 over all a.n_tiles tiles of the job, external clips zero (a.ext_qstart / a.ext_qend are not read): fields and lengths ->
 * a.recs, a.text_len; the exclusive prefix sum of the lengths -> a.text_off with the total behind it (a.text_total[0]) */
hipError_t launch_job_text_size(const TextArgs &a, hipStream_t st);
/* pass 2 into an arena of `cap` bytes (a.text) sized before the total was known: a tile whose whole text [off, off + len) lies
 * below cap writes it (the two NULs of a tile without an alignment included), any other tile writes nothing; a.text_total[0]
 * (the scan's) says how many bytes there are, a.text_total[1] receives cap */
hipError_t launch_job_text_bounded(const TextArgs &a, unsigned long long cap, hipStream_t st);

}  // namespace cvx

#endif
