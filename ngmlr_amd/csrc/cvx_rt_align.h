/*
 * cvx_rt_align.h -- what the alignment job pipeline (cvx_rt_align.cpp) and the ladder jobs (cvx_rt_ladder.cpp) call of each
 * other: stage_compute queues the next rung inline and pump advances the climbers; a rung is a batch from the pipeline's pool
 * that goes through its compute, results and ops stages.  Everything else of the two files stays in their anonymous namespaces.
 * Internal, like cvx_rt.h.
 */
#ifndef CVX_RT_ALIGN_H
#define CVX_RT_ALIGN_H

#include "cvx_rt.h"

/* the queries of a job of cvx_submit_segments: the call's read block and one segment per tile (cvx_segments.h) */
struct SegmentsIn {
	int32_t n_reads;
	const uint8_t *arena;
	const uint64_t *offsets;
	const cvx_read_segment *qry;
};

/* ---- cvx_rt_align.cpp */
cvx_batch_s *acquire_batch(cvx_context *h);
void recycle_batch(cvx_context *h, cvx_batch_s *b);
int fail_job(cvx_batch_s *b, int rc);
int stage_compute(cvx_context *h, cvx_batch_s *b, bool streaming = false);
int stage_results(cvx_context *h, cvx_batch_s *b);
int stage_ops(cvx_context *h, cvx_batch_s *b);
int submit_common(cvx_handle h, int32_t n, const cvx_tile *tiles, const cvx_genome_s *genome, const uint64_t *ref_position, cvx_job *out,
		const SegmentsIn *segs = nullptr, const cvx_ladder *ladders = nullptr, int max_rungs = 0);

/* ---- cvx_rt_ladder.cpp (ladder_drop: cvx_rt.h, for the batch's destructor) */
void ladder_release(cvx_context *h, cvx_batch_s *root);
int ladder_queue_next(cvx_context *h, cvx_batch_s *root, cvx_batch_s *prev, int m, bool inline_);
void ladder_advance(cvx_context *h, cvx_batch_s *root, bool block);
void ladder_pump(cvx_context *h);
int ladder_finish(cvx_context *h, cvx_batch_s *root);

#endif
