/*
 * cvx_rt_stages.cpp -- the result stages a handle runs with every job (JobRegions with the inversion checks, JobText: cvx_rt.h),
 * over the kernels of cvx_text.hip and cvx_inv_checks.hip: what the pipeline (cvx_rt_align.cpp: stage_compute, stage_results,
 * stage_ops) calls to queue them and bring them back, and the getters that hand their data out (cvx_job_regions, _regions_info,
 * cvx_job_checks, cvx_job_texts, _texts_info) -- for a ladder job, what ladder_merge_stages (cvx_rt_ladder.cpp) merged from the
 * same members of its rungs.  The stages of FINISHED jobs, run on request on the text stream: cvx_rt_text.cpp.
 */
#include <algorithm>
#include <cstring>

#include "cvx_rt.h"

/* regions the dense arena of a job's low-identity regions is first sized for: a 10 kb PacBio tile has four or five */
static const uint64_t kJobRegionsPerTile = 8;

/* the batch's own stream set: behind everything the batch queued */
static hipStream_t rewrite_stream(const cvx_context *h, const cvx_batch_s *b) { return b->s_run ? b->s_run : h->s_main; }

/* A CVX_CREATE_NM_REGIONS handle: the peak finder of detectMisalignment over the batch's op lists (cvx_text.hip), queued on `st`
 * behind the compaction with no host step in between -- count + stage per tile, the offset scan, then the write into an arena
 * sized by an estimate, the way finalize and compact treat the dense ops.  Offsets, total, the capacity the write ran with and
 * the end states travel in the copies queued here, in front of the event stage_results waits for; the regions themselves with
 * the dense ops (fetch).  rewrite: the arena has grown, only the write runs again. */
int JobRegions::queue(cvx_batch_s *b, hipStream_t st, bool rewrite) {
	const int n = b->n;
	const size_t n1 = (size_t) n;
	const TextArgs a = job_text_args(b);
	if (!rewrite) {
		RC_TRY(d_off.ensure(2 * n1 + 8));
		RC_TRY(d_open.ensure(n1));
		RC_TRY(d_stage.ensure(n1 * (size_t) kNmStage));
		RC_TRY(d_reg.ensure((size_t) (kJobRegionsPerTile * n1) + 64));
		RC_TRY(h_off.ensure((n1 + 2) * sizeof(unsigned long long)));
		RC_TRY(h_open.ensure(n1 * sizeof(NmOpen)));
		cap = d_reg.cap;
		rewrites = 0;
	}
	unsigned long long *d_len = d_off.p, *d_o = d_off.p + n1, *d_total = d_o + n1;
	if (!rewrite) HIP_TRY(launch_nm_regions_count(a, 0, n, d_len, d_o, d_total, d_open.p, d_stage.p, st));
	HIP_TRY(launch_nm_regions_bounded(a, n, d_len, d_o, d_total, d_stage.p, d_reg.p, cap, st));
	if (checks_on) {
		/* the checks of whatever the write has just put into the arena, behind it on the same stream: the total is the device's
		 * (d_o[n], right behind the offsets), so the first launch covers the arena; a rewrite knows it and runs over the grown
		 * arena again, all records */
		RC_TRY(d_chk.ensure((size_t) cap));
		InvCheckArgs c;
		memset(&c, 0, sizeof(c));
		c.bin = bin; c.L = L;
		c.seq = b->seq(); c.tin = b->d_tin.p; c.win = b->d_win.p;      /* (a later rung's d_win: gathered by ladder_next_kernel) */
		c.rec = reinterpret_cast<const ResultRec *>(b->d_res.p);
		c.off = d_o; c.regions = d_reg.p; c.checks = d_chk.p;
		c.cap = cap; c.n_tiles = n;
		HIP_TRY(launch_inv_checks(c, rewrite ? std::min<unsigned long long>(total, cap) : cap, st));
	}
	if (!rewrite) {
		HIP_TRY(hipMemcpyAsync(h_off.p, d_o, (n1 + 2) * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
		HIP_TRY(hipMemcpyAsync(h_open.p, d_open.p, n1 * sizeof(NmOpen), hipMemcpyDeviceToHost, st));
	}
	return CVX_OK;
}

/* what cvx_job_regions / cvx_job_texts hand out for an empty job: one offset, 0 */
static int one_zero_offset(PinBuf &h_off) {
	RC_TRY(h_off.ensure(2 * sizeof(unsigned long long)));
	memset(h_off.p, 0, 2 * sizeof(unsigned long long));
	return CVX_OK;
}
int JobRegions::set_empty() { return one_zero_offset(h_off); }
int JobText::set_empty() { return one_zero_offset(h_off); }

int JobRegions::fetch(cvx_context *h, cvx_batch_s *b) {
	if (!on) return CVX_OK;
	if (total > cap) {
		/* as rare as a dense-ops overflow: more regions than eight per tile -- a larger arena, and the write alone runs again (counts,
		 * offsets and the staged regions are still the job's) */
		RC_TRY(d_reg.ensure((size_t) total + 64));
		cap = d_reg.cap;
		rewrites += 1;
		hipStream_t ps = rewrite_stream(h, b);
		RC_TRY(queue(b, ps, true));
		HIP_TRY(hipStreamSynchronize(ps));
	}
	if (total) {
		/* the regions ride in front of the dense ops, under the one wait behind those (a job with regions has ops) */
		RC_TRY(h_reg.ensure((size_t) total * sizeof(NmRegion)));
		HIP_TRY(hipMemcpyAsync(h_reg.p, d_reg.p, (size_t) total * sizeof(NmRegion), hipMemcpyDeviceToHost, h->s_io));
		if (checks_on) {      /* ... and their checks beside them */
			RC_TRY(h_chk.ensure((size_t) total * sizeof(InvCheck)));
			HIP_TRY(hipMemcpyAsync(h_chk.p, d_chk.p, (size_t) total * sizeof(InvCheck), hipMemcpyDeviceToHost, h->s_io));
		}
		if (!b->ops_total) HIP_TRY(hipStreamSynchronize(h->s_io));
	}
	return CVX_OK;
}

/* A CVX_CREATE_JOB_TEXT handle: the device text stage over the batch's op lists and its sequences in HBM (cvx_text.hip), external
 * clips zero, queued on `st` behind the compaction with no host step in between -- the size pass, the offset scan, then the write
 * into an arena sized by an estimate (job_text_first_capacity over the job's read rows; tune: CVX_TUNE_JOB_TEXT_CAP).  Records,
 * offsets, total and the capacity the write ran with travel in the copies queued here, in front of the event stage_results
 * waits for; the strings themselves with the dense ops (fetch).  rewrite: the arena has grown, only the write runs again. */
int JobText::queue(cvx_batch_s *b, hipStream_t st, bool rewrite, uint64_t tune) {
	const int n = b->n;
	const size_t n1 = (size_t) n;
	if (!rewrite) {
		RC_TRY(d_rec.ensure(n1));
		RC_TRY(d_off.ensure(2 * n1 + 8));
		RC_TRY(d_text.ensure((size_t) job_text_first_capacity(b->n_rows, (uint64_t) n, tune)));
		RC_TRY(h_rec.ensure(n1 * sizeof(TextRec)));
		RC_TRY(h_off.ensure((n1 + 2) * sizeof(unsigned long long)));
		cap = d_text.cap;      /* (a slot's arena never shrinks: a job the arena already holds needs no estimate) */
		rewrites = 0;
	}
	TextArgs a = job_text_args(b);
	a.recs = d_rec.p;
	a.text_len = d_off.p; a.text_off = d_off.p + n1; a.text_total = d_off.p + 2 * n1;
	a.text = d_text.p;
	if (!rewrite) HIP_TRY(launch_job_text_size(a, st));
	HIP_TRY(launch_job_text_bounded(a, cap, st));
	if (!rewrite) {
		HIP_TRY(hipMemcpyAsync(h_off.p, a.text_off, (n1 + 2) * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
		HIP_TRY(hipMemcpyAsync(h_rec.p, d_rec.p, n1 * sizeof(TextRec), hipMemcpyDeviceToHost, st));
	}
	return CVX_OK;
}

void JobText::take_total(int n, bool twin) {
	if (!on) return;
	total = h_off.as<unsigned long long>()[(size_t) n];      /* (the total sits behind the n offsets) */
	if (twin) {      /* Convex::ConvexAlign stores neither field (cvx_job_text does the same to its copy) */
		TextRec *rec = h_rec.as<TextRec>();
		for (int i = 0; i < n; ++i) { rec[i].cigar_op_count = CVX_NOT_WRITTEN; rec[i].sv_type = CVX_NOT_WRITTEN; }
	}
}

int JobText::fetch(cvx_context *h, cvx_batch_s *b) {
	if (!on) return CVX_OK;
	if (total > cap) {
		/* more text than the estimate (sane reads stay below it: CVX_TUNE_JOB_TEXT_CAP reaches this) -- a larger arena, and the
		 * write alone runs again: records, lengths and offsets are still the job's */
		RC_TRY(d_text.ensure((size_t) total));
		cap = d_text.cap;
		rewrites += 1;
		hipStream_t ps = rewrite_stream(h, b);
		RC_TRY(queue(b, ps, true));
		HIP_TRY(hipStreamSynchronize(ps));
	}
	if (total) {
		/* the strings ride in front of the dense ops, under the one wait behind those (only a job without a valid tile has text and no ops) */
		RC_TRY(h_text.ensure((size_t) total));
		HIP_TRY(hipMemcpyAsync(h_text.p, d_text.p, (size_t) total, hipMemcpyDeviceToHost, h->s_io));
		if (!b->ops_total) HIP_TRY(hipStreamSynchronize(h->s_io));
	}
	return CVX_OK;
}

/* ---- the getters: nothing is launched, copied or waited for here -- what queue() put behind the job's compaction came back in
 * the waits of stage_results and stage_ops */

/* what every getter asks first: the handle runs the stage the job ran it and cvx_wait has brought it back */
static int stage_ready(const char *who, cvx_handle h, cvx_job j, bool on_handle, const char *flag_name, bool ran) {
	if (!h || !j) { set_err("%s: NULL argument", who); return CVX_ERR_ARG; }
	if (!on_handle) { set_err("%s: the handle was created without %s", who, flag_name); return CVX_ERR_ARG; }
	if (j->state < kFinished || !j->have_ops || !ran || (j->ladder && !j->ladder->merged)) { set_err("%s: job not finished (call cvx_wait first)", who); return CVX_ERR_ARG; }
	return CVX_OK;
}
static int regions_ready(const char *who, cvx_handle h, cvx_job j) { return stage_ready(who, h, j, h && h->nm_regions, "CVX_CREATE_NM_REGIONS", j && j->jr.on); }
static int texts_ready(const char *who, cvx_handle h, cvx_job j) { return stage_ready(who, h, j, h && h->job_text, "CVX_CREATE_JOB_TEXT", j && j->jt.on); }

/* the capacity the job's first write ran with, as that write reported it behind the offsets and the total (a ladder job: rung 1's) */
static uint64_t first_capacity_of(const PinBuf &h_off, int n) { return n > 0 ? h_off.as<uint64_t>()[(size_t) n + 1] : 0; }

extern "C" {

int cvx_job_regions(cvx_handle h, cvx_job j, const uint64_t **region_off, const cvx_nm_region **regions, const cvx_nm_open **open) {
	ABI_GUARD_BEGIN
	static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the offsets leave as the scan wrote them");
	static_assert(sizeof(NmRegion) == sizeof(cvx_nm_region) && sizeof(NmOpen) == sizeof(cvx_nm_open), "NmRegion / NmOpen mirror cvx_nm_region / cvx_nm_open");
	if (region_off) *region_off = nullptr;
	if (regions) *regions = nullptr;
	if (open) *open = nullptr;
	RC_TRY(regions_ready("cvx_job_regions", h, j));
	const LadderState *L = j->ladder;      /* a ladder job: what cvx_wait merged from its rungs, in the same layout */
	if (region_off) *region_off = L ? L->jr_off.data() : j->jr.h_off.as<uint64_t>();
	/* (NULL for a job that never had a region: nothing to point at) */
	if (regions) *regions = L ? (L->jr_reg.empty() ? nullptr : reinterpret_cast<const cvx_nm_region *>(L->jr_reg.data())) : j->jr.h_reg.as<cvx_nm_region>();
	if (open && j->n > 0) *open = L ? reinterpret_cast<const cvx_nm_open *>(L->jr_open.data()) : j->jr.h_open.as<cvx_nm_open>();
	return CVX_OK;
	ABI_GUARD_END
}

int cvx_job_regions_info(cvx_handle h, cvx_job j, uint64_t *total, uint64_t *first_capacity, int32_t *rewrites) {
	ABI_GUARD_BEGIN
	RC_TRY(regions_ready("cvx_job_regions_info", h, j));
	/* a ladder job: the merged total, the rungs' rewrites summed */
	if (total) *total = j->ladder ? j->ladder->jr_off[(size_t) j->n] : j->jr.total;
	if (first_capacity) *first_capacity = first_capacity_of(j->jr.h_off, j->n);
	if (rewrites) *rewrites = j->ladder ? j->ladder->jr_rewrites : j->jr.rewrites;
	return CVX_OK;
	ABI_GUARD_END
}

int cvx_job_checks(cvx_handle h, cvx_job j, const cvx_inv_check **checks) {
	ABI_GUARD_BEGIN
	static_assert(sizeof(InvCheck) == sizeof(cvx_inv_check) && sizeof(cvx_inv_check) == 16, "InvCheck mirrors cvx_inv_check");
	if (checks) *checks = nullptr;
	if (!checks) { set_err("cvx_job_checks: NULL argument"); return CVX_ERR_ARG; }
	RC_TRY(stage_ready("cvx_job_checks", h, j, h && h->inv_checks, "CVX_CREATE_INV_CHECKS", j && j->jr.on));
	const LadderState *L = j->ladder;      /* a ladder job: the checks cvx_wait merged beside its regions; else they came with the regions (fetch) */
	if (j->jr.checks_on && (L ? !L->jr_chk.empty() : j->jr.total > 0))
		*checks = L ? reinterpret_cast<const cvx_inv_check *>(L->jr_chk.data()) : j->jr.h_chk.as<cvx_inv_check>();
	return CVX_OK;
	ABI_GUARD_END
}

int cvx_job_texts(cvx_handle h, cvx_job j, const cvx_alignment_text **recs, const uint64_t **text_off, const char **text) {
	ABI_GUARD_BEGIN
	static_assert(sizeof(TextRec) == sizeof(cvx_alignment_text), "TextRec mirrors cvx_alignment_text");
	static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the offsets leave as the scan wrote them");
	if (recs) *recs = nullptr;
	if (text_off) *text_off = nullptr;
	if (text) *text = nullptr;
	RC_TRY(texts_ready("cvx_job_texts", h, j));
	const LadderState *L = j->ladder;      /* a ladder job: what cvx_wait merged from its rungs, in the same layout */
	if (recs && j->n > 0) *recs = L ? reinterpret_cast<const cvx_alignment_text *>(L->jt_rec.data()) : j->jt.h_rec.as<cvx_alignment_text>();
	if (text_off) *text_off = L ? L->jt_off.data() : j->jt.h_off.as<uint64_t>();
	if (text) *text = j->n <= 0 ? "" : L ? L->jt_text.data() : j->jt.h_text.as<char>();
	return CVX_OK;
	ABI_GUARD_END
}

int cvx_job_texts_info(cvx_handle h, cvx_job j, uint64_t *total_bytes, uint64_t *first_capacity, int32_t *rewrites) {
	ABI_GUARD_BEGIN
	RC_TRY(texts_ready("cvx_job_texts_info", h, j));
	if (total_bytes) *total_bytes = j->ladder ? j->ladder->jt_off[(size_t) j->n] : j->jt.total;
	if (first_capacity) *first_capacity = first_capacity_of(j->jt.h_off, j->n);
	if (rewrites) *rewrites = j->ladder ? j->ladder->jt_rewrites : j->jt.rewrites;
	return CVX_OK;
	ABI_GUARD_END
}

}  /* extern "C" */
