/*
 * cvx_rt_score.cpp -- sub-read scoring (the StrippedSW scores of ngmlr's interval and inversion checks) over the
 * kernels of cvx_score.hip and cvx_score_wave.hip.  Both forms are one job of the handle's scoring state, packed, copied,
 * launched and copied back by score_job_enqueue on the handle's `main` stream: cvx_score_batch waits for it at once,
 * cvx_score_submit hands it to the caller (cvx_score_poll / cvx_score_wait).  cvx_score_windows* are the same job with its
 * strings written on the device (score_windows_enqueue: stage_score_windows_kernel of cvx_score_stage.hip in front of the
 * class launches); the host half of that -- lengths, classes, offsets -- is cvx_score_windows.h.
 */
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "cvx_rt.h"
#include "cvx_score_stage.h"
#include "cvx_score_wave.h"
#include "cvx_score_windows.h"

/* One scoring call: the pairs reordered by shape class (slot order), each class a contiguous range of the pair table and of the
 * output, launched one after the other on the handle's stream; order[slot] is the caller's index.  Kept for reuse once waited
 * for, with its per-call vectors: no allocation on the steady-state path. */
struct cvx_score_job_s {
	cvx_context *h = nullptr;
	int32_t n = 0;
	int32_t n_scored = 0;            /* slots [0, n_scored) were launched; the others (a window whose decode fails) score -1.0f */
	bool windows = false;            /* a cvx_score_windows* job: ev_st lies between the stage kernel and the class launches */
	PinBuf hseq, hpairs, hout;
	PinBuf hreads, hdesc;            /* cvx_score_windows*: the call's read block and its ScoreWinDesc table */
	ScoreWinPlan plan;
	DevBuf<uint8_t> reads;
	DevBuf<ScoreWinDesc> desc;
	Event ev_st;
	std::vector<size_t> rl, ql;      /* per pair: bytes of the reference and of the query, NULs included */
	std::vector<int> cls;            /* ... and its shape class */
	std::vector<int32_t> order;
	DevBuf<uint8_t> seq;
	DevBuf<ScorePair> pairs;
	DevBuf<int32_t> rows;
	DevBuf<float> out;
	Event ev0, ev1, done;
};

/* a handle's scoring jobs: the ones waited for, kept for reuse, and the ones in flight (cvx_destroy frees both) */
struct cvx_score_state {
	std::vector<cvx_score_job_s *> free, live;
	float kernel_ms = 0.0f;          /* the kernels of the last call waited for (cvx_score_kernel_ms) */
	float stage_ms = 0.0f;           /* ... of them stage_score_windows_kernel (CVX_STAGE_SCORE_WINDOWS; 0 for a call on strings) */
};

namespace cvx {
void score_state_free(cvx_score_state *ss) {
	if (!ss) return;
	for (cvx_score_job_s *j : ss->free) delete j;
	for (cvx_score_job_s *j : ss->live) delete j;
	delete ss;
}
}  // namespace cvx

namespace {
/* a job of the handle's scoring state (made by the first call), on its live list */
cvx_score_job_s *score_job_acquire(cvx_context *h, int32_t n) {
	if (!h->score) {
		h->score = new cvx_score_state();
		/* (the class rule's own statement of score_wave_rows, cvx_score_windows.h, against the kernel's: once per handle) */
		for (int64_t len = 1; len <= kScoreWaveMaxShort + 2; ++len)
			if (score_class_wave_rows(len) != score_wave_rows(len)) { fprintf(stderr, "cvx: score_class_wave_rows(%lld) differs from score_wave_rows\n", (long long) len); abort(); }
	}
	cvx_score_state *ss = h->score;
	cvx_score_job_s *j;
	if (!ss->free.empty()) { j = ss->free.back(); ss->free.pop_back(); }
	else j = new cvx_score_job_s();
	j->h = h;
	j->n = n;
	j->n_scored = n;
	j->windows = false;
	ss->live.push_back(j);
	return j;
}

void score_job_recycle(cvx_score_job_s *j) {
	cvx_score_state *ss = j->h->score;
	ss->live.erase(std::find(ss->live.begin(), ss->live.end(), j));
	ss->free.push_back(j);
}

/* one launch per shape class with pairs, in class order on st: class c holds the slots [first[c], first[c + 1]) */
int score_launch_classes(cvx_score_job_s *j, const size_t *first, bool whole_call, size_t max_rl, size_t max_rl_rows, hipStream_t st) {
	static const int kRows[kScClasses] = {0, 1, 2, 4, 8, 16, 0};
	for (int c = 0; c < kScClasses; ++c) {
		if (first[c + 1] == first[c]) continue;
		const ScorePair *cp = j->pairs.p + first[c];
		float *co = j->out.p + first[c];
		const int cn = (int) (first[c + 1] - first[c]);
		if (c == kScDiag) HIP_TRY(launch_score_diag(j->seq.p, cp, co, cn, st));      /* the batched shape (256-base sub-read x ~300-base window) */
		else if (c == kScRows) HIP_TRY(launch_score(j->seq.p, cp, j->rows.p, co, cn, (int) std::min<size_t>(whole_call ? max_rl : std::max<size_t>(max_rl_rows, 513), 0x7fffffff), st));
		else HIP_TRY(launch_score_wave(j->seq.p, cp, co, cn, kRows[c], st));
	}
	return CVX_OK;
}

int score_job_events(cvx_score_job_s *j) {
	HIP_TRY(j->ev0.make());
	HIP_TRY(j->ev1.make());
	HIP_TRY(j->ev_st.make());
	HIP_TRY(j->done.make(hipEventBlockingSync | hipEventDisableTiming));
	return CVX_OK;
}

/* Measures and packs the job's pairs, copies them to the device, launches, and queues the copy back and the job's `done` event.
 * whole_call (cvx_score_batch): one class for the whole call -- the diagonal kernel when every pair fits it, else launch_score
 * over all pairs with the longest reference of the call, which keeps score_reg_kernel<5> / <8> serving short calls; otherwise
 * (cvx_score_submit) every pair by its own class, launch_score's reference length floored at 513. */
int score_job_enqueue(cvx_context *h, cvx_score_job_s *j, int32_t n, const char *const *refs, const char *const *qrys, bool whole_call, const char *who) {
	HIP_TRY(hipSetDevice(h->device));
	std::vector<size_t> &rl = j->rl, &ql = j->ql;
	std::vector<int> &cls = j->cls;
	rl.resize((size_t) n); ql.resize((size_t) n); cls.resize((size_t) n);
	size_t count[kScClasses] = {0}, max_rl = 0, max_rl_rows = 0;
	uint64_t bytes = 0, rows = 0;
	bool all_diag = true;
	for (int i = 0; i < n; ++i) {
		if (!refs[i] || !qrys[i]) { set_err("%s: NULL sequence %d", who, i); return CVX_ERR_ARG; }
		rl[i] = strlen(refs[i]) + 1;
		ql[i] = strlen(qrys[i]) + 1;
		cls[i] = score_class(rl[i], ql[i], h->score_no_diag);
		all_diag = all_diag && cls[i] == kScDiag;
		max_rl = std::max(max_rl, rl[i]);
		bytes += rl[i] + ql[i];
	}
	if (whole_call) std::fill(cls.begin(), cls.end(), all_diag ? (int) kScDiag : (int) kScRows);
	for (int i = 0; i < n; ++i) ++count[cls[i]];
	size_t first[kScClasses + 1] = {0};
	for (int c = 0; c < kScClasses; ++c) first[c + 1] = first[c] + count[c];
	size_t fill[kScClasses];
	memcpy(fill, first, sizeof(fill));
	j->order.resize((size_t) n);
	for (int i = 0; i < n; ++i) j->order[fill[cls[i]]++] = i;
	RC_TRY(j->hpairs.ensure((size_t) n * sizeof(ScorePair)));
	RC_TRY(j->hout.ensure((size_t) n * sizeof(float)));
	RC_TRY(j->hseq.ensure((size_t) bytes + 256));
	ScorePair *pairs = j->hpairs.as<ScorePair>();
	uint8_t *hseq = j->hseq.as<uint8_t>();
	bytes = 0;
	for (int s = 0; s < n; ++s) {
		const int i = j->order[(size_t) s];
		ScorePair &p = pairs[s];
		p.ref_off = bytes; memcpy(hseq + bytes, refs[i], rl[i]); bytes += rl[i];
		p.qry_off = bytes; memcpy(hseq + bytes, qrys[i], ql[i]); bytes += ql[i];
		p.ref_len = (int32_t) std::min<size_t>(rl[i], 0x7fffffff);
		p.qry_len = (int32_t) std::min<size_t>(ql[i], 0x7fffffff);
		p.scratch_off = 0;
		if ((size_t) s >= first[kScRows] && rl[i] < 100000 && ql[i] < 100000) {    /* score_kernel's two DP rows */
			p.scratch_off = rows;
			rows += 2 * (uint64_t) rl[i];
			max_rl_rows = std::max(max_rl_rows, rl[i]);
		}
	}
	RC_TRY(j->seq.ensure((size_t) bytes + 256));
	RC_TRY(j->pairs.ensure((size_t) n));
	RC_TRY(j->rows.ensure((size_t) rows + 64));
	RC_TRY(j->out.ensure((size_t) n));
	RC_TRY(score_job_events(j));
	hipStream_t st = h->s_main;
	HIP_TRY(hipMemcpyAsync(j->seq.p, hseq, (size_t) ((bytes + 255) / 256 * 256), hipMemcpyHostToDevice, st));   /* dword-aligned size: SDMA, not a blit kernel */
	HIP_TRY(hipMemcpyAsync(j->pairs.p, pairs, (size_t) n * sizeof(ScorePair), hipMemcpyHostToDevice, st));
	/* the kernels alone, on the stream they run on (cvx_score_kernel_ms: the device-resident rate beside the marshalled one) */
	HIP_TRY(hipEventRecord(j->ev0, st));
	RC_TRY(score_launch_classes(j, first, whole_call, max_rl, max_rl_rows, st));
	HIP_TRY(hipEventRecord(j->ev1, st));
	HIP_TRY(hipMemcpyAsync(j->hout.p, j->out.p, (size_t) n * sizeof(float), hipMemcpyDeviceToHost, st));
	HIP_TRY(hipEventRecord(j->done, st));
	return CVX_OK;
}

/* The same job with its strings written on the device: plans the call (cvx_score_windows.h), copies the read block and one
 * ScoreWinDesc per pair, and queues stage_score_windows_kernel in front of the class launches.  Every pair goes by its own class,
 * as in cvx_score_submit.  stage_only (cvx_stage_windows): no scoring, the sequence arena comes back into hseq instead. */
int score_windows_enqueue(cvx_context *h, const cvx_genome_s *g, cvx_score_job_s *j, int32_t n_reads, const uint8_t *arena, const uint64_t *offsets,
		int32_t n, const cvx_score_window *pairs, bool stage_only, const char *who) {
	HIP_TRY(hipSetDevice(h->device));
	ScoreWinPlan &pl = j->plan;
	int64_t bad = 0;
	if (score_windows_plan(score_windows_concat_len(g->n_nibbles), n_reads, offsets, n, pairs, h->score_no_diag, pl, &bad) != CVX_OK) {
		if (bad < 0) set_err("%s: the offsets of read %lld do not ascend (or span 2 GB)", who, (long long) (-1 - bad));
		else set_err("%s: pair %lld has buffer_len %d, read %d of %d", who, (long long) bad, pairs[bad].buffer_len, pairs[bad].read, n_reads);
		return CVX_ERR_ARG;
	}
	j->order = pl.order;
	j->windows = true;
	j->n_scored = stage_only ? 0 : pl.n_scored();
	const uint64_t rbytes = offsets[n_reads] - offsets[0];
	RC_TRY(j->hreads.ensure((size_t) rbytes + 256));
	RC_TRY(j->hdesc.ensure((size_t) n * sizeof(ScoreWinDesc)));
	RC_TRY(j->hout.ensure((size_t) n * sizeof(float)));
	if (stage_only) RC_TRY(j->hseq.ensure((size_t) pl.seq_bytes + 256));
	memcpy(j->hreads.p, arena + offsets[0], (size_t) rbytes);
	memset(j->hreads.as<uint8_t>() + rbytes, 0, 256);
	memcpy(j->hdesc.p, pl.desc.data(), (size_t) n * sizeof(ScoreWinDesc));
	RC_TRY(j->reads.ensure((size_t) rbytes + 256));
	RC_TRY(j->desc.ensure((size_t) n));
	RC_TRY(j->seq.ensure((size_t) pl.seq_bytes + 256));
	RC_TRY(j->pairs.ensure((size_t) n));
	RC_TRY(j->rows.ensure((size_t) pl.rows + 64));
	RC_TRY(j->out.ensure((size_t) n));
	RC_TRY(score_job_events(j));
	hipStream_t st = h->s_main;
	HIP_TRY(hipMemcpyAsync(j->reads.p, j->hreads.p, (size_t) ((rbytes + 255) / 256 * 256), hipMemcpyHostToDevice, st));   /* (dword-aligned size, as above) */
	HIP_TRY(hipMemcpyAsync(j->desc.p, j->hdesc.p, (size_t) n * sizeof(ScoreWinDesc), hipMemcpyHostToDevice, st));
	HIP_TRY(hipEventRecord(j->ev0, st));
	/* every slot is staged, the ones whose decode fails too (an empty window): cvx_stage_windows shows them; no class holds them */
	HIP_TRY(launch_stage_score_windows(g->d_bin.p, j->reads.p, j->desc.p, n, j->seq.p, j->pairs.p, st));
	HIP_TRY(hipEventRecord(j->ev_st, st));
	if (!stage_only) RC_TRY(score_launch_classes(j, pl.first, false, 0, pl.max_rl_rows, st));
	HIP_TRY(hipEventRecord(j->ev1, st));
	if (j->n_scored > 0) HIP_TRY(hipMemcpyAsync(j->hout.p, j->out.p, (size_t) j->n_scored * sizeof(float), hipMemcpyDeviceToHost, st));
	if (stage_only && pl.seq_bytes > 0) HIP_TRY(hipMemcpyAsync(j->hseq.p, j->seq.p, (size_t) pl.seq_bytes, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipEventRecord(j->done, st));
	return CVX_OK;
}

bool score_windows_args_ok(cvx_handle h, cvx_genome g, int32_t n_reads, const uint8_t *arena, const uint64_t *offsets, int32_t n,
		const cvx_score_window *pairs, const char *who) {
	if (!h || !g || n_reads < 0 || n < 0 || !offsets || (n_reads > 0 && !arena) || (n > 0 && !pairs)) { set_err("%s: bad argument", who); return false; }
	if (g->device != h->device) { set_err("%s: the genome lies on device %d, the handle on %d", who, g->device, h->device); return false; }
	return true;
}
}  // namespace

extern "C" {

int cvx_score_batch(cvx_handle h, int32_t n, const char *const *refs, const char *const *qrys, float *scores) {
	ABI_GUARD_BEGIN
	if (!h || n < 0 || (n > 0 && (!refs || !qrys || !scores))) { set_err("cvx_score_batch: bad argument"); return CVX_ERR_ARG; }
	if (n == 0) return CVX_OK;
	/* waited for on the job's blocking event, not by spinning on the stream: in ngmlr dozens of worker threads sit in this call
	 * at the same time on a host that needs its cores for the stages that stayed on the CPU */
	cvx_score_job_s *j = score_job_acquire(h, n);
	const int rc = score_job_enqueue(h, j, n, refs, qrys, true, "cvx_score_batch");
	if (rc != CVX_OK) { score_job_recycle(j); return rc; }
	return cvx_score_wait(j, scores);      /* (recycles the job) */
	ABI_GUARD_END
}

int cvx_score_submit(cvx_handle h, int32_t n, const char *const *refs, const char *const *qrys, cvx_score_job *job) {
	ABI_GUARD_BEGIN
	if (!h || !job || n < 0 || (n > 0 && (!refs || !qrys))) { set_err("cvx_score_submit: bad argument"); return CVX_ERR_ARG; }
	*job = nullptr;
	cvx_score_job_s *j = score_job_acquire(h, n);
	if (n > 0) {
		const int rc = score_job_enqueue(h, j, n, refs, qrys, false, "cvx_score_submit");
		if (rc != CVX_OK) { score_job_recycle(j); return rc; }
	}
	*job = j;
	return CVX_OK;
	ABI_GUARD_END
}

int cvx_score_poll(cvx_score_job j) {
	ABI_GUARD_BEGIN
	if (!j) { set_err("cvx_score_poll: NULL job"); return CVX_ERR_ARG; }
	if (j->n == 0) return 1;
	const hipError_t e = hipEventQuery(j->done);
	if (e == hipSuccess) return 1;
	if (e == hipErrorNotReady) return 0;
	(void) hipGetLastError();
	set_err("cvx_score_poll: %s", hipGetErrorString(e));
	return CVX_ERR_HIP;
	ABI_GUARD_END
}

int cvx_score_wait(cvx_score_job j, float *scores) {
	ABI_GUARD_BEGIN
	if (!j || (j->n > 0 && !scores)) { set_err("cvx_score_wait: bad argument"); return CVX_ERR_ARG; }
	int rc = CVX_OK;
	if (j->n > 0) {
		const hipError_t e = hipEventSynchronize(j->done);
		if (e != hipSuccess) {
			(void) hipGetLastError();
			set_err("cvx_score_wait: %s", hipGetErrorString(e));
			rc = CVX_ERR_HIP;
		} else {
			const float *o = j->hout.as<float>();
			for (int32_t s = 0; s < j->n; ++s) scores[j->order[(size_t) s]] = s < j->n_scored ? o[s] : -1.0f;
			j->h->score->kernel_ms = ev_ms(j->ev0, j->ev1);
			j->h->score->stage_ms = j->windows ? ev_ms(j->ev0, j->ev_st) : 0.0f;
		}
	}
	score_job_recycle(j);
	return rc;
	ABI_GUARD_END
}

int cvx_score_windows_submit(cvx_handle h, cvx_genome g, int32_t n_reads, const uint8_t *arena, const uint64_t *offsets,
		int32_t n, const cvx_score_window *pairs, cvx_score_job *job) {
	ABI_GUARD_BEGIN
	if (!job) { set_err("cvx_score_windows_submit: bad argument"); return CVX_ERR_ARG; }
	*job = nullptr;
	if (!score_windows_args_ok(h, g, n_reads, arena, offsets, n, pairs, "cvx_score_windows_submit")) return CVX_ERR_ARG;
	cvx_score_job_s *j = score_job_acquire(h, n);
	if (n > 0) {
		const int rc = score_windows_enqueue(h, g, j, n_reads, arena, offsets, n, pairs, false, "cvx_score_windows_submit");
		if (rc != CVX_OK) { score_job_recycle(j); return rc; }
	}
	*job = j;
	return CVX_OK;
	ABI_GUARD_END
}

int cvx_score_windows(cvx_handle h, cvx_genome g, int32_t n_reads, const uint8_t *arena, const uint64_t *offsets,
		int32_t n, const cvx_score_window *pairs, float *scores, int32_t *status) {
	ABI_GUARD_BEGIN
	if (n > 0 && !scores) { set_err("cvx_score_windows: bad argument"); return CVX_ERR_ARG; }
	if (!score_windows_args_ok(h, g, n_reads, arena, offsets, n, pairs, "cvx_score_windows")) return CVX_ERR_ARG;
	if (n == 0) return CVX_OK;
	cvx_score_job_s *j = score_job_acquire(h, n);
	const int rc = score_windows_enqueue(h, g, j, n_reads, arena, offsets, n, pairs, false, "cvx_score_windows");
	if (rc != CVX_OK) { score_job_recycle(j); return rc; }
	if (status) for (int32_t i = 0; i < n; ++i) status[i] = j->plan.cls[(size_t) i] == kScClasses;
	return cvx_score_wait(j, scores);      /* (recycles the job) */
	ABI_GUARD_END
}

int cvx_stage_windows(cvx_handle h, cvx_genome g, int32_t n_reads, const uint8_t *arena, const uint64_t *offsets,
		int32_t n, const cvx_score_window *pairs, uint8_t *out, uint64_t cap, uint64_t *ref_off, uint64_t *qry_off,
		int32_t *status, uint64_t *used) {
	ABI_GUARD_BEGIN
	if (!used || (n > 0 && (!ref_off || !qry_off)) || (cap > 0 && !out)) { set_err("cvx_stage_windows: bad argument"); return CVX_ERR_ARG; }
	if (!score_windows_args_ok(h, g, n_reads, arena, offsets, n, pairs, "cvx_stage_windows")) return CVX_ERR_ARG;
	*used = 0;
	if (n == 0) return CVX_OK;
	cvx_score_job_s *j = score_job_acquire(h, n);
	int rc = score_windows_enqueue(h, g, j, n_reads, arena, offsets, n, pairs, true, "cvx_stage_windows");
	if (rc != CVX_OK) { score_job_recycle(j); return rc; }
	const hipError_t e = hipEventSynchronize(j->done);
	if (e != hipSuccess) {
		(void) hipGetLastError();
		set_err("cvx_stage_windows: %s", hipGetErrorString(e));
		rc = CVX_ERR_HIP;
	} else {
		const ScoreWinPlan &pl = j->plan;
		*used = pl.seq_bytes;
		for (int32_t s = 0; s < n; ++s) {
			const int32_t i = pl.order[(size_t) s];
			ref_off[i] = pl.desc[(size_t) s].ref_off;
			qry_off[i] = pl.desc[(size_t) s].qry_off;
			if (status) status[i] = pl.cls[(size_t) i] == kScClasses;
		}
		if (cap < pl.seq_bytes) { set_err("cvx_stage_windows: %llu bytes needed, %llu given", (unsigned long long) pl.seq_bytes, (unsigned long long) cap); rc = CVX_ERR_CAPACITY; }
		else memcpy(out, j->hseq.p, (size_t) pl.seq_bytes);
		j->h->score->kernel_ms = ev_ms(j->ev0, j->ev1);
		j->h->score->stage_ms = ev_ms(j->ev0, j->ev_st);
	}
	score_job_recycle(j);
	return rc;
	ABI_GUARD_END
}

int cvx_stage_windows_host(const uint8_t *bin_ref, uint64_t n_nibbles, const uint64_t *start_table, int32_t n_starts,
		int32_t n_reads, const uint8_t *arena, const uint64_t *offsets, int32_t n, const cvx_score_window *pairs,
		uint8_t *out, uint64_t cap, uint64_t *ref_off, uint64_t *qry_off, int32_t *status, uint64_t *used) {
	ABI_GUARD_BEGIN
	uint64_t L = 0;
	if (!bin_ref || !used || n_reads < 0 || n < 0 || !offsets || (n_reads > 0 && !arena) || (n > 0 && (!pairs || !ref_off || !qry_off)) || (cap > 0 && !out) ||
			cvx_genome_concat_len(n_nibbles, start_table, n_starts, &L) != CVX_OK) { set_err("cvx_stage_windows_host: bad argument"); return CVX_ERR_ARG; }
	*used = 0;
	ScoreWinPlan pl;
	int64_t bad = 0;
	if (score_windows_plan(L, n_reads, offsets, n, pairs, false, pl, &bad) != CVX_OK) {
		if (bad < 0) set_err("cvx_stage_windows_host: the offsets of read %lld do not ascend (or span 2 GB)", (long long) (-1 - bad));
		else set_err("cvx_stage_windows_host: pair %lld has buffer_len %d, read %d of %d", (long long) bad, pairs[bad].buffer_len, pairs[bad].read, n_reads);
		return CVX_ERR_ARG;
	}
	*used = pl.seq_bytes;
	for (int32_t s = 0; s < n; ++s) {
		const int32_t i = pl.order[(size_t) s];
		ref_off[i] = pl.desc[(size_t) s].ref_off;
		qry_off[i] = pl.desc[(size_t) s].qry_off;
		if (status) status[i] = pl.cls[(size_t) i] == kScClasses;
	}
	if (cap < pl.seq_bytes) { set_err("cvx_stage_windows_host: %llu bytes needed, %llu given", (unsigned long long) pl.seq_bytes, (unsigned long long) cap); return CVX_ERR_CAPACITY; }
	if (n > 0 && !score_windows_stage_host(bin_ref, L, pairs, pl, arena + offsets[0], out)) { set_err("cvx_stage_windows_host: a window is not as long as planned"); return CVX_ERR_HIP; }
	return CVX_OK;
	ABI_GUARD_END
}

int cvx_genome_concat_len(uint64_t n_nibbles, const uint64_t *start_table, int32_t n_starts, uint64_t *concat_len) {
	ABI_GUARD_BEGIN
	/* (the start table has no say in the length; it only has to lie inside the genome) */
	if (!concat_len || !start_table || n_starts < 2 || n_nibbles < 2 || start_table[n_starts - 2] >= n_nibbles) { set_err("cvx_genome_concat_len: bad argument"); return CVX_ERR_ARG; }
	*concat_len = score_windows_concat_len(n_nibbles);
	return CVX_OK;
	ABI_GUARD_END
}

int cvx_stage_kernel_ms(cvx_handle h, int32_t stage, float *ms) {
	ABI_GUARD_BEGIN
	if (!h || !ms) { set_err("cvx_stage_kernel_ms: NULL argument"); return CVX_ERR_ARG; }
	switch (stage) {
	case CVX_STAGE_SCORE: *ms = h->score ? h->score->kernel_ms : 0.0f; return CVX_OK;
	case CVX_STAGE_SCORE_WINDOWS: *ms = h->score ? h->score->stage_ms : 0.0f; return CVX_OK;
	case CVX_STAGE_DECODE: *ms = h->decode_kernel_ms; return CVX_OK;
	case CVX_STAGE_SEARCH: *ms = search_kernel_ms(h->search); return CVX_OK;
	case CVX_STAGE_SEARCH_SCORE: *ms = search_score_kernel_ms(h->search); return CVX_OK;
	case CVX_STAGE_SEGMENTS: *ms = h->segments_kernel_ms; return CVX_OK;
	default: set_err("cvx_stage_kernel_ms: unknown stage %d", stage); return CVX_ERR_ARG;
	}
	ABI_GUARD_END
}

int cvx_score_kernel_ms(cvx_handle h, float *ms) {
	ABI_GUARD_BEGIN
	if (!h || !ms) { set_err("cvx_score_kernel_ms: NULL argument"); return CVX_ERR_ARG; }
	*ms = h->score ? h->score->kernel_ms : 0.0f;
	return CVX_OK;
	ABI_GUARD_END
}

}  /* extern "C" */
