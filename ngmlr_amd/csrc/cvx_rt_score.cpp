/*
 * cvx_rt_score.cpp -- sub-read scoring (the StrippedSW scores of ngmlr's interval and inversion checks) over the
 * kernels of cvx_score.hip and cvx_score_wave.hip.  Both forms are one job of the handle's scoring state, packed, copied,
 * launched and copied back by score_job_enqueue on the handle's `main` stream: cvx_score_batch waits for it at once,
 * cvx_score_submit hands it to the caller (cvx_score_poll / cvx_score_wait).
 */
#include <algorithm>
#include <cstring>
#include <vector>

#include "cvx_rt.h"
#include "cvx_score_wave.h"

/* One scoring call: the pairs reordered by shape class (slot order), each class a contiguous range of the pair table and of the
 * output, launched one after the other on the handle's stream; order[slot] is the caller's index.  Kept for reuse once waited
 * for, with its per-call vectors: no allocation on the steady-state path. */
struct cvx_score_job_s {
	cvx_context *h = nullptr;
	int32_t n = 0;
	PinBuf hseq, hpairs, hout;
	std::vector<size_t> rl, ql;      /* per pair: bytes of the reference and of the query, NULs included */
	std::vector<int> cls;            /* ... and its shape class */
	std::vector<int32_t> order;
	DevBuf<uint8_t> seq;
	DevBuf<ScorePair> pairs;
	DevBuf<int32_t> rows;
	DevBuf<float> out;
	hipEvent_t ev0 = nullptr, ev1 = nullptr, done = nullptr;
	void release() {
		hseq.release(); hpairs.release(); hout.release();
		seq.release(); pairs.release(); rows.release(); out.release();
		if (ev0) (void) hipEventDestroy(ev0);
		if (ev1) (void) hipEventDestroy(ev1);
		if (done) (void) hipEventDestroy(done);
		ev0 = ev1 = done = nullptr;
	}
};

/* a handle's scoring jobs: the ones waited for, kept for reuse, and the ones in flight (cvx_destroy frees both) */
struct cvx_score_state {
	std::vector<cvx_score_job_s *> free, live;
	float kernel_ms = 0.0f;          /* the kernels of the last call waited for (cvx_score_kernel_ms) */
};

namespace cvx {
void score_state_free(cvx_score_state *ss) {
	if (!ss) return;
	for (cvx_score_job_s *j : ss->free) { j->release(); delete j; }
	for (cvx_score_job_s *j : ss->live) { j->release(); delete j; }
	delete ss;
}
}  // namespace cvx

namespace {
/* shape classes of cvx_score_submit, in launch order */
enum { kScDiag = 0, kScWave1, kScWave2, kScWave4, kScWave8, kScWave16, kScRows, kScClasses };

int score_class(size_t rl, size_t ql, bool no_diag) {
	if (ql <= 512 && rl <= 2048 && !no_diag) return kScDiag;             /* cvx_score_batch's condition, per pair */
	switch (score_wave_rows((int64_t) std::min(rl, ql))) {
	case 1: return kScWave1;
	case 2: return kScWave2;
	case 4: return kScWave4;
	case 8: return kScWave8;
	case 16: return kScWave16;
	default: return kScRows;
	}
}

/* a job of the handle's scoring state (made by the first call), on its live list */
cvx_score_job_s *score_job_acquire(cvx_context *h, int32_t n) {
	if (!h->score) h->score = new cvx_score_state();
	cvx_score_state *ss = h->score;
	cvx_score_job_s *j;
	if (!ss->free.empty()) { j = ss->free.back(); ss->free.pop_back(); }
	else j = new cvx_score_job_s();
	j->h = h;
	j->n = n;
	ss->live.push_back(j);
	return j;
}

void score_job_recycle(cvx_score_job_s *j) {
	cvx_score_state *ss = j->h->score;
	ss->live.erase(std::find(ss->live.begin(), ss->live.end(), j));
	ss->free.push_back(j);
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
	if (!j->ev0) {
		HIP_TRY(hipEventCreate(&j->ev0));
		HIP_TRY(hipEventCreate(&j->ev1));
		HIP_TRY(hipEventCreateWithFlags(&j->done, hipEventBlockingSync | hipEventDisableTiming));
	}
	hipStream_t st = h->s_main;
	HIP_TRY(hipMemcpyAsync(j->seq.p, hseq, (size_t) ((bytes + 255) / 256 * 256), hipMemcpyHostToDevice, st));   /* dword-aligned size: SDMA, not a blit kernel */
	HIP_TRY(hipMemcpyAsync(j->pairs.p, pairs, (size_t) n * sizeof(ScorePair), hipMemcpyHostToDevice, st));
	/* the kernels alone, on the stream they run on (cvx_score_kernel_ms: the device-resident rate beside the marshalled one) */
	HIP_TRY(hipEventRecord(j->ev0, st));
	static const int kRows[kScClasses] = {0, 1, 2, 4, 8, 16, 0};
	for (int c = 0; c < kScClasses; ++c) {
		if (!count[c]) continue;
		const ScorePair *cp = j->pairs.p + first[c];
		float *co = j->out.p + first[c];
		const int cn = (int) count[c];
		if (c == kScDiag) HIP_TRY(launch_score_diag(j->seq.p, cp, co, cn, st));      /* the batched shape (256-base sub-read x ~300-base window) */
		else if (c == kScRows) HIP_TRY(launch_score(j->seq.p, cp, j->rows.p, co, cn, (int) std::min<size_t>(whole_call ? max_rl : std::max<size_t>(max_rl_rows, 513), 0x7fffffff), st));
		else HIP_TRY(launch_score_wave(j->seq.p, cp, co, cn, kRows[c], st));
	}
	HIP_TRY(hipEventRecord(j->ev1, st));
	HIP_TRY(hipMemcpyAsync(j->hout.p, j->out.p, (size_t) n * sizeof(float), hipMemcpyDeviceToHost, st));
	HIP_TRY(hipEventRecord(j->done, st));
	return CVX_OK;
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
			for (int32_t s = 0; s < j->n; ++s) scores[j->order[(size_t) s]] = o[s];
			j->h->score->kernel_ms = ev_ms(j->ev0, j->ev1);
		}
	}
	score_job_recycle(j);
	return rc;
	ABI_GUARD_END
}

int cvx_stage_kernel_ms(cvx_handle h, int32_t stage, float *ms) {
	ABI_GUARD_BEGIN
	if (!h || !ms) { set_err("cvx_stage_kernel_ms: NULL argument"); return CVX_ERR_ARG; }
	switch (stage) {
	case CVX_STAGE_SCORE: *ms = h->score ? h->score->kernel_ms : 0.0f; return CVX_OK;
	case CVX_STAGE_DECODE: *ms = h->decode_kernel_ms; return CVX_OK;
	case CVX_STAGE_SEARCH: *ms = search_kernel_ms(h->search); return CVX_OK;
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
