/*
 * cvx_runtime.cpp -- host side of libcvxalign.so: the C ABI of include/cvx_align.h
 * over the gfx950 kernels of cvx_kernels.hip / cvx_generic.hip / cvx_score.hip.
 *
 * One cvx_context = one device (ngmlr creates one aligner per worker thread, reference
 * src/CS.cpp:418; contexts are independent, a context is not re-entrant -- same contract as
 * the reference's ConvexAlignFast instances).  This file holds what belongs to the process and to
 * the handle: load-time settings, the error string and the build ids, cvx_create_ex / cvx_destroy
 * and the handle's stream set, the page-locked arenas of cvx_host_alloc.  The subsystems have a file
 * each, over the structures and helpers of cvx_rt.h (the error layer: cvx_rt_err.h):
 *
 *   cvx_rt_align.cpp    the alignment job pipeline: the upload / plan / compute / results / ops stages,
 *                       cvx_batch_*, cvx_align_batch, cvx_submit / cvx_wait / cvx_job_*
 *   cvx_rt_stages.cpp   the result stages a handle runs with every job (regions, inversion checks, text): what the
 *                       pipeline's stages call, and cvx_job_regions / _checks / _texts that hand the data out
 *   cvx_rt_ladder.cpp   ladder jobs: cvx_submit_ladder(_ex), the rungs, the merge in cvx_wait (cvx_rt_align.h: what it
 *                       and the pipeline call of each other)
 *   cvx_rt_text.cpp     the device-side text stage of finished jobs and the NM profile
 *   cvx_rt_checks.cpp   the inversion checks of regions the caller holds
 *   cvx_rt_search.cpp   the resident genome and its window decode, the k-mer index, the candidate search
 *   cvx_rt_score.cpp    sub-read scoring, blocking and asynchronous
 *
 * There is no CPU compute path in the runtime: without a device every entry point returns
 * CVX_ERR_NO_DEVICE.
 */
#include <hip/hip_runtime_api.h>
#include <dirent.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "cvx_rt.h"

namespace {

/* the streams the service handles of a process share, per device (cvx_create_ex; never destroyed: they die with the process) */
static const int kServiceStreamsMax = 16, kMaxServiceDevices = 64;
struct ServiceStreams { hipStream_t st[kServiceStreamsMax] = {nullptr}; unsigned next = 0; };
ServiceStreams g_service_streams[kMaxServiceDevices];
std::mutex g_service_mtx;

/* page-locked blocks handed out by cvx_host_alloc: sequences found inside one travel without packing */
std::mutex g_pin_mtx;
std::vector<std::pair<const char *, size_t>> g_pin_blocks;

}  // namespace

namespace cvx {

thread_local std::string g_err;

void set_err(const char *fmt, ...) {
	char buf[512];
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(buf, sizeof(buf), fmt, ap);
	va_end(ap);
	g_err = buf;
}

DeferredFrees g_deferred;

bool in_pinned_block(const void *p, uint64_t bytes) {
	const char *c = static_cast<const char *>(p);
	std::lock_guard<std::mutex> lk(g_pin_mtx);
	for (const auto &b : g_pin_blocks)
		if (c >= b.first && c + bytes <= b.first + b.second) return true;
	return false;
}

float ev_ms(hipEvent_t a, hipEvent_t b) {
	float ms = 0.0f;
	if (hipEventElapsedTime(&ms, a, b) != hipSuccess) { (void) hipGetLastError(); return 0.0f; }
	return ms;
}

int event_fired(hipEvent_t e) {
	const hipError_t q = hipEventQuery(e);
	if (q == hipSuccess) return 1;
	if (q == hipErrorNotReady) { (void) hipGetLastError(); return 0; }
	set_err("hipEventQuery: %s", hipGetErrorString(q));
	return -1;
}

/* the streams of an aligning handle beside `main` (cvx_create makes only that one) */
int ensure_streams(cvx_context *c) {
	if (c->streams_ready.load(std::memory_order_acquire)) return CVX_OK;
	/* (a handle is not re-entrant, but two threads making a handle's first alignment-side calls at once -- stage_upload and
	 * cvx_nm_profile_ops both come here -- must not create the set twice; and a creation that fails half-way leaves what exists in
	 * place: the next call creates only what is missing -- ADVICE r5) */
	std::lock_guard<std::mutex> lk(c->streams_mtx);
	if (c->streams_ready.load(std::memory_order_relaxed)) return CVX_OK;
	int prio_lo = 0, prio_hi = 0;
	(void) hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);     /* numerically lower = higher priority */
	hipError_t e = hipSuccess;
	auto make = [&](hipStream_t *st) { if (e == hipSuccess && *st == nullptr) e = hipStreamCreateWithFlags(st, hipStreamNonBlocking); };
	make(&c->s_post);
	/* the text stage of finished jobs runs beside the fills of the jobs behind them: at normal priority its stream shared a
	 * hardware queue with one of the fill classes and every one of its waits sat out a whole fill kernel (38 ms per launch of
	 * 500 tiles inside ngmlr, profiles/r06_e2e_device_decode.txt); the high-priority queues carry only uploads and plans
	 * (CVX_TEXT_STREAM_PRIO=0: as before) */
	{
		const char *tp = getenv("CVX_TEXT_STREAM_PRIO");
		if (e == hipSuccess && c->s_text == nullptr && !(tp && atoi(tp) == 0)) e = hipStreamCreateWithPriority(&c->s_text, hipStreamNonBlocking, prio_hi);
	}
	make(&c->s_text);
	for (int i = 0; i < kAuxStreams; ++i) make(&c->aux[i]);
	make(&c->s_main2);
	make(&c->s_post2);
	for (int i = 0; i < kAuxStreams; ++i) make(&c->aux2[i]);
	/* the tails of split fill classes (cvx_context::s_tail): one stream at the lowest priority the device has.  Default priority is 0
	 * and numerically greater is lower: a device that reports no such level gets no stream, and no class of the handle is split */
	if (e == hipSuccess && c->s_tail == nullptr && c->tail_split != 0 && prio_lo > 0) e = hipStreamCreateWithPriority(&c->s_tail, hipStreamNonBlocking, prio_lo);
	if (e == hipSuccess) e = hipStreamCreateWithPriority(&c->s_io, hipStreamNonBlocking, prio_hi);
	if (e != hipSuccess) { set_err("hipStreamCreate failed: %s", hipGetErrorString(e)); return CVX_ERR_HIP; }
	c->streams_ready.store(true, std::memory_order_release);      /* last: the whole set exists */
	return CVX_OK;
}

}  // namespace cvx

/* the process's pack threads for the host-only text code (cvx_sam.cpp) */
namespace cvx {
void pack_pool_run(int n_tasks, const std::function<void(int)> &fn) { PackPool::get().run(n_tasks, fn); }
}

/* Before the HIP runtime reads its settings (it does at the first HIP call of the process, which for ngmlr and for bench.py is
 * one of ours): sixteen hardware queues per device instead of the runtime's four.  A handle runs its fill classes side by side
 * on three streams beside the upload stream, and a process holds several handles (ngmlr: the aligner, sixteen search handles,
 * the scoring plugin's); with four hardware queues the streams of a later handle share queues, and two fill classes that
 * share a queue run one after the other -- measured (gpurun_out/r05b): the ONT mix 45 ms per batch on the first handle of a
 * process, 59 ms on every later one (C5 mix: 195 / 288 ms); with eight queues every handle gets the 45 / 195.  Sixteen, not
 * eight, because of ngmlr: there the aligner's fill streams are created when fifty streams of the search and scoring handles
 * exist, and with eight queues two of its classes still landed on one -- the launch trace of the pipeline
 * (CVX_LAUNCH_TRACE=1, profiles/r05_e2e_launch_trace.txt) showed a launch's fill lasting the SUM of its classes (M = 4 10.1 ms +
 * M = 3 7.7 ms = 19 ms of a 20.5 ms launch); with sixteen: 10.7 of 12.2 ms, mapping 3.0 -> 2.6 s for 20 000 reads
 * (profiles/r05_e2e_hw_queues.txt).  The bench configurations do not care (8 against 16: C5 6 834 - 6 887 both, ONT 8 550 - 8 970
 * both); thirty-two oversubscribe the hardware (launches 53 ms in flight).  Not overridden when the user has set
 * GPU_MAX_HW_QUEUES. */
static int g_hwq_set_by_library = 0;            /* 1: the constructor exported GPU_MAX_HW_QUEUES itself (the user had not) */
static std::atomic<int> g_blocking_sync[64];    /* per device: 0 not decided, 1 applied, 2 refused by the runtime, 3 CVX_WAIT=spin */
static int g_runtime_up_at_load = 0;             /* 1: the process had /dev/kfd open when this library was loaded -- a HIP / HSA runtime was already
                                                  * initialised, so the variable exported below cannot reach it any more */
__attribute__((constructor)) static void cvx_process_settings() {
	g_hwq_set_by_library = getenv("GPU_MAX_HW_QUEUES") == nullptr;
	if (DIR *d = opendir("/proc/self/fd")) {
		while (struct dirent *e = readdir(d)) {
			char path[320], target[64];
			snprintf(path, sizeof(path), "/proc/self/fd/%s", e->d_name);
			const ssize_t n = readlink(path, target, sizeof(target) - 1);
			if (n > 0) { target[n] = 0; if (strcmp(target, "/dev/kfd") == 0) { g_runtime_up_at_load = 1; break; } }
		}
		closedir(d);
	}
	setenv("GPU_MAX_HW_QUEUES", "16", 0);
}

extern "C" {

const char *cvx_last_error(void) { return g_err.c_str(); }

int cvx_abi_version(void) { return CVX_ABI_VERSION; }

#ifndef CVX_BUILD_ID
#define CVX_BUILD_ID "unknown"
#endif
const char *cvx_build_id(void) { return CVX_BUILD_ID; }
#ifndef CVX_FILL_ID
#define CVX_FILL_ID "unknown"
#endif
#ifndef CVX_SEARCH_ID
#define CVX_SEARCH_ID "unknown"
#endif
const char *cvx_source_id(const char *family) {
	if (family && strcmp(family, "fill") == 0) return CVX_FILL_ID;
	if (family && strcmp(family, "search") == 0) return CVX_SEARCH_ID;
	return CVX_BUILD_ID;
}

int cvx_device_count(void) {
	ABI_GUARD_BEGIN
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess) return 0;
	return n;
	ABI_GUARD_END
}

int cvx_device_synchronize(int device_id) {
	ABI_GUARD_BEGIN
	HIP_TRY(hipSetDevice(device_id));
	HIP_TRY(hipDeviceSynchronize());
	return CVX_OK;
	ABI_GUARD_END
}

int cvx_create(int device_id, const cvx_params *p, uint64_t max_matrix_mb, cvx_handle *out) {
	ABI_GUARD_BEGIN return cvx_create_ex(device_id, p, max_matrix_mb, 0u, out); ABI_GUARD_END
}

int cvx_runtime_regime(int device_id, cvx_regime *out) {
	ABI_GUARD_BEGIN
	if (!out || device_id < 0) { set_err("cvx_runtime_regime: bad argument"); return CVX_ERR_ARG; }
	memset(out, 0, sizeof(*out));
	const char *q = getenv("GPU_MAX_HW_QUEUES");
	out->hw_queues_env = q ? atoi(q) : 0;
	out->hw_queues_set_by_library = g_hwq_set_by_library;
	const int b = g_blocking_sync[device_id & 63].load();
	out->blocking_sync = b == 1 ? 1 : (b == 0 ? -1 : 0);
	out->blocking_sync_why = b;
	int shared = 4;
	if (const char *e2 = getenv("CVX_SERVICE_STREAMS")) shared = atoi(e2) > 0 ? std::min(atoi(e2), kServiceStreamsMax) : 0;
	out->service_streams = shared;
	out->runtime_up_at_load = g_runtime_up_at_load;
	return CVX_OK;
	ABI_GUARD_END
}

int cvx_create_ex(int device_id, const cvx_params *p, uint64_t max_matrix_mb, uint32_t flags, cvx_handle *out) {
	ABI_GUARD_BEGIN
	if (!p || !out) { set_err("cvx_create: NULL argument"); return CVX_ERR_ARG; }
	*out = nullptr;
	/* The ring kernels implement the scalar recurrence (reference src/ConvexAlignFast.cpp:606-774)
	 * and use its sign structure (match > 0 > every penalty, extension never dearer than its floor).
	 * The SSE path the reference actually runs is identical to that recurrence only while opening a
	 * gap directly off the other gap type can never win: gap_open + gap_ext_min < mismatch (SURVEY.md
	 * Appendix A; the 0.25 keeps float rounding out of the argument).  Any other scoring -- the
	 * reference accepts whatever --match/--mismatch/--gap-* the user passes -- is served by the
	 * catch-all kernel's SSE-variant instantiation, which restates fwdFillMatrixSSESimple cell by cell
	 * (cvx_generic.hip): slower per cell, same results as the reference. */
	const bool finite = std::isfinite(p->match) && std::isfinite(p->mismatch) && std::isfinite(p->gap_open) &&
			std::isfinite(p->gap_extend) && std::isfinite(p->gap_extend_min) && std::isfinite(p->gap_decay);
	if (!finite) {
		set_err("cvx_create: scoring (%g,%g,%g,%g,%g,%g) is not finite",
				p->match, p->mismatch, p->gap_open, p->gap_extend, p->gap_extend_min, p->gap_decay);
		return CVX_ERR_PARAMS;
	}
	if (flags & ~(uint32_t) (CVX_CREATE_SERVICE | CVX_CREATE_SCALAR_TWIN | CVX_CREATE_NM_REGIONS | CVX_CREATE_JOB_TEXT | CVX_CREATE_INV_CHECKS)) { set_err("cvx_create_ex: unknown flags 0x%x", flags); return CVX_ERR_ARG; }
	if ((flags & CVX_CREATE_NM_REGIONS) && (flags & CVX_CREATE_SERVICE)) {
		set_err("cvx_create_ex: CVX_CREATE_NM_REGIONS on a CVX_CREATE_SERVICE handle (a service handle runs no alignment jobs)");
		return CVX_ERR_ARG;
	}
	if ((flags & CVX_CREATE_JOB_TEXT) && (flags & CVX_CREATE_SERVICE)) {
		set_err("cvx_create_ex: CVX_CREATE_JOB_TEXT on a CVX_CREATE_SERVICE handle (a service handle runs no alignment jobs)");
		return CVX_ERR_ARG;
	}
	if ((flags & CVX_CREATE_INV_CHECKS) && (flags & CVX_CREATE_SERVICE)) {
		set_err("cvx_create_ex: CVX_CREATE_INV_CHECKS on a CVX_CREATE_SERVICE handle (a service handle runs no alignment jobs)");
		return CVX_ERR_ARG;
	}
	if ((flags & CVX_CREATE_INV_CHECKS) && !(flags & CVX_CREATE_NM_REGIONS)) {
		set_err("cvx_create_ex: CVX_CREATE_INV_CHECKS without CVX_CREATE_NM_REGIONS (the checks are those of the job's regions)");
		return CVX_ERR_ARG;
	}
	/* (a scalar-twin handle runs the scalar recurrence for any scoring: rings where their sign structure holds, else the
	 * catch-all kernel with scalar rules, never the SSE variant -- fill_semantics, cvx_host_logic.h) */
	const bool scalar_twin = (flags & CVX_CREATE_SCALAR_TWIN) != 0;
	const FillSemantics sem = fill_semantics(p->match, p->mismatch, p->gap_open, p->gap_extend, p->gap_extend_min, p->gap_decay, scalar_twin);
	int ndev = 0;
	if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
		set_err("cvx_create: no HIP device available (the HIP path has no CPU fallback)");
		return CVX_ERR_NO_DEVICE;
	}
	if (device_id < 0 || device_id >= ndev) {
		set_err("cvx_create: device %d out of range (%d devices)", device_id, ndev);
		return CVX_ERR_NO_DEVICE;
	}
	HIP_TRY(hipSetDevice(device_id));
	/* How a host thread waits for this device.  The runtime's default is to spin: hipStreamSynchronize and hipEventSynchronize
	 * burn a core for as long as they wait -- an event created with hipEventBlockingSync included (tools/wait_probe.hip,
	 * profiles/r04_wait_probe.txt: 50.0 ms of thread CPU per 50 ms wait in every form).  Inside ngmlr that is a core per CS
	 * thread parked in a search or scoring call and one for the dispatcher, on a host that needs its cores for the reads'
	 * own code.  With the device in blocking-sync mode the same waits cost 0.5 ms of CPU per 50 ms and return 0.04 ms later.
	 * CVX_WAIT=spin keeps the runtime's default. */
	{
		/* once per device and process, by whichever thread gets here first (the others wait in call_once): the flag is a
		 * process-wide property of the device, documented as such in cvx_align.h; a runtime that refuses it (a context that is
		 * already active with another policy) is reported, the waits then spin */
		static std::once_flag once[64];
		std::call_once(once[device_id & 63], [&] {
			if (g_runtime_up_at_load && g_hwq_set_by_library)
				fprintf(stderr, "cvx_create: a HIP runtime was already initialised when libcvxalign.so was loaded: GPU_MAX_HW_QUEUES=16 came too late for it -- "
						"export it before the process starts, or mixed launches run their fill classes one after the other (cvx_runtime_regime)\n");
			const char *w = getenv("CVX_WAIT");
			if (w && strcmp(w, "spin") == 0) { g_blocking_sync[device_id & 63] = 3; return; }
			const hipError_t fe = hipSetDeviceFlags(hipDeviceScheduleBlockingSync);
			g_blocking_sync[device_id & 63] = fe == hipSuccess ? 1 : 2;
			if (fe != hipSuccess) {
				(void) hipGetLastError();
				fprintf(stderr, "cvx_create: device %d stays in its current scheduling mode (%s): host threads that wait for it will spin\n", device_id, hipGetErrorString(fe));
			}
		});
	}
	hipDeviceProp_t prop;
	HIP_TRY(hipGetDeviceProperties(&prop, device_id));
	if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
		set_err("cvx_create: device %d is %s; this library carries gfx950 code only", device_id, prop.gcnArchName);
		return CVX_ERR_NO_DEVICE;
	}
	cvx_context *c = new (std::nothrow) cvx_context();
	if (!c) return CVX_ERR_OOM;
	c->device = device_id;
	c->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
	c->sp.mat = p->match; c->sp.mis = p->mismatch; c->sp.go = p->gap_open;
	c->sp.ge = p->gap_extend; c->sp.gem = p->gap_extend_min; c->sp.decay = p->gap_decay;
	c->sp.misx = twin_mismatch_x(p->mismatch);
	c->scalar_twin = scalar_twin;
	/* the twin has no matrix-size cap (its AlignmentMatrix::prepare allocates whatever is asked): no tile of a twin handle is
	 * CVX_TILE_TOO_LARGE because of max_matrix_mb */
	c->max_matrix_mb = !sem.matrix_cap ? ~0ull : (max_matrix_mb ? max_matrix_mb : 10000);
	c->sse_variant = sem.sse_variant;
	if (const char *e = getenv("CVX_TUNE_BT_GROUP")) c->bt_group = atoi(e);
	if (const char *e = getenv("CVX_TUNE_BT_PER_CLASS")) c->bt_per_class = atoi(e) != 0;
	if (const char *e = getenv("CVX_TUNE_OVERLAP_POST")) c->overlap_post = atoi(e) != 0;
	if (const char *e = getenv("CVX_TUNE_TAIL_SPLIT")) c->tail_split = std::max(0, atoi(e));
	if (const char *e = getenv("CVX_TUNE_TAIL_ROUNDS")) c->tail_rounds = (float) std::max(0.0, atof(e));
	if (const char *e = getenv("CVX_TUNE_TAIL_TRACE")) c->tail_trace = atoi(e);
	if (const char *e = getenv("CVX_TUNE_TAIL_GATE")) c->tail_gate = atoi(e);
	if (const char *e = getenv("CVX_TUNE_SSE_VARIANT")) c->sse_variant = c->sse_variant || (atoi(e) != 0 && !scalar_twin);   /* test knob */
	c->force_generic = sem.force_generic || c->sse_variant;
	c->pack_threads = PackPool::get().size();      /* the process's shared pack threads (CVX_PACK_THREADS) */
	if (const char *e = getenv("CVX_TUNE_MIN_M")) c->tune_min_slots = atoi(e);
	if (const char *e = getenv("CVX_TUNE_FORCE_WRAP16")) c->tune_force_wrap = atoi(e);
	if (const char *e = getenv("CVX_TUNE_PEN_TABLE")) c->tune_pen_table = atoi(e) != 0;
	{
		/* the table form needs the penalty min(gem, gext + run * decay) to be constant from run kPenClamp on.  With decay >= 0 the sum
		 * never shrinks as the run grows (binary32 multiply and add are monotone), so that is the case exactly when the penalty of run
		 * kPenClamp has already reached gem, or decay is 0 (it is from run 27 on with the default scoring); anything else -- a tiny
		 * decay -- keeps the arithmetic form */
		volatile float prod = (float) kPenClamp * p->gap_decay;
		volatile float at_clamp = p->gap_extend + prod;
		const bool reached = !(at_clamp < p->gap_extend_min);
		if (!(p->gap_decay >= 0.0f) || !(reached || p->gap_decay == 0.0f)) c->tune_pen_table = 0;
		/* the table form without a gang computes on scores scaled by 2^-64 (the clamp bit of its v_max3_f32 is the cell's zero
		 * clamp); a scoring whose values could leave the range in which that is exact keeps the arithmetic form as well */
		if (!score_scale_exact(p->match, p->mismatch, scalar_twin ? c->sp.misx : 0.0f, p->gap_open, p->gap_extend, p->gap_extend_min, p->gap_decay))
			c->tune_pen_table = 0;
	}
	if (const char *e = getenv("CVX_TUNE_FAIL_COMPUTE")) c->test_fail_compute = atoi(e);
	if (const char *e = getenv("CVX_TUNE_SCORE_NO_DIAG")) c->score_no_diag = atoi(e) != 0;
	if (const char *e = getenv("CVX_TUNE_MAX_M")) c->tune_max_slots = atoi(e);
	if (const char *e = getenv("CVX_TUNE_CHAIN_M")) c->tune_chain_m = atoi(e);
	if (const char *e = getenv("CVX_TUNE_CHAIN_PRIO")) c->tune_chain_prio = atoi(e) != 0;
	if (const char *e = getenv("CVX_TUNE_CHAIN_LDS_KB")) c->tune_chain_lds_kb = atoi(e) > 0 ? atoi(e) : 0;
	if (const char *e = getenv("CVX_TUNE_WIDE_PRIO")) c->tune_wide_prio = atoi(e);
	if (const char *e = getenv("CVX_TUNE_EXACT_STEPS")) c->tune_exact_steps = atoi(e);
	if (const char *e = getenv("CVX_TUNE_TWO_LANES")) c->single_lane = atoi(e) == 0;
	if (const char *e = getenv("CVX_TUNE_LONG_STEPS")) c->tune_long_steps = atoi(e);
	if (const char *e = getenv("CVX_TUNE_SMALL_BATCH")) c->tune_small_batch = atoi(e);
	if (const char *e = getenv("CVX_TUNE_LONG_NEED")) c->tune_long_need = atoi(e);
	if (const char *e = getenv("CVX_TUNE_GANGS")) c->tune_gangs = atoi(e) != 0 && !sem.no_gangs;
	if (const char *e = getenv("CVX_TUNE_GANG_PRIO")) c->tune_gang_prio = atoi(e) != 0;
	if (const char *e = getenv("CVX_TUNE_LATE_MIN")) c->tune_late_min = std::max(1, atoi(e));
	c->tune_job_text_cap = job_text_cap_knob(getenv("CVX_TUNE_JOB_TEXT_CAP"));
	if (const char *e = getenv("CVX_TUNE_LATE_SHIFT")) c->tune_late_shift = std::min(16, std::max(0, atoi(e)));
	/* One stream now; the seven others an aligning handle uses (upload, post, text, the fill classes' side streams and the second
	 * set for small jobs) are created by its first alignment call (ensure_streams).  ngmlr holds 32 handles that only ever
	 * score or search on `main`: 224 streams that were created at start-up and destroyed at exit for nothing
	 * (0.8 s between the last alignment and the process's exit, profiles/r04_timeline_e2e.txt). */
	/* A SERVICE handle (CVX_CREATE_SERVICE: ngmlr's 16 searching and 32 scoring handles) makes short, latency-bound calls from a
	 * thread that blocks in them: its stream is created at the device's highest priority, which on this runtime also means a
	 * hardware queue out of another pool than the aligning handle's fill streams' -- 50 normal streams on 16 hardware queues put
	 * fill classes behind each other and scoring kernels behind 10 ms fills (profiles/r06_e2e_launch_trace.txt). */
	hipError_t e = hipSuccess;
	c->service = (flags & CVX_CREATE_SERVICE) != 0;
	c->nm_regions = (flags & CVX_CREATE_NM_REGIONS) != 0;
	c->inv_checks = (flags & CVX_CREATE_INV_CHECKS) != 0;
	c->job_text = (flags & CVX_CREATE_JOB_TEXT) != 0;
	const char *sp = getenv("CVX_SERVICE_PRIO");
	int shared = 4;      /* CVX_SERVICE_STREAMS: streams per device the service handles of a process share (0 = one of its own per handle) */
	if (const char *e2 = getenv("CVX_SERVICE_STREAMS")) shared = atoi(e2) > 0 ? std::min(atoi(e2), kServiceStreamsMax) : 0;
	if (c->service && shared > 0) {
		/* ngmlr holds 32 service handles beside the aligner's ten streams, and the runtime spreads a process's streams over
		 * sixteen hardware queues: two fill classes that land on one queue run one after the other (a launch's fill was the SUM
		 * of its classes again with -t 32, profiles/r06_e2e_launch_trace.txt), a 0.3 ms scoring kernel waits behind a 10 ms fill.
		 * The service handles therefore take turns on a few shared streams -- their calls are short, every call waits on its own
		 * event -- and the process stays below sixteen streams: one hardware queue each. */
		std::lock_guard<std::mutex> lk(g_service_mtx);
		ServiceStreams &ss = g_service_streams[device_id % kMaxServiceDevices];
		const int k = ss.next++ % shared;
		if (ss.st[k] == nullptr) e = hipStreamCreateWithFlags(&ss.st[k], hipStreamNonBlocking);
		c->s_main = ss.st[k];
		c->owns_main = false;
	} else if (c->service && sp && atoi(sp) != 0) {      /* (measured: 20 000 reads map in 3.07 s with it against 2.33 s without, search calls 7.0 against 3.4 ms -- off unless asked for) */
		int prio_lo = 0, prio_hi = 0;
		(void) hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);     /* numerically lower = higher priority */
		e = hipStreamCreateWithPriority(&c->s_main, hipStreamNonBlocking, prio_hi);
	} else {
		e = hipStreamCreateWithFlags(&c->s_main, hipStreamNonBlocking);
	}
	if (e != hipSuccess) {
		set_err("hipStreamCreate failed: %s", hipGetErrorString(e));
		cvx_destroy(c);
		return CVX_ERR_HIP;
	}
	*out = c;
	return CVX_OK;
	ABI_GUARD_END
}

int cvx_handle_pen_table(cvx_handle h) {
	ABI_GUARD_BEGIN
	if (!h) { set_err("cvx_handle_pen_table: NULL handle"); return CVX_ERR_ARG; }
	return h->tune_pen_table ? 1 : 0;
	ABI_GUARD_END
}

void cvx_destroy(cvx_handle h) {
	ABI_GUARD_BEGIN
	if (!h) return;
	(void) hipSetDevice(h->device);
	(void) hipDeviceSynchronize();
	g_deferred.drain();
	if (h->s_main && h->owns_main) (void) hipStreamDestroy(h->s_main);      /* (a service handle's stream belongs to the process) */
	if (h->s_post) (void) hipStreamDestroy(h->s_post);
	if (h->s_text) (void) hipStreamDestroy(h->s_text);
	if (h->s_io) (void) hipStreamDestroy(h->s_io);
	for (auto &a : h->aux) if (a) (void) hipStreamDestroy(a);
	if (h->s_main2) (void) hipStreamDestroy(h->s_main2);
	if (h->s_post2) (void) hipStreamDestroy(h->s_post2);
	for (auto &a : h->aux2) if (a) (void) hipStreamDestroy(a);
	if (h->s_tail) (void) hipStreamDestroy(h->s_tail);
	for (cvx_batch_s *b : h->pool) delete b;
	h->pool.clear();
	/* jobs the caller never released (submitted, maybe waited for): the device is idle, free them too --
	 * their handles are dead from here on, like everything else that belonged to this context */
	for (cvx_batch_s *b : h->live) delete b;
	h->live.clear();
	h->pending.clear();
	h->climbing.clear();
	score_state_free(h->score);
	search_state_free(h->search);
	delete h;
	ABI_GUARD_END_VOID
}

/* ------------------------------------------------------------------ page-locked arenas */

int cvx_host_alloc(uint64_t bytes, void **out) {
	ABI_GUARD_BEGIN
	if (!out) { set_err("cvx_host_alloc: NULL argument"); return CVX_ERR_ARG; }
	*out = nullptr;
	int ndev = 0;
	if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { (void) hipGetLastError(); set_err("cvx_host_alloc: no HIP device"); return CVX_ERR_NO_DEVICE; }
	void *p = nullptr;
	const size_t want = (size_t) bytes + 4096;        /* slack: block copies are rounded up to whole dwords */
	hipError_t e = hipHostMalloc(&p, want, hipHostMallocPortable);
	if (e != hipSuccess) { (void) hipGetLastError(); set_err("hipHostMalloc(%zu bytes) failed: %s", want, hipGetErrorString(e)); return CVX_ERR_OOM; }
	{
		std::lock_guard<std::mutex> lk(g_pin_mtx);
		g_pin_blocks.emplace_back(static_cast<const char *>(p), want);
	}
	*out = p;
	return CVX_OK;
	ABI_GUARD_END
}

void cvx_host_free(void *p) {
	ABI_GUARD_BEGIN
	if (!p) return;
	{
		std::lock_guard<std::mutex> lk(g_pin_mtx);
		for (size_t i = 0; i < g_pin_blocks.size(); ++i)
			if (g_pin_blocks[i].first == p) { g_pin_blocks.erase(g_pin_blocks.begin() + (long) i); break; }
	}
	(void) hipHostFree(p);
	ABI_GUARD_END_VOID
}

}  /* extern "C" */
