/*
 * cvx_rt.h -- what the files of the host runtime share (cvx_runtime.cpp and the cvx_rt_*.cpp of its subsystems): the HIP error
 * macro, the grow-only device and page-locked buffers, the handle, job and genome structures -- a job's two result stages
 * (JobRegions, JobText: cvx_rt_stages.cpp) and the definition of a fresh job (cvx_batch_s::begin_job) among them -- and the helpers
 * more than one of those files calls.  What only the pipeline (cvx_rt_align.cpp) and the ladder jobs (cvx_rt_ladder.cpp) call of
 * each other: cvx_rt_align.h.  Internal; the public boundary is include/cvx_align.h.
 */
#ifndef CVX_RT_H
#define CVX_RT_H

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "cvx_align.h"
#include "cvx_buf.h"
#include "cvx_host_logic.h"
#include "cvx_inv_checks_dev.h"
#include "cvx_launch.h"
#include "cvx_nm_regions.h"
#include "cvx_job_text.h"
#include "cvx_rt_err.h"
#include "cvx_types.h"

using namespace cvx;      /* (only the runtime's own files include this header, and all of them work in namespace cvx) */

#define HIP_TRY(expr)                                                              \
	do {                                                                           \
		hipError_t e_ = (expr);                                                    \
		if (e_ != hipSuccess) {                                                    \
			set_err("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
			return (e_ == hipErrorOutOfMemory) ? CVX_ERR_OOM : CVX_ERR_HIP;        \
		}                                                                          \
	} while (0)

/* the same for an entry that reports every HIP failure after its allocations as CVX_ERR_HIP, under its own name */
#define HIP_TRY_IN(who, expr)                                                      \
	do {                                                                           \
		hipError_t e_ = (expr);                                                    \
		if (e_ != hipSuccess) {                                                    \
			set_err("%s: %s", who, hipGetErrorString(e_));                         \
			return CVX_ERR_HIP;                                                    \
		}                                                                          \
	} while (0)

struct cvx_search_state;         /* cvx_rt_search.cpp */
struct cvx_score_state;          /* cvx_rt_score.cpp */

namespace cvx {

/* Buffers that grow while a handle streams jobs of changing size (ngmlr's pipeline: launches of 50 to 4 000 tiles on five job
 * slots).  Two things made cvx_submit take 15-50 ms per call there (profiles/r06_e2e_submit_trace.txt, `upload stage`):
 *   - hipFree / hipHostFree wait for everything in flight on the device.  An outgrown block is therefore not freed on the spot
 *     but parked (defer_release) and given back when its handle has nothing in flight, or at cvx_destroy;
 *   - every slot climbed to the size of the largest launch by itself.  Slots of one handle share a high-water mark per buffer
 *     (bind): the first growth of a slot goes straight to the largest capacity any of them has had. */
struct DeferredFrees {
	std::mutex mtx;
	std::vector<void *> dev, host;
	void drain() {
		std::vector<void *> d, h;
		{
			std::lock_guard<std::mutex> lk(mtx);
			d.swap(dev);
			h.swap(host);
		}
		for (void *p : d) (void) hipFree(p);
		for (void *p : h) (void) hipHostFree(p);
	}
	bool empty() { std::lock_guard<std::mutex> lk(mtx); return dev.empty() && host.empty(); }
};
extern DeferredFrees g_deferred;

/* the two memories of cvx_buf.h's buffer: an outgrown block is parked in g_deferred, a buffer that dies frees its block at once */
struct DevMem {
	static constexpr size_t kSlack = 64;
	static constexpr const char *kName = "hipMalloc";
	static const char *alloc(void **p, size_t bytes) { const hipError_t e = hipMalloc(p, bytes); return e == hipSuccess ? nullptr : hipGetErrorString(e); }
	static void free(void *p) { (void) hipFree(p); }
	static void park(void *p) { std::lock_guard<std::mutex> lk(g_deferred.mtx); g_deferred.dev.push_back(p); }
	static void drain() { (void) hipGetLastError(); g_deferred.drain(); }      /* (a failed hipMalloc's error is cleared where a retry follows, and only there) */
};
struct PinMem {
	static constexpr size_t kSlack = 4096;
	static constexpr const char *kName = "hipHostMalloc";
	static const char *alloc(void **p, size_t bytes) {
		const hipError_t e = hipHostMalloc(p, bytes, hipHostMallocDefault);
		if (e == hipSuccess) return nullptr;
		(void) hipGetLastError();
		return hipGetErrorString(e);
	}
	static void free(void *p) { (void) hipHostFree(p); }
	static void park(void *p) { std::lock_guard<std::mutex> lk(g_deferred.mtx); g_deferred.host.push_back(p); }
	static void drain() { g_deferred.drain(); }
};
template <typename T> using DevBuf = Buf<T, DevMem>;      /* cap in elements */
using PinBuf = Buf<void, PinMem>;                         /* grow-only page-locked host buffer, cap in bytes */

/* an event made when first asked for, with the flags of its site, and destroyed with its owner */
struct Event {
	hipEvent_t e = nullptr;
	Event() = default;
	Event(const Event &) = delete;
	Event &operator=(const Event &) = delete;
	Event(Event &&o) noexcept : e(o.e) { o.e = nullptr; }
	Event &operator=(Event &&o) noexcept { if (this != &o) { reset(); e = o.e; o.e = nullptr; } return *this; }
	~Event() { reset(); }
	hipError_t make(unsigned flags = hipEventDefault) { return e ? hipSuccess : hipEventCreateWithFlags(&e, flags); }
	void reset() { if (e) (void) hipEventDestroy(e); e = nullptr; }
	operator hipEvent_t() const { return e; }
};

bool in_pinned_block(const void *p, uint64_t bytes);      /* [p, p + bytes) lies inside one block of cvx_host_alloc */
float ev_ms(hipEvent_t a, hipEvent_t b);
int event_fired(hipEvent_t e);      /* 1: fired; 0: not yet (the query's error is cleared); -1: the query failed (set_err done) */
int ensure_streams(cvx_context *c);
/* the per-handle state of the search and of the scoring, owned by their files (cvx_destroy) */
void search_state_free(cvx_search_state *ss);
float search_kernel_ms(const cvx_search_state *ss);      /* of the handle's last search (cvx_stage_kernel_ms) */
float search_score_kernel_ms(const cvx_search_state *ss);      /* the plan + stage + score kernels of its last cvx_search_score_arena */
void score_state_free(cvx_score_state *ss);

}  // namespace cvx

/* Four streams per handle (io, main, post, one aux) and not more: the ROCm runtime multiplexes the streams of a process onto
 * (by default) four hardware queues, and two streams that land on the same queue serialise --
 * measured: with seven streams the 18-tile M = 4 launch ran alone for 11 ms in front of the
 * 24 558-tile M = 3 launch instead of beside it. */
static const int kAuxStreams = 2;      /* (round 5: a batch has up to four fill classes -- chained, gangs, M = 4, M = 3 -- and each wants a stream of its own) */

/* the events of one fill launch: its start, two-phase pass done, exact pass done, the class's own backtrack done; and of the tail of a
 * split launch (FillLaunch::tail_count, recorded on the handle's low-priority stream): its start, two-phase pass done, exact pass done */
enum LaunchEvent { kLevStart = 0, kLevTwoPhase = 1, kLevExact = 2, kLevWalked = 3, kLevTailStart = 4, kLevTailTwoPhase = 5, kLevTailExact = 6, kLevPerLaunch = 7 };

enum BatchState { kFailed = -1, kEmpty = 0, kUploaded = 1, kPlanned = 2, kComputed = 3, kFinished = 4 };

struct LadderState;              /* below: what the first rung of a ladder job (cvx_submit_ladder) carries */
void ladder_drop(struct cvx_batch_s *root);      /* frees it and the later rungs' batches (cvx_rt_ladder.cpp); the device is idle, or has nothing of them queued */

/* The two result stages a handle can run behind every job's compaction (cvx_rt_stages.cpp: what queues them, and the getters that
 * hand their data out).  Both write into an arena sized by an estimate, the way finalize and compact treat the dense ops, and both
 * have one life, a call per step from the pipeline:
 *   queue       (stage_compute) the first pass on the batch's stream, with no host step in front: sizes, the offset scan, the write
 *               into the estimated arena; the offsets -- the total and the capacity the write ran with behind them -- and the per-tile
 *               records travel in copies queued here, in front of the event stage_results waits for
 *   set_empty   (stage_compute, a job without tiles) one offset, 0
 *   take_total  (stage_results) the total, from the slot behind the n offsets
 *   fetch       (stage_ops) the total exceeds the capacity: the arena grows and the write alone runs again on the batch's stream,
 *               waited for; then the arena to the host on `io`, in front of the dense ops and under their wait
 * reset() is the stage's part of cvx_batch_s::begin_run.  Buffers of their own, so that a stage of the finished job on the text
 * stream (cvx_job_nm_regions, cvx_job_text) never meets them. */

/* the low-identity regions of the job's tiles (a CVX_CREATE_NM_REGIONS handle; cvx_job_regions), and riding with them the inversion
 * check of every region (a CVX_CREATE_INV_CHECKS handle, a job submitted with a genome: inv_checks_kernel behind the finder's write;
 * cvx_job_checks): one record per region of the arena, to the host with the regions */
struct JobRegions {
	DevBuf<unsigned long long> d_off;    /* counts[n], offsets[n], the total, the capacity the write ran with */
	DevBuf<NmOpen> d_open;
	DevBuf<NmRegion> d_stage, d_reg;
	DevBuf<InvCheck> d_chk;
	PinBuf h_off, h_open, h_reg, h_chk;  /* offsets[n] + total + capacity and the end states arrive with the result records, the regions and checks with the dense ops */
	bool on = false;                 /* this run of the compute stage queued the finder */
	bool checks_on = false;          /* ... and the checks */
	uint64_t cap = 0, total = 0;     /* regions the arena holds; regions of the job (after stage_results) */
	int rewrites = 0;                /* times the write ran again over a larger arena (stage_ops) */
	const uint8_t *bin = nullptr;    /* the genome the job was submitted with (its owner keeps it alive until cvx_wait), NULL: none, or no flag */
	uint64_t L = 0;                  /* its GetConcatRefLen() */

	void reset() { on = checks_on = false; cap = total = 0; rewrites = 0; }
	int queue(struct cvx_batch_s *b, hipStream_t st, bool rewrite = false);
	int set_empty();
	void take_total(int n) { if (on) total = h_off.as<unsigned long long>()[(size_t) n]; }
	int fetch(struct cvx_context *h, struct cvx_batch_s *b);
};

/* the device text stage over the job's op lists and its sequences in HBM, external clips zero (a CVX_CREATE_JOB_TEXT handle;
 * cvx_job_texts) */
struct JobText {
	DevBuf<TextRec> d_rec;
	DevBuf<unsigned long long> d_off;    /* lengths[n], offsets[n], the total, the capacity the write ran with */
	DevBuf<uint8_t> d_text;
	PinBuf h_rec, h_off, h_text;         /* records and offsets[n] + total + capacity arrive with the result records, the strings with the dense ops */
	bool on = false;                 /* this run of the compute stage queued the text stage */
	uint64_t cap = 0, total = 0;     /* bytes the arena holds; bytes of the job's text (after stage_results) */
	int rewrites = 0;                /* times the write ran again over a larger arena (stage_ops) */

	void reset() { on = false; cap = total = 0; rewrites = 0; }
	int queue(struct cvx_batch_s *b, hipStream_t st, bool rewrite = false, uint64_t tune = 0);
	int set_empty();
	void take_total(int n, bool twin);
	int fetch(struct cvx_context *h, struct cvx_batch_s *b);
};

struct cvx_batch_s {
	int n = 0;
	int state = kEmpty;
	bool in_flight = false;          /* submitted through the streaming API and not yet released */
	hipStream_t s_run = nullptr;     /* the `main` stream of the set that carried this batch's kernels */
	int fail_rc = CVX_OK;            /* state == kFailed: what went wrong with THIS job (cvx_wait returns it) */
	std::string fail_msg;
	uint64_t seq_total = 0, n_rows = 0, n_rowsx = 0;
	uint64_t zero_copy_bytes = 0;    /* sequence bytes of the last upload that travelled straight from the caller's page-locked arena */
	uint64_t ops_total = 0;          /* valid after the compute stage has been waited for */
	uint64_t dense_cap = 0;
	bool have_ops = false;           /* dense ops are in h_ops */

	/* host side, page-locked */
	PinBuf h_zero;                   /* zeros for the pads around blocks that travel straight from the caller's arena */
	size_t zero_cap = 0;
	PinBuf h_seq, h_delta, h_rsrc, h_rowsx, h_tin;     /* upload staging (owned by the batch: no wait before reuse by another batch):
	                                                    * sequences, one step byte per corridor row, RowSrc[n], rows that need the verbatim form */
	std::vector<RowDesc> chain_rows;                   /* scratch: expanded rows of a tile being chained */
	PinBuf h_plan;                   /* TilePlan[n] */
	PinBuf h_trun, h_tout, h_lists, h_goff;   /* what the host planning produces */
	PinBuf h_res;                    /* ResultRec[n] + BatchSummary */
	PinBuf h_ops;                    /* dense ops */

	DevBuf<uint8_t> d_seq;
	DevBuf<RowDesc> d_rows;          /* the expanded rows arena (expand_rows_kernel) */
	DevBuf<uint8_t> d_delta;
	DevBuf<RowSrc> d_rsrc;
	DevBuf<RowDesc> d_rowsx;
	DevBuf<TileIn> d_tin;
	DevBuf<TilePlan> d_plan;
	DevBuf<TileRun> d_trun;
	DevBuf<TileOut> d_tout;
	DevBuf<uint32_t> d_dirs;
	DevBuf<int32_t> d_regions;
	DevBuf<int32_t> d_lists;
	DevBuf<int32_t> d_counters;
	DevBuf<uint64_t> d_dstoff;
	DevBuf<uint32_t> d_dense;
	DevBuf<uint8_t> d_res;           /* ResultRec[n] + BatchSummary */
	DevBuf<uint8_t> d_gscratch;      /* slot state of tiles taken by the catch-all kernel */
	DevBuf<uint64_t> d_gscratch_off;
	/* chained tiles (row blocks) */
	/* device-side text stage (cvx_job_text) */
	PinBuf h_ext, h_trec, h_toff, h_text;
	DevBuf<int32_t> d_ext;
	DevBuf<TextRec> d_trec;
	DevBuf<unsigned long long> d_tlen;   /* lengths, offsets, total */
	DevBuf<uint8_t> d_text;
	bool text_done = false;          /* d_trec holds this job's text records (cvx_job_text ran) */
	DevBuf<unsigned long long> d_nmoff;  /* nmPerPosition: entry counts, offsets, total of the requested tile range */
	DevBuf<int32_t> d_nm;            /* ... and the triples */
	PinBuf h_nmoff;
	PinBuf h_nm;                     /* the triples on the host (cvx_job_nm_profile_resident) */
	Event ev_nm0, ev_nm1;
	DevBuf<unsigned long long> d_nmroff; /* the profile's low-identity regions (cvx_job_nm_regions): counts, offsets, total of the tile range */
	DevBuf<NmOpen> d_nmopen;         /* ... the state every tile's scan ends in */
	DevBuf<NmRegion> d_nmstage;      /* ... kNmStage regions per tile as the first pass found them */
	DevBuf<NmRegion> d_nmreg;        /* ... and the regions, dense */
	PinBuf h_nmroff, h_nmopen;
	PinBuf h_nmreg;                  /* the regions on the host: what cvx_job_nm_regions hands out */
	JobRegions jr;                   /* the same regions, and their inversion checks, found with the job's results */
	JobText jt;                      /* the text stage run with the job's results */
	PinBuf h_win;                   /* WindowDesc[n]: reference windows decoded on the device (cvx_submit_windows) */
	PinBuf h_refs;                   /* ... and the decoded windows back on the host (cvx_job_window_refs): the reference part of d_seq */
	uint64_t refs_base = 0;          /* offset of that part in the sequence arena */
	bool have_refs = false;
	DevBuf<WindowDesc> d_win;
	PinBuf h_reads;                  /* the read block of cvx_submit_segments on its way up (a caller's block in page-locked memory travels as it is) */
	PinBuf h_segs;                   /* SegDesc[n] and the SegChunk table behind them (cvx_segments.h) */
	DevBuf<uint8_t> d_reads, d_segs;
	PinBuf h_chain;                  /* ChainTask[] of all chain classes, ChainBlk[], tile lists */
	DevBuf<uint8_t> d_chain;
	DevBuf<BoundaryRec> d_bnd;
	uint32_t bnd_epoch = 0;          /* tag of the records the latest launch wrote (0: buffer freshly zeroed) */
	DevBuf<ChainOut> d_chain_out;
	/* ladder jobs (cvx_submit_ladder): the job the caller holds is rung 1; every later rung is a batch of its own -- its own plan,
	 * lists, direction words, result block and ops -- that reads the sequences of rung 1 */
	LadderState *ladder = nullptr;   /* rung 1: the job's ladder */
	cvx_batch_s *ladder_root = nullptr;      /* a later rung: the rung 1 whose sequence arena it reads */
	DevBuf<int32_t> d_lhead;         /* a later rung: tiles that climbed to it, then the job tile of each (ladder_next_kernel) */
	PinBuf h_lhead;
	DevBuf<cvx_ladder> d_lad;        /* rung 1: cvx_ladder[n] as submitted */
	PinBuf h_lad;
	PinBuf h_lres, h_lops, h_lout;   /* rung 1: the job's answer merged by cvx_wait -- ResultRec[n], dense ops, cvx_ladder_result[n] */

	Event ev_bt0, ev_bt1;   /* fork / join of the long-read backtrack launch */
	Event ev_in;      /* upload + plan records on the host */
	Event ev_res;     /* result records on the host */
	Event ev_rec;     /* result records final on the device, dense ops compacted: in front of the job's regions / checks / text stages */
	Event ev[5];   /* timing: plan begin/end, fills done, all done, fills may start */
	std::vector<Event> lev;     /* kLevPerLaunch events per fill launch (LaunchEvent) */
	std::vector<cvx_launch_info> launches;
	std::vector<int> launch_tail;    /* per fill launch: tiles of its tail (0: not split, its tail events were not recorded) */
	cvx_timing timing;

	const TileIn *tin() const { return h_tin.as<TileIn>(); }
	const TilePlan *plan() const { return h_plan.as<TilePlan>(); }
	const ResultRec *res() const { return h_res.as<ResultRec>(); }
	const BatchSummary *summary() const { return reinterpret_cast<const BatchSummary *>(h_res.as<uint8_t>() + (size_t) n * sizeof(ResultRec)); }

	/* the buffers whose size follows the job's tile count or cells: the same buffer of every slot of a handle shares one mark */
	static const int kSharedMarks = 40;
	void bind(size_t *marks) {
		int k = 0;
		PinBuf *pins[] = { &h_seq, &h_delta, &h_rsrc, &h_tin, &h_plan, &h_trun, &h_tout, &h_lists, &h_res, &h_ops, &h_chain };
		for (PinBuf *b_ : pins) b_->hwm = &marks[k++];
		d_seq.hwm = &marks[k++]; d_rows.hwm = &marks[k++]; d_delta.hwm = &marks[k++]; d_rsrc.hwm = &marks[k++]; d_tin.hwm = &marks[k++];
		d_plan.hwm = &marks[k++]; d_trun.hwm = &marks[k++]; d_tout.hwm = &marks[k++]; d_dirs.hwm = &marks[k++]; d_regions.hwm = &marks[k++];
		d_lists.hwm = &marks[k++]; d_dstoff.hwm = &marks[k++]; d_dense.hwm = &marks[k++]; d_res.hwm = &marks[k++];
		d_chain.hwm = &marks[k++]; d_bnd.hwm = &marks[k++]; d_chain_out.hwm = &marks[k++];
		/* the big buffers of the text stage (strings, profile triples: 125 kB per 10 kb alignment); written by the one thread that
		 * runs a handle's text stages -- never the thread that submits, and these entries are nobody else's */
		h_text.hwm = &marks[k++]; h_nm.hwm = &marks[k++]; d_text.hwm = &marks[k++]; d_nm.hwm = &marks[k++];
		h_reads.hwm = &marks[k++]; h_segs.hwm = &marks[k++]; d_reads.hwm = &marks[k++]; d_segs.hwm = &marks[k++];
		static_assert(11 + 17 + 4 + 4 <= kSharedMarks, "marks");
	}
	int make_events() {
		for (Event *e : { &ev_in, &ev_res, &ev_rec, &ev_bt0, &ev_bt1 }) HIP_TRY(e->make(hipEventDisableTiming));
		for (Event &e : ev) HIP_TRY(e.make());
		return CVX_OK;
	}
	/* the sequence arena the batch's kernels read: a later rung of a ladder job reads rung 1's sequences where they lie */
	const uint8_t *seq() const { return ladder_root ? ladder_root->d_seq.p : d_seq.p; }

	/* What a run of the compute stage starts from.  Apart from begin_job: stage_compute itself, since a staged batch can be run
	 * again without a new upload (cvx_batch_upload, then cvx_batch_run twice). */
	void begin_run() {
		launches.clear();
		launch_tail.clear();
		ops_total = 0;
		have_ops = false;
		jr.reset();
		jt.reset();
	}
	/* THE definition of a fresh job: every per-job member in the state a job starts from.  For a slot that goes back to the pool
	 * (recycle_batch), one that takes a job's upload (stage_upload) and one that becomes a later rung of a ladder job
	 * (ladder_queue_next); each then sets what is particular to it.  A failed job's fail_rc / fail_msg live until cvx_job_release:
	 * none of the three is reached with a job the caller still holds (the last two take their slot from acquire_batch).
	 * Not here, on purpose: what belongs to the slot's buffers and outlives a job (zero_cap, bnd_epoch, the d_counters' once-only
	 * clearing, the capacities), and the links between the batches of a ladder job (ladder, ladder_root), which
	 * ladder_release / ladder_queue_next cut and tie. */
	void begin_job() {
		begin_run();
		n = 0;
		state = kEmpty;
		in_flight = false;
		fail_rc = CVX_OK;
		fail_msg.clear();
		seq_total = n_rows = n_rowsx = 0;
		zero_copy_bytes = 0;
		have_refs = false;
		text_done = false;
		jr.bin = nullptr;
		jr.L = 0;
		memset(&timing, 0, sizeof(timing));
	}
	~cvx_batch_s() { if (ladder) ladder_drop(this); }      /* a ladder job's later rungs go with it; the buffers and events free themselves */
};

/* The ladder of one job.  Where a tile's reported record and ops are kept: every rung's batch keeps its own result block and
 * dense ops in its own page-locked memory, as any job does, and cvx_wait merges them on the host -- per tile the record of the
 * last rung it took part in, its ops copied into one arena in tile order. */
struct LadderState {
	std::vector<cvx_batch_s *> rungs;      /* rungs[r]: the batch of rung r + 1; rungs[0] is the job itself */
	cvx_batch_s *next = nullptr;     /* the rung whose list and plan are on their way back (its ev_in says when) */
	bool done = false;               /* no further rung will be queued */
	bool merged = false;             /* the job's h_lres / h_lops / h_lout hold its answer */
	int max_rungs = 0;               /* the longest ladder any tile of the job has (host rule at submit) */
	uint64_t ops_total = 0;          /* ops of the merged arena */
	uint64_t seq_bytes_after_submit = 0;   /* sequence bytes queued for upload, copy or decode by a later rung: nothing adds to it */
	cvx_timing timing;               /* summed over the rungs */
	std::vector<cvx_launch_info> launches; /* the rungs' launches, in order */
	/* a handle with CVX_CREATE_NM_REGIONS / _INV_CHECKS / _JOB_TEXT (cvx_submit_ladder_ex): every rung runs those stages behind its
	 * own compaction, and cvx_wait merges what they brought back -- per tile the reporting rung's, in tile order, offsets rebased
	 * (cvx_ladder_merge.h).  What cvx_job_regions / _checks / _texts hand out for the job, in an ordinary job's layout */
	std::vector<uint64_t> jr_off;          /* region_off[n + 1] */
	std::vector<NmRegion> jr_reg;
	std::vector<NmOpen> jr_open;
	std::vector<InvCheck> jr_chk;          /* parallel to jr_reg (a job with a genome on a checks handle) */
	int jr_rewrites = 0;                   /* summed over the rungs */
	std::vector<TextRec> jt_rec;
	std::vector<uint64_t> jt_off;          /* text_off[n + 1] */
	std::vector<char> jt_text;
	int jt_rewrites = 0;
};

struct cvx_context {
	int device = 0;
	hipStream_t s_io = nullptr;      /* uploads, plan, downloads (high priority: its short kernels and copies
	                                  * must not queue behind the fill's workgroups) */
	hipStream_t s_main = nullptr;    /* forward fills (and the small input copies in front of them) */
	hipStream_t s_text = nullptr;    /* the text stage of FINISHED jobs (cvx_job_text, nm profile): its own stream, never queued behind the
	                                  * fills of the batches that follow */
	hipStream_t s_post = nullptr;    /* backtrack, finalize, compaction, result download: runs beside the NEXT batch's fill */
	hipStream_t aux[kAuxStreams] = {nullptr};  /* concurrent fill classes */
	hipStream_t s_tail = nullptr;    /* the tails of split fill classes and nothing else (stage_compute): the device's lowest queue priority, so that a tail
	                                  * is dispatched where its head leaves wave slots free.  Stays null, and no class is split, when the device has no
	                                  * priority below the default */
	bool service = false;                      /* cvx_create_ex(CVX_CREATE_SERVICE): short search / scoring / decode calls only */
	bool owns_main = true;                     /* false: s_main is one of the process's shared service streams */
	std::mutex streams_mtx;                    /* ensure_streams */
	std::atomic<bool> streams_ready{false};    /* ensure_streams: the whole set exists (stored last, with release: read without the mutex) */
	/* a second set (main, post, aux) for small streaming jobs (experiment, off by default: see single_lane): the jobs of a
	 * batching driver (tens of tiles each) are latency-bound chains of small kernels on an otherwise empty device;
	 * consecutive ones can alternate between the two sets */
	hipStream_t s_main2 = nullptr, s_post2 = nullptr, aux2[kAuxStreams] = {nullptr};
	unsigned small_jobs = 0;         /* small streaming jobs queued so far (their parity picks the set) */
	ScoreParams sp;
	uint64_t max_matrix_mb = 10000;
	int num_cus = 256;
	int pack_threads = 16;
	int tune_min_slots = 0;   /* tuning knob (env CVX_TUNE_MIN_M): smallest M*NW a tile may use */
	int tune_late_min = kLateMinGroups;  /* test knob (env CVX_TUNE_LATE_MIN): groups of the exactly tracked tail (huge: exact everywhere) */
	int tune_late_shift = kLateShift;    /* tuning knob (env CVX_TUNE_LATE_SHIFT): the exactly tracked tail is groups >> this (at least tune_late_min) */
	int tune_max_slots = 0;   /* tuning knob (env CVX_TUNE_MAX_M): largest whole-tile ring class; wider tiles are chained */
	int tune_long_need = 0;   /* tuning knob (env CVX_TUNE_LONG_NEED): see PlanTuning */
	int tune_gang_prio = 0;   /* tuning knob (env CVX_TUNE_GANG_PRIO = 0 / 1): gang tiles at raised wave priority (measured: 26.9 against 24.0 ms, a loss) */
	int tune_gangs = 0;       /* tuning knob (env CVX_TUNE_GANGS = 0 / 1): rings of 384 / 576 slots as gangs of two / three waves instead of chained row
	                           * blocks.  Off: measured, the gangs lose -- the ONT mix's retry tiles alone 24.0 ms against 21.4 ms chained, the whole mix
	                           * equal within noise (profiles/r05_gang_ab.txt): short tiles leave a 576-slot ring idle through its ramps (60 % slot use
	                           * against 85 % for 64-row blocks), which eats the 1.6 x cheaper cell update, and three waves in lock step on three SIMDs
	                           * wait for the slowest of them every step */
	int tune_long_steps = 0, tune_small_batch = 0;   /* tuning knobs (env CVX_TUNE_LONG_STEPS / CVX_TUNE_SMALL_BATCH): see PlanTuning */
	bool single_lane = true;  /* experiment (env CVX_TUNE_TWO_LANES=1 clears it): small streaming jobs alternate between two stream sets.
	                           * Measured with the batching dispatcher at four launches in flight: no gain -- 20 000 reads 25.1 s against
	                           * 21.2 s, launches get smaller and each still lasts as long as its slowest tile -- so it stays off. */
	int tune_exact_steps = kExactDirectSteps;   /* tuning knob (env CVX_TUNE_EXACT_STEPS, 0 = off): tiles of this many steps go straight to the exact fill */
	int tune_wide_prio = 1;   /* tuning knob (env CVX_TUNE_WIDE_PRIO = 0 / 1 / 2: off, priority 1, priority 2): the widest ring class of a batch of several one priority notch up */
	int tune_chain_prio = -1; /* tuning knob (env CVX_TUNE_CHAIN_PRIO = 0 / 1): wave priority of chained blocks; -1 = the default (raised) */
	int tune_chain_lds_kb = 48; /* tuning knob (env CVX_TUNE_CHAIN_LDS_KB): LDS per CU the residency cap of a chained class may hold while ring classes
	                           * of the same batch run beside it (0 = no limit: round 5's rule) */
	int tune_chain_m = 0;     /* test knob (env CVX_TUNE_CHAIN_M): row-block height class (1, 2, 4) of chained tiles */
	int tune_force_wrap = 0;  /* test knob (env CVX_TUNE_FORCE_WRAP16): route every tile to the int16-run kernels */
	int tune_pen_table = 1;   /* tuning knob (env CVX_TUNE_PEN_TABLE = 0 / 1): convex penalty from the LDS table in the two-phase float-score fills */
	int test_fail_compute = 0; /* test knob (env CVX_TUNE_FAIL_COMPUTE = k): the k-th compute stage of this handle fails (error-path tests) */
	int bt_group = 0;          /* lanes per tile in the backtrack: 0 = auto (by the number of tiles walked together: 64 / 32 / 16 / 8, and 32 for
	                            * the much-longer-than-average reads of a bulk walked at 8 or 16), 8 / 16 / 32 = that many for all, 64 = the
	                            * one-wave-per-tile walk, -1 = round 4's rule (64 below 4 096 tiles, else 8 + 32) (env CVX_TUNE_BT_GROUP) */
	int tail_split = cvx::kTailAuto;   /* tuning knob (env CVX_TUNE_TAIL_SPLIT): 0 = no fill class is split, N > 0 = every whole-tile class with more than N
	                            * two-phase tiles gets a tail of N (test knob), unset = by the class's resident waves (tail_split, cvx_host_logic.h) */
	float tail_rounds = 1.0f;  /* the automatic rule's tail in resident rounds of the class (env CVX_TUNE_TAIL_ROUNDS) */
	int tail_gate = 1;         /* experiment (env CVX_TUNE_TAIL_GATE): 1 = the tail waits for the head's start event, 0 = for the batch's inputs only */
	int tail_trace = 0;        /* env CVX_TUNE_TAIL_TRACE = 1: one stderr line per split launch of a finished batch, from its events */
	int fill_waves[cvx::kNumClasses * 2] = {0};   /* resident waves per SIMD of each whole-tile class's two-phase fill as the runtime reports the kernel's
	                            * occupancy (0: not asked yet, -1: unknown); filled by stage_compute for the classes a batch uses */
	bool bt_per_class = true;  /* tuning knob (env CVX_TUNE_BT_PER_CLASS = 0 clears it): a batch of several fill classes walks each class behind its own fill (build_schedule) */
	bool overlap_post = false; /* tuning knob (env CVX_TUNE_OVERLAP_POST): backtrack/finalize/compaction of batch k on their own stream, beside the fills of batch k+1 */
	bool job_text = false;    /* cvx_create_ex(CVX_CREATE_JOB_TEXT): every job runs the device text stage behind its compaction (cvx_job_texts) */
	uint64_t tune_job_text_cap = 0; /* tuning knob (env CVX_TUNE_JOB_TEXT_CAP, bytes; 0: job_text_first_capacity's rule): the capacity a job's first text write runs with */
	bool nm_regions = false;  /* cvx_create_ex(CVX_CREATE_NM_REGIONS): every job finds the low-identity regions of its tiles behind its compaction (cvx_job_regions) */
	bool inv_checks = false;  /* cvx_create_ex(CVX_CREATE_INV_CHECKS): a job submitted with a genome scores the inversion check of every region behind the finder (cvx_job_checks) */
	bool scalar_twin = false; /* cvx_create_ex(CVX_CREATE_SCALAR_TWIN): the semantics of Convex::ConvexAlign (cvx_host_logic.h, fill_semantics) */
	bool force_generic = false; /* every tile to the catch-all kernel: sse_variant, or a twin handle whose scoring lacks the rings' sign structure */
	bool sse_variant = false; /* scoring outside the regime where the reference's SSE path equals the scalar recurrence:
	                           * every tile goes to the catch-all kernel's SSE-variant instantiation */
	/* freed batches keep their device arenas and pinned staging and wait here for the next upload
	 * (at most kPoolBatches): hipMalloc / hipFree of multi-GB arenas per call are slow, and hipFree
	 * synchronises the whole device, which would serialise handles that work side by side */
	size_t marks[cvx_batch_s::kSharedMarks] = {0};   /* high-water marks of the streaming slots' buffers (cvx_batch_s::bind) */
	std::vector<cvx_batch_s *> pool;
	std::vector<cvx_batch_s *> pending;      /* streaming jobs whose compute stage is not queued yet */
	std::vector<cvx_batch_s *> live;         /* every streaming job the caller has not released yet (cvx_destroy frees what is left) */
	std::vector<cvx_batch_s *> climbing;     /* ladder jobs whose first rung is queued and whose ladder is not done (pump advances them) */
	float segments_kernel_ms = 0.0f;   /* stage_segments_kernel of the last cvx_stage_segments (cvx_stage_kernel_ms) */
	float decode_kernel_ms = 0.0f;     /* decode_windows_kernel of the last cvx_genome_decode (cvx_stage_kernel_ms) */
	bool score_no_diag = false;   /* test knob (env CVX_TUNE_SCORE_NO_DIAG): always the row-by-row kernels */
	struct cvx_score_state *score = nullptr;   /* sub-read scoring (cvx_score_batch, cvx_score_submit): jobs kept for reuse once waited for */
	struct cvx_search_state *search = nullptr;   /* candidate search (cvx_search_batch): persistent staging and device buffers */
};

/* the job off the handle's lists (any of the three it is on); h may be NULL: a batch that is freed without its handle */
enum JobList { kListPending = 1, kListLive = 2, kListClimbing = 4 };
inline void unlist_job(cvx_context *h, const cvx_batch_s *b, int lists) {
	if (!h) return;
	std::vector<cvx_batch_s *> *const of[] = { &h->pending, &h->live, &h->climbing };      /* (in JobList's bit order) */
	for (int k = 0; k < 3; ++k) {
		const auto it = std::find(of[k]->begin(), of[k]->end(), b);
		if ((lists >> k & 1) && it != of[k]->end()) of[k]->erase(it);
	}
}

/* the buffers that hold one record per tile of a batch of n, for an uploaded job and for a later rung of a ladder job alike; the
 * counters with them, cleared once when they are allocated (why never again: stage_compute) */
inline int ensure_tile_records(cvx_batch_s *b, int n) {
	const size_t n1 = (size_t) std::max(n, 1);
	RC_TRY(b->h_rsrc.ensure(n1 * sizeof(RowSrc)));
	RC_TRY(b->h_tin.ensure(n1 * sizeof(TileIn)));
	RC_TRY(b->h_plan.ensure(n1 * sizeof(TilePlan)));
	RC_TRY(b->h_res.ensure(n1 * sizeof(ResultRec) + sizeof(BatchSummary)));
	RC_TRY(b->d_rsrc.ensure(n1));
	RC_TRY(b->d_tin.ensure(n1));
	RC_TRY(b->d_plan.ensure(n1));
	RC_TRY(b->d_trun.ensure(n1));
	RC_TRY(b->d_tout.ensure(n1));
	RC_TRY(b->d_dstoff.ensure(n1 + 2 * (size_t) finalize_blocks(n)));      /* ... + launch_finalize's per-block sums behind the n offsets */
	RC_TRY(b->d_lists.ensure(2 * n1));             /* fill lists + backtrack order */
	if (b->d_counters.cap < 64) {
		RC_TRY(b->d_counters.ensure(64));
		HIP_TRY(hipMemset(b->d_counters.p, 0, b->d_counters.cap * sizeof(int32_t)));
	}
	RC_TRY(b->d_res.ensure(n1 * sizeof(ResultRec) + sizeof(BatchSummary)));
	return CVX_OK;
}

/* the TextArgs of the text stage's kernels over a job's arenas; the caller adds the outputs of its own pass */
inline TextArgs job_text_args(const cvx_batch_s *b) {
	TextArgs a;
	memset(&a, 0, sizeof(a));
	a.seq = b->seq(); a.tin = b->d_tin.p; a.trun = b->d_trun.p; a.tout = b->d_tout.p; a.ops = b->d_regions.p;
	a.n_tiles = b->n;
	return a;
}

struct cvx_genome_s {            /* an encoded reference genome resident in HBM (cvx_genome.hip) */
	int device = 0;
	uint64_t n_nibbles = 0;
	int32_t n_starts = 0;
	DevBuf<uint8_t> d_bin;
	DevBuf<uint64_t> d_starts;
};

#endif
