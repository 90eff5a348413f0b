/*
 * cvx_rt_align.cpp -- the alignment job pipeline of libcvxalign.so (the handle and its streams: cvx_runtime.cpp).
 * A batch of tiles moves through four stages:
 *
 *   upload   host threads pack sequences + corridor rows into the batch's own pinned staging,
 *            piece by piece, each piece's DMA running under the packing of the next  (stream `io`)
 *   plan     plan_kernel, plan records back to pinned memory                          (stream `io`)
 *   compute  host: kernel class / arena offsets / LPT lists from the plan records;
 *            fill_ring_kernel per class (+ exact redo pass)                   (streams `main` + `aux`)
 *            backtrack_kernel, finalize_kernel (device-side prefix sums and result records),
 *            compact_ops_kernel, result records back to pinned memory               (stream `main`;
 *            optionally `post`, beside the next batch's fills: measured to gain nothing, see stage_compute)
 *   finish   dense ops back to pinned memory                                          (stream `io`)
 *
 * The streaming entry points (cvx_submit / cvx_wait / cvx_job_release) keep several batches in
 * flight on one handle: the upload and plan of batch k+1 and the download of batch k-1 run
 * under the kernels of batch k, and the only host waits are on events of work that was queued a
 * whole batch earlier.  The staged entry points (cvx_batch_*) and cvx_align_batch run the same
 * stages back to back.
 */
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "cvx_rt.h"

namespace {

static const size_t kPoolBatches = 8;      /* (4 until the text stage of a finished job got its own thread: a launch in the fill, one uploading, two in the text stage and those the workers still copy from) */

cvx_batch_s *acquire_batch(cvx_context *h) {
	if (!h->pool.empty()) {
		cvx_batch_s *b = h->pool.back();
		h->pool.pop_back();
		return b;
	}
	return new (std::nothrow) cvx_batch_s();
}

void recycle_batch(cvx_context *h, cvx_batch_s *b) {
	const bool failed = b->state == kFailed;
	b->state = kEmpty;
	b->in_flight = false;
	b->have_ops = false;
	b->have_refs = false;
	b->text_done = false;
	b->fail_rc = CVX_OK;
	b->fail_msg.clear();
	if (h) {
		auto it = std::find(h->live.begin(), h->live.end(), b);
		if (it != h->live.end()) h->live.erase(it);
	}
	/* (a job that failed half-way keeps nothing worth pooling: its arenas go back to the allocator) */
	if (h && !failed && h->pool.size() < kPoolBatches) { h->pool.push_back(b); return; }
	b->release();
	delete b;
}

/* something failed after work was queued: nothing may still be running on the arenas when they
 * go back to the allocator (or to the pool) */
void discard_batch(cvx_context *h, cvx_batch_s *b) {
	(void) hipDeviceSynchronize();
	if (h) {
		auto it = std::find(h->pending.begin(), h->pending.end(), b);
		if (it != h->pending.end()) h->pending.erase(it);
		it = std::find(h->live.begin(), h->live.end(), b);
		if (it != h->live.end()) h->live.erase(it);
	}
	b->release();
	delete b;
}

/* A streaming job whose stage failed stays alive (the caller still holds its handle) and remembers why:
 * cvx_wait on it returns this code, cvx_job_release frees it.  Whatever was queued for it is drained first. */
int fail_job(cvx_batch_s *b, int rc) {
	(void) hipDeviceSynchronize();
	b->state = kFailed;
	b->fail_rc = rc;
	b->fail_msg = g_err;
	return rc;
}

/* ---- stage 1: pack into pinned staging and copy to the device, piece by piece (stream `io`) */
int stage_upload(cvx_context *h, cvx_batch_s *b, int32_t n, const cvx_tile *tiles,
		const cvx_genome_s *genome = nullptr, const uint64_t *ref_position = nullptr) {
	RC_TRY(ensure_streams(h));
	UploadLayout L;
	std::vector<TileIn> tin;
	int bad = -1;
	const bool windows = genome != nullptr;
	const int lrc = upload_layout(n, tiles, tin, L, &bad, windows);
	if (lrc == kLayoutMalformed) { set_err("tile %d malformed", bad); return CVX_ERR_ARG; }
	if (lrc == kLayoutTooLarge) {
		set_err("%llu sequence bytes exceed one batch (4 GiB); split the batch", (unsigned long long) L.seq_total);
		return CVX_ERR_ARG;
	}
	b->n = n;
	b->state = kEmpty;
	b->have_ops = false;
	b->have_refs = false;
	b->text_done = false;
	b->ops_total = 0;
	b->seq_total = L.seq_total;
	b->n_rows = L.n_rows;
	memset(&b->timing, 0, sizeof(b->timing));
	RC_TRY(b->make_events());
	const size_t n1 = (size_t) std::max(n, 1);
	const size_t rows1 = (size_t) std::max<uint64_t>(L.arena_rows, 1);      /* closed-form corridors own no rows (RowView, cvx_types.h) */
	RC_TRY(b->h_delta.ensure((size_t) L.delta_total + 256));
	RC_TRY(b->h_rsrc.ensure(n1 * sizeof(RowSrc)));
	RC_TRY(b->d_delta.ensure((size_t) L.delta_total + 256));
	RC_TRY(b->d_rsrc.ensure(n1));
	RC_TRY(b->h_tin.ensure(n1 * sizeof(TileIn)));
	RC_TRY(b->h_plan.ensure(n1 * sizeof(TilePlan)));
	RC_TRY(b->h_res.ensure(n1 * sizeof(ResultRec) + sizeof(BatchSummary)));
	RC_TRY(b->d_seq.ensure((size_t) L.seq_total + 256));
	RC_TRY(b->d_rows.ensure(rows1));
	RC_TRY(b->d_tin.ensure(n1));
	RC_TRY(b->d_plan.ensure(n1));
	RC_TRY(b->d_trun.ensure(n1));
	RC_TRY(b->d_tout.ensure(n1));
	RC_TRY(b->d_dstoff.ensure(n1));
	RC_TRY(b->d_lists.ensure(2 * n1));             /* fill lists + backtrack order */
	if (b->d_counters.cap < 64) {
		RC_TRY(b->d_counters.ensure(64));
		HIP_TRY(hipMemset(b->d_counters.p, 0, b->d_counters.cap * sizeof(int32_t)));
	}
	RC_TRY(b->d_res.ensure(n1 * sizeof(ResultRec) + sizeof(BatchSummary)));
	if (n) memcpy(b->h_tin.p, tin.data(), (size_t) n * sizeof(TileIn));

	/* a block of sequences that already lies back to back in page-locked memory is not packed: the
	 * device pulls it out of the caller's arena (the job's staging then holds only what the host wrote) */
	const bool zc_qry = n > 0 && L.qry_contig && L.qry_bytes > 0 && in_pinned_block(tiles[0].qry, L.qry_bytes + 4);
	const bool zc_ref = n > 0 && !windows && L.ref_contig && L.ref_bytes > 0 && in_pinned_block(tiles[0].ref, L.ref_bytes + 4);
	b->zero_copy_bytes = (zc_qry ? L.qry_bytes : 0) + (zc_ref ? L.ref_bytes : 0);
	const bool pack_seq = !(zc_qry && (zc_ref || windows));      /* anything left for the host to copy? */
	if (pack_seq) RC_TRY(b->h_seq.ensure((size_t) L.seq_total + 256));
	uint8_t *hseq = b->h_seq.as<uint8_t>();
	uint8_t *hdelta = b->h_delta.as<uint8_t>();
	std::vector<RowOverflow> overflow;
	hipStream_t st = h->s_io;
	/* the three pads: uploaded with the packed blocks, or cleared on the device around the blocks that travel as they are
	 * (queued behind those copies: a copy rounded up to whole dwords may spill a few bytes into the pad that follows) */
	if (pack_seq) upload_zero_pads(L, hseq);
	if (zc_qry || zc_ref) {
		/* Pads around blocks that travel as they are: copied from a page-locked block of zeros, whole 256-byte
		 * units (SDMA engines; a memset would be a kernel that has to find wave slots beside the fill), queued
		 * BEFORE the blocks, which then overwrite the few bytes of overlap.  A block's own copy is rounded up to
		 * whole dwords: up to three bytes of whatever follows it in the caller's arena land in the pad behind it --
		 * pads only have to be readable (every cell outside a tile is forced to the empty element), not zero. */
		const uint64_t zmax = L.pad + 1024;
		RC_TRY(b->h_zero.ensure((size_t) zmax));
		if (b->zero_cap != b->h_zero.cap) { memset(b->h_zero.p, 0, b->h_zero.cap); b->zero_cap = b->h_zero.cap; }
		auto zero_range = [&](uint64_t lo, uint64_t hi) -> int {      /* [lo, hi) widened to 256-byte units, inside the arena */
			lo = lo / 256 * 256;
			hi = std::min<uint64_t>((hi + 255) / 256 * 256, (L.seq_total + 255) / 256 * 256);
			for (uint64_t at = lo; at < hi; at += zmax / 256 * 256) {
				const uint64_t len = std::min<uint64_t>(hi - at, zmax / 256 * 256);
				HIP_TRY(hipMemcpyAsync(b->d_seq.p + at, b->h_zero.p, (size_t) len, hipMemcpyHostToDevice, st));
			}
			return CVX_OK;
		};
		if (zc_qry) {
			RC_TRY(zero_range(0, L.qry_base));
			RC_TRY(zero_range(L.qry_base + L.qry_bytes, L.ref_base));
			HIP_TRY(hipMemcpyAsync(b->d_seq.p + L.qry_base, tiles[0].qry, (size_t) ((L.qry_bytes + 3) / 4 * 4), hipMemcpyHostToDevice, st));
		}
		if (zc_ref) {
			RC_TRY(zero_range(L.ref_base + L.ref_bytes, L.seq_total));
			HIP_TRY(hipMemcpyAsync(b->d_seq.p + L.ref_base, tiles[0].ref, (size_t) ((L.ref_bytes + 3) / 4 * 4), hipMemcpyHostToDevice, st));
		}
	}
	/* what the host still moves per tile decides whether packing is worth threads and pieces */
	uint64_t pack_work = L.delta_total * 9ull;
	if (!zc_qry) pack_work += L.qry_bytes;
	if (!zc_ref && !windows) pack_work += L.ref_bytes;
	const std::vector<uint64_t> &wprefix = L.wprefix;
	int threads = std::max(1, std::min(h->pack_threads, PackPool::get().size()));
	if (pack_work < (8u << 20)) threads = 1;      /* not worth a thread below ~8 MB */
	const int pieces = threads > 1 ? 8 : 1;
	int t0 = 0;
	/* bytes of the two blocks of hseq / of hdelta already on their way (block A = [pad][reads][pad], block B = [references][pad]) */
	uint64_t a_done = 0, b_done = L.ref_base, delta_done = 0;
	const uint64_t a_end_all = L.ref_base, b_end_all = (L.seq_total + 255) / 256 * 256;
	for (int pc = 1; pc <= pieces; ++pc) {
		int t1 = n;
		if (pc < pieces) {
			const uint64_t target = wprefix[(size_t) n] / (uint64_t) pieces * (uint64_t) pc;
			t1 = (int) (std::upper_bound(wprefix.begin(), wprefix.end(), target) - wprefix.begin());
			t1 = std::min(std::max(t1, t0), n);
		}
		if (t1 > t0 && pack_work > 0) {
			std::vector<uint64_t> wp((size_t) (t1 - t0) + 1);
			for (int i = t0; i <= t1; ++i) wp[(size_t) (i - t0)] = wprefix[(size_t) i] - wprefix[(size_t) t0];
			const int base = t0;
			/* every packing range of the piece collects the rows of its misfits in its own list */
			const size_t first = overflow.size();
			overflow.resize(first + (size_t) threads + 1);
			std::atomic<int> slot(0);
			parallel_ranges(t1 - t0, wp, threads, [&](int bg, int en) {
				upload_pack(base + bg, base + en, tiles, tin, hseq, hdelta, L.rsrc, overflow[first + (size_t) slot.fetch_add(1)], !zc_qry, !zc_ref && !windows);
			});
		}
		/* Copy boundaries are multiples of 256 bytes: a host-to-device copy whose address or size is
		 * not dword-aligned is not handed to the SDMA engines but to a blit kernel that pulls the bytes
		 * over PCIe with compute units the fill needs.  The bytes below the rounded-down end are all
		 * packed (tiles are laid out in order inside either block); the remainder travels with the next
		 * piece, the last piece runs to the aligned end. */
		if (!zc_qry) {
			const uint64_t a_end = (t1 == n) ? a_end_all : (uint64_t) tin[(size_t) t1].qry_off / 256 * 256;
			if (a_end > a_done) HIP_TRY(hipMemcpyAsync(b->d_seq.p + a_done, hseq + a_done, (size_t) (a_end - a_done), hipMemcpyHostToDevice, st));
			a_done = std::max(a_done, a_end);
		}
		if (!zc_ref && !windows) {
			const uint64_t b_end = (t1 == n) ? b_end_all : (uint64_t) tin[(size_t) t1].ref_off / 256 * 256;
			if (b_end > b_done) HIP_TRY(hipMemcpyAsync(b->d_seq.p + b_done, hseq + b_done, (size_t) (b_end - b_done), hipMemcpyHostToDevice, st));
			b_done = std::max(b_done, b_end);
		}
		if (L.delta_total) {
			uint64_t del_end = L.delta_total;
			if (t1 < n) {        /* first tile at or after t1 whose rows travel as steps (src_off = step-stream offset until the misfits are renumbered below) */
				int q = t1;
				while (q < n && L.rsrc[(size_t) q].fmt != kRowsDelta8 && L.rsrc[(size_t) q].fmt != kRowsExplicit) q++;
				if (q < n) del_end = L.rsrc[(size_t) q].src_off;
			}
			del_end = (t1 == n) ? (del_end + 255) / 256 * 256 : del_end / 256 * 256;
			if (del_end > delta_done)
				HIP_TRY(hipMemcpyAsync(b->d_delta.p + delta_done, hdelta + delta_done, (size_t) (del_end - delta_done), hipMemcpyHostToDevice, st));
			delta_done = std::max(delta_done, del_end);
		}
		t0 = t1;
	}
	if (n) HIP_TRY(hipMemcpyAsync(b->d_tin.p, b->h_tin.p, (size_t) n * sizeof(TileIn), hipMemcpyHostToDevice, st));
	if (n) {
		/* the misfits' rows (none in any corridor the reference builds), then the rows arena on the device */
		uint64_t n_x = 0;
		for (const RowOverflow &o : overflow) n_x += o.rows.size();
		b->n_rowsx = n_x;
		if (n_x) {
			RC_TRY(b->h_rowsx.ensure((size_t) n_x * sizeof(RowDesc)));
			RC_TRY(b->d_rowsx.ensure((size_t) n_x));
			RowDesc *hx = b->h_rowsx.as<RowDesc>();
			uint64_t at = 0;
			for (const RowOverflow &o : overflow) {
				uint64_t r = 0;
				for (int32_t ti : o.tiles) {
					L.rsrc[(size_t) ti].src_off = at + r;
					r += (uint64_t) tin[(size_t) ti].H;
				}
				if (!o.rows.empty()) memcpy(hx + at, o.rows.data(), o.rows.size() * sizeof(RowDesc));
				at += o.rows.size();
			}
			HIP_TRY(hipMemcpyAsync(b->d_rowsx.p, hx, (size_t) n_x * sizeof(RowDesc), hipMemcpyHostToDevice, st));
		}
		memcpy(b->h_rsrc.p, L.rsrc.data(), (size_t) n * sizeof(RowSrc));
		HIP_TRY(hipMemcpyAsync(b->d_rsrc.p, b->h_rsrc.p, (size_t) n * sizeof(RowSrc), hipMemcpyHostToDevice, st));
		/* rows arena: only for the tiles whose corridors came as arrays; closed forms are evaluated where they are needed */
		if (L.arena_rows) HIP_TRY(launch_expand_rows(b->d_rsrc.p, b->d_tin.p, b->d_delta.p, b->d_rowsx.p, b->d_rows.p, n, false, st));
	}
	if (windows && n) {
		/* the references: decoded from the resident genome straight into the arena (and its last pad cleared) */
		RC_TRY(b->h_win.ensure((size_t) n * sizeof(WindowDesc)));
		RC_TRY(b->d_win.ensure((size_t) n));
		WindowDesc *hw = b->h_win.as<WindowDesc>();
		for (int i = 0; i < n; ++i) {
			hw[i].position = ref_position[i];
			hw[i].dst_off = tin[(size_t) i].ref_off;
			hw[i].n_chars = tiles[i].ref_len;
		}
		HIP_TRY(hipMemcpyAsync(b->d_win.p, hw, (size_t) n * sizeof(WindowDesc), hipMemcpyHostToDevice, st));
		HIP_TRY(hipMemsetAsync(b->d_seq.p + L.ref_base + L.ref_bytes, 0, (size_t) (L.seq_total - L.ref_base - L.ref_bytes), st));
		HIP_TRY(launch_decode_windows(genome->d_bin.p, genome->d_starts.p, genome->n_starts, b->d_win.p, n, b->d_seq.p, st));
		/* the decoded characters back to the host, 1 byte per reference base under everything that follows: a caller whose
		 * text stage runs on the host (MD needs the reference base of every mismatch and deletion) reads them there
		 * (cvx_job_window_refs) instead of decoding the window a second time on a core */
		RC_TRY(b->h_refs.ensure((size_t) L.ref_bytes + 64));
		HIP_TRY(hipMemcpyAsync(b->h_refs.p, b->d_seq.p + L.ref_base, (size_t) L.ref_bytes, hipMemcpyDeviceToHost, st));
		b->refs_base = L.ref_base;
		b->have_refs = true;
	}
	b->state = kUploaded;
	return CVX_OK;
}

/* ---- stage 2: corridor analysis on `st`, records back to the host */
int stage_plan(cvx_context *h, cvx_batch_s *b, hipStream_t st) {
	const int n = b->n;
	HIP_TRY(hipEventRecord(b->ev[0], st));
	if (n) {
		HIP_TRY(launch_plan(b->d_rows.p, b->d_rsrc.p, b->d_tin.p, b->d_plan.p, n, b->n_rows / (uint64_t) n, h->max_matrix_mb, st));
		HIP_TRY(hipMemcpyAsync(b->h_plan.p, b->d_plan.p, (size_t) n * sizeof(TilePlan), hipMemcpyDeviceToHost, st));
	}
	HIP_TRY(hipEventRecord(b->ev[1], st));
	HIP_TRY(hipEventRecord(b->ev_in, st));
	b->state = kPlanned;
	return CVX_OK;
}

/* ---- stage 3: host planning, then every kernel of the batch on `main` (+ aux); nothing waits */
int stage_compute(cvx_context *h, cvx_batch_s *b, bool streaming = false) {
	const int n = b->n;
	if (h->test_fail_compute > 0 && --h->test_fail_compute == 0) {      /* test knob: this job fails before anything is queued for it */
		set_err("stage_compute: failure injected by CVX_TUNE_FAIL_COMPUTE");
		return CVX_ERR_OOM;
	}
	/* which stream set carries this batch's kernels (see cvx_context::s_main2) */
	const bool second = streaming && n > 0 && n < kSmallJobTiles && !h->single_lane && ((h->small_jobs++ & 1u) != 0u);
	hipStream_t const S_main = second ? h->s_main2 : h->s_main;
	hipStream_t const S_post = second ? h->s_post2 : h->s_post;
	hipStream_t const *S_aux = second ? h->aux2 : h->aux;
	b->s_run = S_main;
	hipStream_t st = S_main;
	HIP_TRY(hipEventSynchronize(b->ev_in));        /* queued a whole batch ago in the streaming case */
	b->launches.clear();
	b->ops_total = 0;
	b->have_ops = false;
	if (n == 0) {
		HIP_TRY(hipEventRecord(b->ev[4], st));
		hipStream_t ps = h->overlap_post ? S_post : S_main;
		HIP_TRY(hipStreamWaitEvent(ps, b->ev[4], 0));
		HIP_TRY(hipEventRecord(b->ev[2], ps));
		HIP_TRY(hipEventRecord(b->ev[3], ps));
		HIP_TRY(hipEventRecord(b->ev_res, ps));
		b->state = kComputed;
		return CVX_OK;
	}

	/* host planning: kernel class, arena offsets, work lists (cvx_host_logic.h) */
	HostPlan hp;
	PlanTuning tune;
	tune.min_slots = h->tune_min_slots; tune.max_slots = h->tune_max_slots; tune.force_wrap = h->tune_force_wrap; tune.chain_m = h->tune_chain_m;
	tune.force_generic = h->sse_variant ? 1 : 0;
	tune.long_steps = h->tune_long_steps; tune.small_batch = h->tune_small_batch; tune.long_need = h->tune_long_need;
	tune.no_gangs = h->tune_gangs ? 0 : 1;
	/* (a tile that gets chained needs its rows on the host: rebuilt from the step stream the batch still owns) */
	const RowSrc *rsrc = b->h_rsrc.as<RowSrc>();
	host_plan_rows(n, b->plan(), b->tin(), [&](int i, std::vector<RowDesc> &tmp) -> const RowDesc * {
		tmp.resize((size_t) std::max(b->tin()[(size_t) i].H, 1));
		expand_rows_host(rsrc[(size_t) i], b->tin()[(size_t) i].H, b->h_delta.as<uint8_t>(), b->h_rowsx.as<RowDesc>(), tmp.data());
		return tmp.data();
	}, true, tune, hp);
	std::vector<std::vector<int32_t>> &cls = hp.cls;
	std::vector<int32_t> &generic = hp.generic;
	RC_TRY(b->d_dirs.ensure((size_t) hp.dir_dwords + 64));
	RC_TRY(b->d_regions.ensure((size_t) hp.ops_ints + 64));
	/* dense ops arena: an alignment of H read bases has far fewer than H run-length ops (about
	 * 0.3 H at 15 % error); if a batch ever needs more, finalize reports it and stage_ops
	 * compacts again into a larger arena */
	b->dense_cap = std::min<uint64_t>(hp.ops_ints, hp.ops_ints / 3 + 64ull * (uint64_t) n);
	RC_TRY(b->d_dense.ensure((size_t) b->dense_cap + 64));
	b->dense_cap = std::max<uint64_t>(b->dense_cap, b->d_dense.cap - 64);

	RC_TRY(b->h_trun.ensure((size_t) n * sizeof(TileRun)));
	RC_TRY(b->h_tout.ensure((size_t) n * sizeof(TileOut)));
	RC_TRY(b->h_lists.ensure((size_t) 2 * n * sizeof(int32_t) + 64));
	memcpy(b->h_trun.p, hp.trun.data(), (size_t) n * sizeof(TileRun));
	memcpy(b->h_tout.p, hp.tout.data(), (size_t) n * sizeof(TileOut));
	int32_t *lists = b->h_lists.as<int32_t>();
	size_t n_listed = 0;
	std::vector<int> seg_begin(cls.size(), 0);
	/* Very long tiles go straight to the exact-tracking instantiation.  The two-phase pass saves three half-rate ops per
	 * cell (~12 %) but a tile whose best cell is not in its last anti-diagonals -- a local alignment: an inverted segment,
	 * a read that does not reach its end -- is redone from step 0, and for a 100 kb tile that second pass is another
	 * ~100 ms on one wave behind everything else (C5 mix: 77 ms of a 200 ms fill).  Tiles of kExactDirectSteps steps and
	 * more are flagged kPadRedo up front and listed first; the exact launch over that prefix does them once.  Only while
	 * the class cannot fill the device several times over (then 12 % of throughput would cost more than the tail). */
	std::vector<int> n_direct(cls.size(), 0);
	for (size_t c = 0; c < cls.size(); ++c) {
		seg_begin[c] = (int) n_listed;      /* already in LPT order */
		if (h->tune_exact_steps > 0 && !cls[c].empty()) {
			int nl = 0;
			for (int32_t ti : cls[c]) if (hp.trun[(size_t) ti].nsteps >= h->tune_exact_steps) nl++;
			if (nl > 0 && nl <= kExactDirectMaxTiles) {
				std::stable_partition(cls[c].begin(), cls[c].end(), [&](int32_t ti) { return hp.trun[(size_t) ti].nsteps >= h->tune_exact_steps; });
				TileOut *ho = b->h_tout.as<TileOut>();
				for (int q = 0; q < nl; ++q) ho[(size_t) cls[c][(size_t) q]].pad = kPadRedo;
				n_direct[c] = nl;
			}
		}
		if (!cls[c].empty()) memcpy(lists + n_listed, cls[c].data(), cls[c].size() * sizeof(int32_t));
		n_listed += cls[c].size();
	}
	const int generic_begin = (int) n_listed;
	if (!generic.empty()) memcpy(lists + n_listed, generic.data(), generic.size() * sizeof(int32_t));
	n_listed += generic.size();
	/* behind the fill lists: every computed tile once, longest read first (counting sort on H / 32) --
	 * the order in which the backtrack takes them, four to a wave: the walk of a tile is a serial
	 * chain of ~H / 7 probes, so the long ones must start first and share their wave with their like.
	 * One segment per fill launch, in launch order (chained classes, whole-tile classes from the widest ring down, the
	 * catch-all kernel): a batch of several classes walks each class right behind its own fill, on that fill's stream,
	 * while the other classes still fill; a batch of one class has one segment = the whole list. */
	const size_t bt_begin = n_listed;
	std::vector<const std::vector<int32_t> *> launch_tiles;
	for (size_t c = 0; c < hp.chain_tasks.size(); ++c) if (!hp.chain_tasks[c].empty()) launch_tiles.push_back(&hp.chain_tiles[c]);
	for (int cc = (int) cls.size() - 1; cc >= 0; --cc) if (!cls[(size_t) cc].empty()) launch_tiles.push_back(&cls[(size_t) cc]);
	if (!generic.empty()) launch_tiles.push_back(&generic);
	std::vector<std::pair<size_t, int>> bt_seg;      /* (offset in lists, tiles) per launch */
	{
		const TileIn *tin = b->tin();
		constexpr int kBuckets = 4096;
		auto bucket = [&](int32_t ti) { const int k = tin[(size_t) ti].H >> 5; return kBuckets - 1 - (k < kBuckets ? k : kBuckets - 1); };
		std::vector<int32_t> count((size_t) kBuckets + 1);
		for (const std::vector<int32_t> *v : launch_tiles) {
			std::fill(count.begin(), count.end(), 0);
			for (int32_t ti : *v) if (!hp.trun[(size_t) ti].skip) count[(size_t) bucket(ti) + 1]++;
			for (int k = 0; k < kBuckets; ++k) count[(size_t) k + 1] += count[(size_t) k];
			const size_t at = n_listed;
			const int m = count[(size_t) kBuckets];
			/* (stable: inside a bucket of equally long reads the class's own order, most cells first) */
			for (int32_t ti : *v) if (!hp.trun[(size_t) ti].skip) lists[at + (size_t) count[(size_t) bucket(ti)]++] = ti;
			n_listed += (size_t) m;
			bt_seg.emplace_back(at, m);
		}
	}
	const int n_walk = (int) (n_listed - bt_begin);
	if (!generic.empty()) {
		RC_TRY(b->h_goff.ensure((generic.size() + 1) * sizeof(uint64_t)));
		uint64_t *goff = b->h_goff.as<uint64_t>();
		goff[0] = 0;
		for (size_t g = 0; g < generic.size(); ++g)
			goff[g + 1] = goff[g] + (uint64_t) generic_scratch_bytes(hp.trun[(size_t) generic[g]].ring);
		RC_TRY(b->d_gscratch.ensure((size_t) goff[generic.size()] + 256));
		RC_TRY(b->d_gscratch_off.ensure(generic.size() + 1));
		HIP_TRY(hipMemcpyAsync(b->d_gscratch_off.p, goff, (generic.size() + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
	}
	/* chained tiles: tasks of every chain class, block table and tile lists in one upload */
	size_t chain_task_off[kNumChainClasses * 2] = {0}, chain_tile_off[kNumChainClasses * 2] = {0};
	size_t chain_blk_off = 0, chain_bytes = 0;
	if (hp.n_chained) {
		for (size_t c = 0; c < hp.chain_tasks.size(); ++c) { chain_task_off[c] = chain_bytes; chain_bytes += hp.chain_tasks[c].size() * sizeof(ChainTask); }
		chain_blk_off = chain_bytes; chain_bytes += hp.chain_blk.size() * sizeof(ChainBlk);
		for (size_t c = 0; c < hp.chain_tiles.size(); ++c) { chain_tile_off[c] = chain_bytes; chain_bytes += (hp.chain_tiles[c].size() * sizeof(int32_t) + 7) / 8 * 8; }
		RC_TRY(b->h_chain.ensure(chain_bytes));
		uint8_t *hc = b->h_chain.as<uint8_t>();
		for (size_t c = 0; c < hp.chain_tasks.size(); ++c)
			if (!hp.chain_tasks[c].empty()) memcpy(hc + chain_task_off[c], hp.chain_tasks[c].data(), hp.chain_tasks[c].size() * sizeof(ChainTask));
		memcpy(hc + chain_blk_off, hp.chain_blk.data(), hp.chain_blk.size() * sizeof(ChainBlk));
		for (size_t c = 0; c < hp.chain_tiles.size(); ++c)
			if (!hp.chain_tiles[c].empty()) memcpy(hc + chain_tile_off[c], hp.chain_tiles[c].data(), hp.chain_tiles[c].size() * sizeof(int32_t));
		RC_TRY(b->d_chain.ensure(chain_bytes));
		RC_TRY(b->d_chain_out.ensure(hp.chain_blk.size()));
		{
			/* boundary records validate themselves by the launch epoch in their upper bits: a buffer starts out zeroed
			 * (epoch 0 = never written) and is zeroed again when the epochs wrap */
			const size_t had = b->d_bnd.cap;
			RC_TRY(b->d_bnd.ensure((size_t) hp.bnd_recs + 64));
			if (b->d_bnd.cap != had || b->bnd_epoch >= kBndEpochMax) {
				HIP_TRY(hipMemsetAsync(b->d_bnd.p, 0, b->d_bnd.cap * sizeof(BoundaryRec), st));
				b->bnd_epoch = 0;
			}
			b->bnd_epoch += 1;
		}
		HIP_TRY(hipMemcpyAsync(b->d_chain.p, hc, chain_bytes, hipMemcpyHostToDevice, st));
	}
	HIP_TRY(hipMemcpyAsync(b->d_trun.p, b->h_trun.p, (size_t) n * sizeof(TileRun), hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemcpyAsync(b->d_tout.p, b->h_tout.p, (size_t) n * sizeof(TileOut), hipMemcpyHostToDevice, st));
	if (n_listed) HIP_TRY(hipMemcpyAsync(b->d_lists.p, lists, n_listed * sizeof(int32_t), hipMemcpyHostToDevice, st));
	/* (the batch's counters are zero: cleared when the arena was allocated and again by finalize_kernel,
	 * their last reader -- a memset here would be a tiny kernel that has to find a free wave slot among
	 * the previous batch's 24 576 backtrack waves before this batch's fills may start: measured 7 ms) */
	HIP_TRY(hipEventRecord(b->ev[4], st));        /* inputs of the fills are in place */

	/* forward fill: one launch per populated kernel class (+ its exact redo pass), classes run
	 * concurrently on separate streams (a sparsely populated class would otherwise serialise a
	 * whole tile latency behind the big one); widest rings first, they have the longest tiles */
	auto fill_args = [&](const int32_t *list, int list_n) {
		FillArgs a;
		a.seq = b->d_seq.p;
		a.rows = reinterpret_cast<const RowDesc2 *>(b->d_rows.p);
		a.rsrc = b->d_rsrc.p;
		a.tin = b->d_tin.p;
		a.trun = b->d_trun.p;
		a.tout = b->d_tout.p;
		a.dirs = b->d_dirs.p;
		a.list = list;
		a.list_n = list_n;
		a.redo_count = b->d_counters.p;
		a.late_min_groups = h->tune_late_min;
		a.late_shift = h->tune_late_shift;
		a.pen_table = h->tune_pen_table;
		a.tasks = nullptr; a.chain_ticket = nullptr; a.bnd = nullptr; a.chain_out = nullptr; a.bnd_epoch = 0; a.chain_prio = 0;
		a.ops = b->d_regions.p;
		a.sp = h->sp;
		return a;
	};
	auto launch_stats = [&](const std::vector<int32_t> &v, int m, int nw, int wrap, int kind) {
		cvx_launch_info li;
		memset(&li, 0, sizeof(li));
		li.slots_per_lane = m; li.waves = nw; li.wrap16 = wrap; li.n_tiles = (int) v.size(); li.kind = kind;
		for (int32_t ti : v) {
			const TilePlan &p = b->plan()[(size_t) ti];
			const TileIn &in = b->tin()[(size_t) ti];
			li.cells += p.cells; li.active_cells += p.active;
			li.alg_bytes += p.cells + 6ull * (uint64_t) in.H + 2ull * (uint64_t) in.W;
			li.read_bases += (uint64_t) in.H;
		}
		b->launches.push_back(li);
	};
	/* backtrack, device-side result records + prefix sums, ops compaction */
	BacktrackArgs ba;
	ba.chain_blk = hp.n_chained ? reinterpret_cast<const ChainBlk *>(b->d_chain.p + chain_blk_off) : nullptr;
	ba.seq = b->d_seq.p;
	ba.rows = reinterpret_cast<const RowDesc2 *>(b->d_rows.p);
	ba.rsrc = b->d_rsrc.p;
	ba.tin = b->d_tin.p;
	ba.trun = b->d_trun.p;
	ba.tout = b->d_tout.p;
	ba.dirs = b->d_dirs.p;
	ba.ops = b->d_regions.p;
	ba.n_tiles = n;
	/* the walk of lists[at, at + count) (longest read first) on `ws`.  Few tiles in the batch: the walk is latency-bound and
	 * 64 probing lanes per tile take the long diagonal runs in a quarter of the probes; many tiles: it is issue-bound and
	 * several tiles share a wave -- eight for the bulk; the few reads much longer than the rest (a latency-bound tail, a
	 * serial chain of H / 7 probes each) get 32 lanes per tile, beside the bulk on `side` when `fork` (one walk for the whole
	 * batch), in front of it on the same stream otherwise (measured: PacBio 5.4 -> 4.9 ms with 8 lanes, ONT mix 8.2 -> 6.6 with 32) */
	auto walk_list = [&](size_t at, int count, hipStream_t ws, hipStream_t side, bool fork) -> int {
		if (count <= 0) return CVX_OK;
		/* Lanes per tile by the number of tiles walked together (round 5): a walk is a serial chain of probes per tile, and
		 * what hides a probe's latency is other waves -- so few tiles get many lanes each (a probe then covers 64 / 32 / 16
		 * path columns of a diagonal run instead of 8) until the walk has about six waves per SIMD, and only beyond that
		 * is it issue-bound and eight lanes per tile the cheapest.  Measured against round 4's rule (one wave per tile below
		 * 4 096 tiles, eight lanes from there on): C5 mix, 4 096 tiles of 100 kb, walk 39.5 ms at 8 lanes = 512 waves on 1 024
		 * SIMDs, 25.9 at 16, 21.6 at 32, 19.4 at 64; ONT mix at 49 152 tiles in one walk 7.6 ms at 8, 6.0 at 16; the PacBio
		 * bench (49 152 tiles): the walk alone 7.7 ms at 8 and 8.4 at 16, the pipelined step 114.4-114.9 against 113.9-114.1 ms
		 * (profiles/r05_ab_bt_group.txt). */
		const int auto_group = count <= 6144 ? 64 : count <= 12288 ? 32 : count <= 49152 ? 16 : 8;
		if (h->bt_group < 0 ? n_walk < 4096 : (h->bt_group == 0 && auto_group == 64)) {
			HIP_TRY(launch_backtrack(ba, b->d_lists.p + at, count, 64, ws));
		} else if (h->bt_group > 0) {
			HIP_TRY(launch_backtrack(ba, b->d_lists.p + at, count, h->bt_group, ws));
		} else if (h->bt_group == 0 && auto_group >= 32) {
			HIP_TRY(launch_backtrack(ba, b->d_lists.p + at, count, auto_group, ws));
		} else {
			const int bulk = h->bt_group < 0 ? 8 : auto_group;      /* 8 or 16; the much-longer-than-average reads at 32 */
			const TileIn *tin = b->tin();
			const uint64_t mean_h = b->n_rows / (uint64_t) std::max(n, 1);
			int n_long = 0;
			while (n_long < count && (uint64_t) tin[(size_t) lists[at + (size_t) n_long]].H > 3 * mean_h) n_long++;
			if (n_long > 0 && fork) {
				HIP_TRY(hipEventRecord(b->ev_bt0, ws));
				HIP_TRY(hipStreamWaitEvent(side, b->ev_bt0, 0));
				HIP_TRY(launch_backtrack(ba, b->d_lists.p + at, n_long, 32, side));
				HIP_TRY(hipEventRecord(b->ev_bt1, side));
			} else if (n_long > 0) {
				HIP_TRY(launch_backtrack(ba, b->d_lists.p + at, n_long, 32, ws));
			}
			HIP_TRY(launch_backtrack(ba, b->d_lists.p + at + n_long, count - n_long, bulk, ws));
			if (n_long > 0 && fork) HIP_TRY(hipStreamWaitEvent(ws, b->ev_bt1, 0));
		}
		return CVX_OK;
	};
	/* Several fill classes (ONT mix: chained retries, M = 4, M = 3; C5): each class is walked right behind its own fill on
	 * that fill's stream.  The launch of such a batch lasts as long as its longest dependency chain, and while the last
	 * chains finish on a few waves the device has issue slots to spare: the other classes' walks run there instead of
	 * behind everything (CVX_TUNE_BT_PER_CLASS=0: one walk behind all fills, as a batch of one class has it anyway). */
	static const bool bt_per_class_env = !(getenv("CVX_TUNE_BT_PER_CLASS") && atoi(getenv("CVX_TUNE_BT_PER_CLASS")) == 0);
	/* Only where the walk is issue-bound (>= 4096 tiles; measured, r04c: ONT mix 60 000 tiles 57.2 -> 56.0 ms, 24 000 tiles
	 * 35.3 -> 34.2, C5 mix 6 144 tiles 397 -> 369 ms); a small batch's one-wave-per-tile walks are latency-bound chains that
	 * gain nothing from starting early and cost the fills still running (C5 mix 2 048 tiles: 183.6 -> 187.2 ms). */
	const bool per_class = bt_per_class_env && launch_tiles.size() > 1 && !h->overlap_post && n_walk >= 4096;
	int launches = 0;
	/* fill launches go round-robin over the two aux streams and the main stream itself (which has
	 * nothing else to do until they are all done): three classes side by side */
	/* (the `post` stream carries a fill class too unless the post-fill overlap experiment owns it) */
	hipStream_t fill_streams[kAuxStreams + 2];
	int n_fill_streams = 0;
	/* (order: first side stream, post, main -- the assignment of rounds 2-4 for up to three classes -- and the second side stream
	 * only for a fourth class, i.e. with gangs.  Which class rides on which stream is not neutral: with the three whole-tile
	 * classes of the C5 mix on side / side / post instead of side / post / main the same batch takes 181 or 236 ms depending on the
	 * handle, on side / post / main 194 every time: gpurun_out r05u, profiles/r05_fill_stream_order.txt) */
	fill_streams[n_fill_streams++] = S_aux[0];
	if (!h->overlap_post) fill_streams[n_fill_streams++] = S_post;
	fill_streams[n_fill_streams++] = st;
	for (int i = 1; i < kAuxStreams; ++i) fill_streams[n_fill_streams++] = S_aux[i];
	auto begin_launch = [&](hipStream_t ls) -> int {
		while (b->lev.size() < (size_t) (launches + 1) * 4) {
			hipEvent_t e;
			HIP_TRY(hipEventCreate(&e));
			b->lev.push_back(e);
		}
		HIP_TRY(hipStreamWaitEvent(ls, b->ev[4], 0));
		HIP_TRY(hipEventRecord(b->lev[(size_t) launches * 4], ls));
		return CVX_OK;
	};
	/* closes launch number `launches` on its stream: the class's own walk (per_class), then the event everything after waits for */
	auto end_launch = [&](hipStream_t ls) -> int {
		if (per_class) RC_TRY(walk_list(bt_seg[(size_t) launches].first, bt_seg[(size_t) launches].second, ls, ls, false));
		HIP_TRY(hipEventRecord(b->lev[(size_t) launches * 4 + 3], ls));
		launches++;
		return CVX_OK;
	};
	/* chained tiles first (their dependency chains are the longest thing in a batch): the row-block
	 * tasks of a class, then the per-tile reduction of the block results */
	for (size_t c = 0; c < hp.chain_tasks.size(); ++c) {
		if (hp.chain_tasks[c].empty()) continue;
		const int m = kChainClasses[c / 2];
		launch_stats(hp.chain_tiles[c], m, (int) hp.chain_tasks[c].size(), (int) (c & 1), CVX_LAUNCH_CHAINED);     /* `waves` = row-block tasks */
		hipStream_t ls = fill_streams[launches % n_fill_streams];
		RC_TRY(begin_launch(ls));
		FillArgs a = fill_args(nullptr, (int) hp.chain_tasks[c].size());
		a.tasks = reinterpret_cast<const ChainTask *>(b->d_chain.p + chain_task_off[c]);
		a.chain_ticket = b->d_counters.p + 8 + (int) c;
		a.bnd = b->d_bnd.p;
		a.bnd_epoch = b->bnd_epoch;
		a.chain_prio = (h->tune_chain_prio >= 0) ? h->tune_chain_prio : 1;
		a.chain_out = b->d_chain_out.p;
		/* tasks are dispatched in order, long before their turn; resident tasks beyond the ones that can
		 * actually run only poll.  Unused dynamic LDS caps the residency at ~1.5x the blocks that are
		 * live at one time (need / rows-per-block per tile, + slack). */
		uint64_t live = 0;
		for (int32_t ti : hp.chain_tiles[c]) live += (uint64_t) b->plan()[(size_t) ti].need / (uint64_t) (64 * m + kChainChunk) + 2;
		const uint64_t resident = std::min<uint64_t>(8192, std::max<uint64_t>(768, live + live / 2 + 256));
		const size_t per_cu = (size_t) ((resident + (uint64_t) h->num_cus - 1) / (uint64_t) h->num_cus);
		size_t pad_lds = per_cu >= 32 ? 0 : (size_t) (160 * 1024) / per_cu - 4096;
		pad_lds = std::min<size_t>(pad_lds, 60 * 1024) / 256 * 256;
		/* The padding is LDS the ring classes of the same batch cannot use: a handful of chained retries among a thousand whole
		 * tiles (ngmlr's own launches: 10-40 chained tiles, resident = 768 tasks = 3 per CU at 50 KB each) held 150 of a CU's
		 * 160 KB for their 7 ms, and the M = 3 / M = 4 classes -- 4-5 KB per wave -- crawled until they were gone: a launch's
		 * fill was the SUM of the chained class and the widest ring class (18.6 = 7.0 + 11.7 ms, profiles/r06_e2e_launch_trace.txt).
		 * Beside ring classes the cap may hold tune_chain_lds_kb per CU; more tasks than can run then sit in their back-off sleep. */
		bool rings_beside = false;
		for (size_t rc_ = 0; rc_ < cls.size(); ++rc_) rings_beside = rings_beside || !cls[rc_].empty();
		if (rings_beside && h->tune_chain_lds_kb > 0 && per_cu > 0 && per_cu < 32) {
			const size_t budget = (size_t) h->tune_chain_lds_kb * 1024 / per_cu;
			const size_t capped = budget > 4096 ? (budget - 4096) / 256 * 256 : 0;
			pad_lds = std::min(pad_lds, capped);
		}
		HIP_TRY(launch_fill(m, 1, (c & 1) != 0, 2, a, pad_lds, ls));
		HIP_TRY(launch_chain_reduce(reinterpret_cast<const int32_t *>(b->d_chain.p + chain_tile_off[c]), (int) hp.chain_tiles[c].size(),
				b->d_trun.p, b->d_chain_out.p, b->d_tout.p, ls));
		HIP_TRY(hipEventRecord(b->lev[(size_t) launches * 4 + 1], ls));
		HIP_TRY(hipEventRecord(b->lev[(size_t) launches * 4 + 2], ls));
		RC_TRY(end_launch(ls));
	}
	int ring_classes = 0;
	for (size_t c = 0; c < cls.size(); ++c) ring_classes += cls[c].empty() ? 0 : 1;
	bool widest = true;
	for (int cc = (int) cls.size() - 1; cc >= 0; --cc) {
		const size_t c = (size_t) cc;
		if (cls[c].empty()) continue;
		const KernelClass &kc = kClasses[c / 2];
		const int wide_prio = (h->tune_wide_prio && widest && ring_classes > 1) ? h->tune_wide_prio : 0;
		widest = false;
		launch_stats(cls[c], kc.m, kc.gang, (int) (c & 1), kc.gang > 1 ? CVX_LAUNCH_GANG : CVX_LAUNCH_WHOLE);      /* `waves` = waves per tile (a gang's size) */
		hipStream_t ls = fill_streams[launches % n_fill_streams];
		RC_TRY(begin_launch(ls));
		if (n_direct[c] > 0) {
			/* the very long tiles of the class, exact from the first step (flagged above), before everything else */
			FillArgs ad = fill_args(b->d_lists.p + seg_begin[c], n_direct[c]);
			ad.chain_prio = kc.gang > 1 ? h->tune_gang_prio : wide_prio;
			HIP_TRY(launch_fill(kc.m, kc.gang, (c & 1) != 0, 1, ad, 0, ls));
		}
		FillArgs a = fill_args(b->d_lists.p + seg_begin[c] + n_direct[c], (int) cls[c].size() - n_direct[c]);
		a.chain_prio = kc.gang > 1 ? h->tune_gang_prio : wide_prio;
		if (a.list_n > 0) HIP_TRY(launch_fill(kc.m, kc.gang, (c & 1) != 0, 0, a, 0, ls));
		HIP_TRY(hipEventRecord(b->lev[(size_t) launches * 4 + 1], ls));
		/* exact-tracking pass over the tiles the two-phase pass flagged (usually none) */
		if (a.list_n > 0) HIP_TRY(launch_fill(kc.m, kc.gang, (c & 1) != 0, 1, a, 0, ls));
		HIP_TRY(hipEventRecord(b->lev[(size_t) launches * 4 + 2], ls));
		RC_TRY(end_launch(ls));
	}
	if (!generic.empty()) {
		launch_stats(generic, 0, 16, 1, CVX_LAUNCH_CATCH_ALL);
		hipStream_t ls = fill_streams[launches % n_fill_streams];
		RC_TRY(begin_launch(ls));
		const FillArgs a = fill_args(b->d_lists.p + generic_begin, (int) generic.size());
		HIP_TRY(launch_fill_generic(a, h->sse_variant, b->d_gscratch.p, b->d_gscratch_off.p, ls));
		HIP_TRY(hipEventRecord(b->lev[(size_t) launches * 4 + 1], ls));
		HIP_TRY(hipEventRecord(b->lev[(size_t) launches * 4 + 2], ls));
		RC_TRY(end_launch(ls));
	}
	/* Everything after the fills CAN run on its own stream, so that `main` goes straight on to the next
	 * batch's fills while this batch's backtrack (one wave per tile) and small kernels run beside them. */
	/* Measured (profiles/r02_timeline.txt): the overlap only moves time around -- fill and backtrack
	 * are bound by the same issue slots, the step takes fill + backtrack either way (76 ms for 24 576
	 * PacBio tiles), and the fill's own launch stretches from 66 to 76 ms.  It therefore stays OFF by
	 * default (post == main, stages back to back, clean per-kernel timings); CVX_TUNE_OVERLAP_POST=1
	 * turns it on. */
	st = h->overlap_post ? S_post : S_main;
	HIP_TRY(hipStreamWaitEvent(st, b->ev[4], 0));  /* also orders `post` behind the input copies when no fill was launched */
	for (int i = 0; i < launches; ++i) HIP_TRY(hipStreamWaitEvent(st, b->lev[(size_t) i * 4 + 3], 0));
	HIP_TRY(hipEventRecord(b->ev[2], st));

	if (!per_class) {
		RC_TRY(walk_list(bt_begin, n_walk, st, S_aux[0], true));
	}
	ResultRec *d_rec = reinterpret_cast<ResultRec *>(b->d_res.p);
	BatchSummary *d_sum = reinterpret_cast<BatchSummary *>(b->d_res.p + (size_t) n * sizeof(ResultRec));
	HIP_TRY(launch_finalize(b->d_tout.p, b->d_plan.p, b->d_dstoff.p, d_rec, d_sum, b->d_counters.p, n, b->dense_cap, st));
	HIP_TRY(launch_compact(b->d_regions.p, b->d_trun.p, b->d_tout.p, b->d_dstoff.p, b->d_dense.p, n, b->dense_cap, st));
	HIP_TRY(hipEventRecord(b->ev[3], st));
	HIP_TRY(hipMemcpyAsync(b->h_res.p, b->d_res.p, (size_t) n * sizeof(ResultRec) + sizeof(BatchSummary), hipMemcpyDeviceToHost, st));
	HIP_TRY(hipEventRecord(b->ev_res, st));

	b->timing.cells = hp.cells;
	b->timing.active_cells = hp.active;
	b->timing.dir_bytes = hp.dir_dwords * 4;
	b->timing.n_fill_launches = launches;
	b->timing.n_tiles_fast = hp.n_fast;
	b->timing.n_tiles_chained = hp.n_chained;
	b->state = kComputed;
	return CVX_OK;
}

/* ---- wait for the result records; timing of the batch */
int stage_results(cvx_context *h, cvx_batch_s *b) {
	(void) h;
	if (b->state < kComputed) { set_err("internal: results requested from a batch whose kernels were never queued (state %d)", b->state); return CVX_ERR_ARG; }
	HIP_TRY(hipEventSynchronize(b->ev_res));
	if (b->n == 0) { b->ops_total = 0; b->state = kFinished; return CVX_OK; }
	const BatchSummary *s = b->summary();
	b->ops_total = s->ops_total;
	const int launches = b->timing.n_fill_launches;
	for (int i = 0; i < launches; ++i) b->launches[(size_t) i].ms = ev_ms(b->lev[(size_t) i * 4], b->lev[(size_t) i * 4 + 1]);
	b->timing.plan_ms = ev_ms(b->ev[0], b->ev[1]);
	/* fill = until the last fill class has finished its exact pass; backtrack = what is left of the compute stage (when every
	 * class is walked behind its own fill, the walks of the early classes lie inside `fill`: the two still add up) */
	float fill_end = 0.0f;
	for (int i = 0; i < launches; ++i) fill_end = std::max(fill_end, ev_ms(b->ev[4], b->lev[(size_t) i * 4 + 2]));
	if (launches == 0) fill_end = ev_ms(b->ev[4], b->ev[2]);
	b->timing.fill_ms = fill_end;
	b->timing.backtrack_ms = std::max(0.0f, ev_ms(b->ev[4], b->ev[3]) - fill_end);
	b->timing.total_ms = b->timing.plan_ms + ev_ms(b->ev[4], b->ev[3]);
	b->timing.n_tiles_redone = s->n_redone;
	b->timing.chain_task_ticks = s->chain_task_ticks;
	b->timing.chain_poll_ticks = s->chain_poll_ticks;
	b->state = kFinished;
	return CVX_OK;
}

/* ---- stage 4: dense ops to pinned host memory (stream `io`) */
int stage_ops(cvx_context *h, cvx_batch_s *b) {
	if (b->have_ops) return CVX_OK;
	if (b->ops_total > b->dense_cap) {
		/* rare: more ops than the arena was sized for -- grow it and compact again */
		const uint64_t cap = b->ops_total;
		RC_TRY(b->d_dense.ensure((size_t) cap + 64));
		b->dense_cap = b->d_dense.cap - 64;
		hipStream_t ps = b->s_run ? b->s_run : h->s_main;      /* the batch's own stream set: behind everything it queued */
		HIP_TRY(launch_compact(b->d_regions.p, b->d_trun.p, b->d_tout.p, b->d_dstoff.p, b->d_dense.p, b->n, b->dense_cap, ps));
		HIP_TRY(hipStreamSynchronize(ps));
	}
	if (b->ops_total) {
		RC_TRY(b->h_ops.ensure((size_t) b->ops_total * sizeof(uint32_t)));
		/* The wait below is for the whole io stream, on purpose: it already carries the upload and corridor analysis of the
		 * job submitted last, and returning only when those are done paces the caller -- it submits its next batch one
		 * step later, so that exactly one corridor analysis runs beside each fill (beside a fill it takes most of the
		 * fill's duration; two of them queued under one fill finish late and the next fill starts late: measured 150
		 * instead of 124 ms per step with an event right behind the copy).  CVX_TUNE_OPS_EVENT=1 selects the event. */
		HIP_TRY(hipMemcpyAsync(b->h_ops.p, b->d_dense.p, (size_t) b->ops_total * sizeof(uint32_t), hipMemcpyDeviceToHost, h->s_io));
		/* Round 4 tried to drop the pacing for closed-form batches (their corridor analysis reads nothing: 2.3 ms alone): over
		 * 3 steps of 24 576 tiles the event-only form measured the same, over the driver's 20 steps of 49 152 tiles it costs
		 * 146.5 instead of 118.7 ms per step (gpurun_out/r04g/pacing.txt) -- the analysis is starved beside a fill whatever it
		 * reads (70-100 ms), and two of them queued under one fill still delay the fill after next.  The stream wait stays;
		 * CVX_TUNE_OPS_EVENT=1 selects the event. */
		static const bool ops_event = getenv("CVX_TUNE_OPS_EVENT") && atoi(getenv("CVX_TUNE_OPS_EVENT")) != 0;
		if (ops_event) {
			HIP_TRY(hipEventRecord(b->ev_ops, h->s_io));
			HIP_TRY(hipEventSynchronize(b->ev_ops));
		} else {
			HIP_TRY(hipStreamSynchronize(h->s_io));
		}
	}
	b->have_ops = true;
	return CVX_OK;
}

/* queue the compute stage of every submitted batch whose plan records have arrived (all of them,
 * up to `upto`, when `block`): keeps the device one batch ahead of the host */
int pump(cvx_context *h, bool block, const cvx_batch_s *upto) {
	while (!h->pending.empty()) {
		cvx_batch_s *b = h->pending.front();
		if (!block) {
			hipError_t q = hipEventQuery(b->ev_in);
			if (q == hipErrorNotReady) { (void) hipGetLastError(); break; }
			if (q != hipSuccess) { set_err("hipEventQuery: %s", hipGetErrorString(q)); h->pending.erase(h->pending.begin()); (void) fail_job(b, CVX_ERR_HIP); continue; }
		}
		h->pending.erase(h->pending.begin());
		/* a failure (say, the direction arena of a multi-GB batch does not fit beside the batches in flight) belongs
		 * to THIS job: it is recorded on it and reported by its own cvx_wait, never against another job's call */
		const int rc = stage_compute(h, b, true);
		if (rc != CVX_OK) (void) fail_job(b, rc);
		if (upto && b == upto) break;
	}
	return CVX_OK;
}

}  // namespace

extern "C" {

/* ------------------------------------------------------------------ staged form */

int cvx_batch_upload(cvx_handle h, int32_t n, const cvx_tile *tiles, cvx_batch *out) {
	ABI_GUARD_BEGIN
	if (!h || !out || n < 0 || (n > 0 && !tiles)) { set_err("cvx_batch_upload: bad argument"); return CVX_ERR_ARG; }
	*out = nullptr;
	HIP_TRY(hipSetDevice(h->device));
	cvx_batch_s *b = acquire_batch(h);
	if (!b) return CVX_ERR_OOM;
	int rc = stage_upload(h, b, n, tiles);
	if (rc == CVX_OK) {
		hipError_t e = hipStreamSynchronize(h->s_io);     /* inputs resident when this returns */
		if (e != hipSuccess) { set_err("upload copy failed: %s", hipGetErrorString(e)); rc = CVX_ERR_HIP; }
	}
	if (rc != CVX_OK) { discard_batch(h, b); return rc; }
	*out = b;
	return CVX_OK;
	ABI_GUARD_END
}

int cvx_batch_run(cvx_handle h, cvx_batch b) {
	ABI_GUARD_BEGIN
	if (!h || !b || b->state < kUploaded) { set_err("cvx_batch_run: NULL argument / batch not uploaded"); return CVX_ERR_ARG; }
	HIP_TRY(hipSetDevice(h->device));
	RC_TRY(stage_plan(h, b, h->s_main));
	RC_TRY(stage_compute(h, b));
	RC_TRY(stage_results(h, b));
	HIP_TRY(hipStreamSynchronize(h->s_main));
	HIP_TRY(hipStreamSynchronize(h->s_post));
	return CVX_OK;
	ABI_GUARD_END
}

int cvx_batch_timing(cvx_batch b, cvx_timing *t) {
	ABI_GUARD_BEGIN
	if (!b || !t) { set_err("cvx_batch_timing: NULL argument"); return CVX_ERR_ARG; }
	*t = b->timing;
	return CVX_OK;
	ABI_GUARD_END
}

int cvx_batch_launch_info(cvx_batch b, int32_t i, cvx_launch_info *info) {
	ABI_GUARD_BEGIN
	if (!b || !info || b->state < kFinished || i < 0 || (size_t) i >= b->launches.size()) { set_err("cvx_batch_launch_info: bad index"); return CVX_ERR_ARG; }
	*info = b->launches[(size_t) i];
	return CVX_OK;
	ABI_GUARD_END
}

int cvx_batch_ops_total(cvx_batch b, uint64_t *n_ops) {
	ABI_GUARD_BEGIN
	if (!b || !n_ops || b->state < kFinished) { set_err("cvx_batch_ops_total: batch not run"); return CVX_ERR_ARG; }
	*n_ops = b->ops_total;
	return CVX_OK;
	ABI_GUARD_END
}

int cvx_batch_download(cvx_handle h, cvx_batch b, cvx_result *results, uint32_t *ops_arena,
		uint64_t ops_capacity, uint64_t *ops_used) {
	ABI_GUARD_BEGIN
	if (!h || !b || b->state < kFinished || (b->n > 0 && !results)) { set_err("cvx_batch_download: bad argument / batch not run"); return CVX_ERR_ARG; }
	HIP_TRY(hipSetDevice(h->device));
	if (ops_used) *ops_used = b->ops_total;
	static_assert(sizeof(cvx_result) == sizeof(ResultRec), "ResultRec mirrors cvx_result");
	if (b->n) memcpy(results, b->res(), (size_t) b->n * sizeof(cvx_result));
	if (b->ops_total > ops_capacity) {
		set_err("cvx_batch_download: ops arena too small (%llu needed, %llu given)",
				(unsigned long long) b->ops_total, (unsigned long long) ops_capacity);
		return CVX_ERR_CAPACITY;
	}
	if (b->ops_total) {
		if (!ops_arena) { set_err("cvx_batch_download: NULL ops arena"); return CVX_ERR_ARG; }
		RC_TRY(stage_ops(h, b));
		memcpy(ops_arena, b->h_ops.p, (size_t) b->ops_total * sizeof(uint32_t));
	}
	return CVX_OK;
	ABI_GUARD_END
}

void cvx_batch_free(cvx_handle h, cvx_batch b) {
	ABI_GUARD_BEGIN
	if (!b) return;
	if (h) (void) hipSetDevice(h->device);
	recycle_batch(h, b);
	ABI_GUARD_END_VOID
}

int cvx_align_batch(cvx_handle h, int32_t n, const cvx_tile *tiles, cvx_result *results,
		uint32_t *ops_arena, uint64_t ops_capacity, uint64_t *ops_used) {
	ABI_GUARD_BEGIN
	cvx_job j = nullptr;
	int rc = cvx_submit(h, n, tiles, &j);
	if (rc != CVX_OK) return rc;
	const cvx_result *res = nullptr;
	const uint32_t *ops = nullptr;
	uint64_t n_ops = 0;
	rc = cvx_wait(h, j, &res, &ops, &n_ops);
	if (rc == CVX_OK) {
		if (ops_used) *ops_used = n_ops;
		if (n && results) memcpy(results, res, (size_t) n * sizeof(cvx_result));
		if (n && !results) { set_err("cvx_align_batch: NULL results"); rc = CVX_ERR_ARG; }
		else if (n_ops > ops_capacity) {
			set_err("cvx_align_batch: ops arena too small (%llu needed, %llu given)",
					(unsigned long long) n_ops, (unsigned long long) ops_capacity);
			rc = CVX_ERR_CAPACITY;
		} else if (n_ops) {
			if (!ops_arena) { set_err("cvx_align_batch: NULL ops arena"); rc = CVX_ERR_ARG; }
			else memcpy(ops_arena, ops, (size_t) n_ops * sizeof(uint32_t));
		}
		cvx_job_release(h, j);
	}
	return rc;
	ABI_GUARD_END
}

/* ------------------------------------------------------------------ streaming form */

static int submit_common(cvx_handle h, int32_t n, const cvx_tile *tiles, const cvx_genome_s *genome, const uint64_t *ref_position, cvx_job *out) {
	if (!h || !out || n < 0 || (n > 0 && !tiles) || (genome && n > 0 && !ref_position)) { set_err("cvx_submit: bad argument"); return CVX_ERR_ARG; }
	*out = nullptr;
	if (genome && genome->device != h->device) { set_err("cvx_submit_windows: the genome lives on device %d, the handle on %d", genome->device, h->device); return CVX_ERR_ARG; }
	HIP_TRY(hipSetDevice(h->device));
	/* first hand the device whatever is ready to run, then spend host time on packing (a job that fails there keeps
	 * its own error; this call reports only what happens to the batch being submitted) */
	static const bool trace = getenv("CVX_SUBMIT_TRACE") != nullptr;      /* where a slow cvx_submit spends its time (stderr, calls over 5 ms) */
	const auto t0 = std::chrono::steady_clock::now();
	if (h->live.empty() && !g_deferred.empty()) g_deferred.drain();      /* nothing of this handle is in flight: outgrown blocks go back now */
	(void) pump(h, false, nullptr);
	const auto t1 = std::chrono::steady_clock::now();
	cvx_batch_s *b = acquire_batch(h);
	if (!b) return CVX_ERR_OOM;
	b->bind(h->marks);
	const auto t2 = std::chrono::steady_clock::now();
	int rc = stage_upload(h, b, n, tiles, genome, ref_position);
	const auto t3 = std::chrono::steady_clock::now();
	if (rc == CVX_OK) rc = stage_plan(h, b, h->s_io);
	if (rc != CVX_OK) { discard_batch(h, b); return rc; }
	b->in_flight = true;
	h->pending.push_back(b);
	h->live.push_back(b);
	const auto t4 = std::chrono::steady_clock::now();
	(void) pump(h, false, nullptr);
	if (trace) {
		const auto t5 = std::chrono::steady_clock::now();
		auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point c) { return std::chrono::duration<double, std::milli>(c - a).count(); };
		if (ms(t0, t5) > 5.0) fprintf(stderr, "cvx_submit: %d tiles in %.2f ms: pump %.2f, batch slot %.2f, upload stage %.2f, plan stage %.2f, pump %.2f\n", n, ms(t0, t5), ms(t0, t1), ms(t1, t2), ms(t2, t3), ms(t3, t4), ms(t4, t5));
	}
	*out = b;
	return CVX_OK;
}

int cvx_submit(cvx_handle h, int32_t n, const cvx_tile *tiles, cvx_job *out) {
	ABI_GUARD_BEGIN return submit_common(h, n, tiles, nullptr, nullptr, out); ABI_GUARD_END
}

int cvx_submit_windows(cvx_handle h, cvx_genome g, int32_t n, const cvx_tile *tiles, const uint64_t *ref_position, cvx_job *out) {
	ABI_GUARD_BEGIN
	if (!g) { set_err("cvx_submit_windows: NULL genome"); return CVX_ERR_ARG; }
	return submit_common(h, n, tiles, g, ref_position, out);
	ABI_GUARD_END
}

int cvx_wait(cvx_handle h, cvx_job j, const cvx_result **results, const uint32_t **ops, uint64_t *n_ops) {
	ABI_GUARD_BEGIN
	if (!h || !j || !j->in_flight) { set_err("cvx_wait: not a submitted job"); return CVX_ERR_ARG; }
	HIP_TRY(hipSetDevice(h->device));
	/* A job that failed (now or in an earlier call) stays valid until cvx_job_release and keeps answering with its
	 * own error; nothing of another job is ever returned in its place. */
	if (j->state != kFailed && j->state < kComputed) (void) pump(h, true, j);
	if (j->state != kFailed && j->state < kFinished) { const int rc = stage_results(h, j); if (rc != CVX_OK) (void) fail_job(j, rc); }
	if (j->state != kFailed) { const int rc = stage_ops(h, j); if (rc != CVX_OK) (void) fail_job(j, rc); }
	if (j->state == kFailed) { g_err = j->fail_msg; return j->fail_rc; }
	(void) pump(h, false, nullptr);      /* later jobs whose inputs have arrived meanwhile */
	if (results) *results = reinterpret_cast<const cvx_result *>(j->res());
	if (ops) *ops = j->h_ops.as<uint32_t>();
	if (n_ops) *n_ops = j->ops_total;
	return CVX_OK;
	ABI_GUARD_END
}

int cvx_job_window_refs(cvx_handle h, cvx_job j, const char **refs) {
	ABI_GUARD_BEGIN
	if (!h || !j || !refs || j->state < kFinished) { set_err("cvx_job_window_refs: job not finished (call cvx_wait first)"); return CVX_ERR_ARG; }
	if (!j->have_refs) { set_err("cvx_job_window_refs: not a job of cvx_submit_windows"); return CVX_ERR_ARG; }
	const char *base = j->h_refs.as<char>();
	const TileIn *tin = j->tin();
	for (int i = 0; i < j->n; ++i) refs[i] = base + (tin[i].ref_off - j->refs_base);
	return CVX_OK;
	ABI_GUARD_END
}

int cvx_job_poll(cvx_handle h, cvx_job j, int32_t *done) {
	ABI_GUARD_BEGIN
	if (!h || !j || !j->in_flight || !done) { set_err("cvx_job_poll: not a submitted job"); return CVX_ERR_ARG; }
	HIP_TRY(hipSetDevice(h->device));
	(void) pump(h, false, nullptr);          /* queue the kernels of whatever has its corridor plans back */
	*done = 0;
	if (j->state == kFailed || j->state >= kFinished) { *done = 1; return CVX_OK; }
	if (j->state >= kComputed) {
		hipError_t q = hipEventQuery(j->ev_res);
		if (q == hipSuccess) *done = 1;
		else if (q == hipErrorNotReady) (void) hipGetLastError();
		else { set_err("hipEventQuery: %s", hipGetErrorString(q)); return CVX_ERR_HIP; }
	}
	return CVX_OK;
	ABI_GUARD_END
}

int cvx_job_timing(cvx_job j, cvx_timing *t) { ABI_GUARD_BEGIN return cvx_batch_timing(j, t); ABI_GUARD_END }
int cvx_job_launch_info(cvx_job j, int32_t i, cvx_launch_info *info) { ABI_GUARD_BEGIN return cvx_batch_launch_info(j, i, info); ABI_GUARD_END }

void cvx_job_release(cvx_handle h, cvx_job j) {
	ABI_GUARD_BEGIN
	if (!j) return;
	if (h) {
		(void) hipSetDevice(h->device);
		auto it = std::find(h->pending.begin(), h->pending.end(), j);
		if (it != h->pending.end()) h->pending.erase(it);
		if ((j->state >= kPlanned && j->state < kFinished) || j->state == kFailed) (void) hipDeviceSynchronize();   /* released without waiting */
	}
	recycle_batch(h, j);
	ABI_GUARD_END_VOID
}

/* ------------------------------------------------------------------ corridor rows, host-side probe */

int cvx_corridor_rows(cvx_handle h, const cvx_tile *tile, int32_t *offset, int32_t *length) {
	ABI_GUARD_BEGIN
	if (!h || !tile || tile->qry_len < 0 || (tile->qry_len > 0 && (!offset || !length))) { set_err("cvx_corridor_rows: bad argument"); return CVX_ERR_ARG; }
	const int H = tile->qry_len;
	if (H == 0) return CVX_OK;
	if (tile->corridor_kind == CVX_CORRIDOR_ROWS) {
		if (!tile->row_offset || !tile->row_length || (tile->row_stride_bytes & 3) || tile->row_stride_bytes < 4) { set_err("cvx_corridor_rows: bad row arrays"); return CVX_ERR_ARG; }
		for (int y = 0; y < H; ++y) {
			memcpy(&offset[y], (const char *) tile->row_offset + (size_t) y * (size_t) tile->row_stride_bytes, 4);
			memcpy(&length[y], (const char *) tile->row_length + (size_t) y * (size_t) tile->row_stride_bytes, 4);
		}
		return CVX_OK;
	}
	/* the closed forms are evaluated as the product evaluates them: on the device, by the function every kernel uses for
	 * the rows of such a tile (affine_row_offset; here through expand_rows_kernel, which writes them out) */
	cvx_tile t = *tile;
	static const char dummy[1] = {0};
	t.ref = t.qry = dummy;      /* only the corridor matters here */
	t.ref_len = 0;
	std::vector<TileIn> tin;
	UploadLayout L;
	int bad = -1;
	{
		cvx_tile probe = t;      /* validate the descriptor (its bounds depend on the number of rows); no sequence is read */
		if (upload_layout(1, &probe, tin, L, &bad, false) != kLayoutOk) { set_err("cvx_corridor_rows: malformed corridor descriptor"); return CVX_ERR_ARG; }
	}
	HIP_TRY(hipSetDevice(h->device));
	RowSrc rs = L.rsrc[0];
	TileIn ti;
	memset(&ti, 0, sizeof(ti));
	ti.H = H;
	DevBuf<RowSrc> d_rs;
	DevBuf<TileIn> d_ti;
	DevBuf<RowDesc> d_rows;
	int rc = d_rs.ensure(1);
	if (rc == CVX_OK) rc = d_ti.ensure(1);
	if (rc == CVX_OK) rc = d_rows.ensure((size_t) H);
	std::vector<RowDesc> rows((size_t) H);
	hipError_t e = hipSuccess;
	if (rc == CVX_OK) {
		e = hipMemcpy(d_rs.p, &rs, sizeof(rs), hipMemcpyHostToDevice);
		if (e == hipSuccess) e = hipMemcpy(d_ti.p, &ti, sizeof(ti), hipMemcpyHostToDevice);
		if (e == hipSuccess) e = launch_expand_rows(d_rs.p, d_ti.p, nullptr, nullptr, d_rows.p, 1, true, h->s_main);
		if (e == hipSuccess) e = hipStreamSynchronize(h->s_main);
		if (e == hipSuccess) e = hipMemcpy(rows.data(), d_rows.p, (size_t) H * sizeof(RowDesc), hipMemcpyDeviceToHost);
	}
	d_rs.release(); d_ti.release(); d_rows.release();
	if (rc != CVX_OK) return rc;
	if (e != hipSuccess) { set_err("cvx_corridor_rows: %s", hipGetErrorString(e)); return CVX_ERR_HIP; }
	for (int y = 0; y < H; ++y) { offset[y] = rows[(size_t) y].off; length[y] = rows[(size_t) y].len; }
	return CVX_OK;
	ABI_GUARD_END
}

int cvx_pack_probe(int32_t n, const cvx_tile *tiles, int32_t iters, int32_t assume_page_locked, double *ms_per_iter, uint64_t *bytes_touched) {
	ABI_GUARD_BEGIN
	if (n < 0 || (n > 0 && !tiles) || iters <= 0 || !ms_per_iter) { set_err("cvx_pack_probe: bad argument"); return CVX_ERR_ARG; }
	/* what stage_upload does on the host, minus every HIP call: layout, packing into (ordinary) staging on the
	 * process's pack threads.  Nothing is aligned -- this measures the submit side, it computes nothing. */
	std::vector<uint8_t> hseq, hdelta;
	uint64_t touched = 0;
	const auto c0 = std::chrono::steady_clock::now();
	for (int it = 0; it < iters; ++it) {
		UploadLayout L;
		std::vector<TileIn> tin;
		int bad = -1;
		const int lrc = upload_layout(n, tiles, tin, L, &bad, false);
		if (lrc != kLayoutOk) { set_err("cvx_pack_probe: tile %d malformed / batch too large", bad); return CVX_ERR_ARG; }
		const bool zc_qry = assume_page_locked && L.qry_contig, zc_ref = assume_page_locked && L.ref_contig;
		if (hseq.size() < L.seq_total + 256) hseq.resize((size_t) L.seq_total + 256);
		if (hdelta.size() < L.delta_total + 256) hdelta.resize((size_t) L.delta_total + 256);
		uint64_t pack_work = L.delta_total * 9ull + (zc_qry ? 0 : L.qry_bytes) + (zc_ref ? 0 : L.ref_bytes);
		int threads = PackPool::get().size();
		if (pack_work < (8u << 20)) threads = 1;
		std::vector<RowOverflow> overflow((size_t) threads + 1);
		std::atomic<int> slot(0);
		if (pack_work > 0)
			parallel_ranges(n, L.wprefix, threads, [&](int bg, int en) {
				upload_pack(bg, en, tiles, tin, hseq.data(), hdelta.data(), L.rsrc, overflow[(size_t) slot.fetch_add(1)], !zc_qry, !zc_ref);
			});
		touched = 2 * ((zc_qry ? 0 : L.qry_bytes) + (zc_ref ? 0 : L.ref_bytes)) + L.delta_total * 9ull + (uint64_t) n * (sizeof(TileIn) + sizeof(RowSrc) + sizeof(cvx_tile));
	}
	const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - c0).count();
	*ms_per_iter = dt * 1e3 / iters;
	if (bytes_touched) *bytes_touched = touched;
	return CVX_OK;
	ABI_GUARD_END
}

}  /* extern "C" */
