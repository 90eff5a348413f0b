/*
 * cvx_rt_align.cpp -- the alignment job pipeline of libcvxalign.so (the handle and its streams: cvx_runtime.cpp).
 * A batch of tiles moves through four stages:
 *
 *   upload   host threads pack sequences + corridor rows into the batch's own pinned staging,
 *            piece by piece, each piece's DMA running under the packing of the next  (stream `io`;
 *            what travels when and from where: build_upload_schedule, cvx_host_logic.h)
 *   plan     plan_kernel, plan records back to pinned memory                          (stream `io`)
 *   compute  host: kernel class / arena offsets / LPT lists from the plan records, then the launch schedule
 *            (build_schedule, cvx_host_logic.h: list contents, one record per fill launch, stream slots, walk lanes);
 *            fill_ring_kernel per class (+ exact redo pass)                   (streams `main` + `aux`)
 *            backtrack_kernel, the finalize kernels (device-side prefix sums and result records),
 *            compact_ops_kernel, result records back to pinned memory               (stream `main`;
 *            optionally `post`, beside the next batch's fills: measured to gain nothing, see stage_compute)
 *   finish   dense ops back to pinned memory                                          (stream `io`)
 *
 * The streaming entry points (cvx_submit / cvx_wait / cvx_job_release) keep several batches in
 * flight on one handle: the upload and plan of batch k+1 and the download of batch k-1 run
 * under the kernels of batch k, and the only host waits are on events of work that was queued a
 * whole batch earlier.  The staged entry points (cvx_batch_*) and cvx_align_batch run the same
 * stages back to back.
 *
 * Beside this file: the result stages a handle runs with every job -- regions, inversion checks, text -- are called from the
 * compute, results and ops stages, a line each, and live in cvx_rt_stages.cpp; ladder jobs, whose rungs are batches that go
 * through the stages here, in cvx_rt_ladder.cpp (cvx_rt_align.h: what the two files call of each other).  What a fresh job
 * is: cvx_batch_s::begin_job (cvx_rt.h).
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

#include "cvx_qry_stage.h"
#include "cvx_rt_align.h"

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
	if (b->ladder) ladder_release(h, b);
	const bool failed = b->state == kFailed;
	b->begin_job();      /* (the caller has let go of the job: a failed one's error ends here) */
	unlist_job(h, b, kListLive);
	/* (a job that failed half-way keeps nothing worth pooling: its arenas go back to the allocator) */
	if (h && !failed && h->pool.size() < kPoolBatches) { h->pool.push_back(b); return; }
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

namespace {

/* something failed after work was queued: nothing may still be running on the arenas when they
 * go back to the allocator (or to the pool) */
void discard_batch(cvx_context *h, cvx_batch_s *b) {
	(void) hipDeviceSynchronize();
	unlist_job(h, b, kListPending | kListLive | kListClimbing);
	delete b;
}

/* ---- stage 1: pack into pinned staging and copy to the device, piece by piece (stream `io`) */
int stage_upload(cvx_context *h, cvx_batch_s *b, int32_t n, const cvx_tile *tiles,
		const cvx_genome_s *genome = nullptr, const uint64_t *ref_position = nullptr, const SegmentsIn *segs = nullptr) {
	RC_TRY(ensure_streams(h));
	UploadLayout L;
	std::vector<TileIn> tin;
	int bad = -1;
	const bool windows = genome != nullptr, segments = segs != nullptr;
	const int lrc = upload_layout(n, tiles, tin, L, &bad, windows, segments);
	if (lrc == kLayoutMalformed) { set_err("tile %d malformed", bad); return CVX_ERR_ARG; }
	if (lrc == kLayoutTooLarge) {
		set_err("%llu sequence bytes exceed one batch (4 GiB); split the batch", (unsigned long long) L.seq_total);
		return CVX_ERR_ARG;
	}
	b->begin_job();
	b->n = n;
	b->jr.bin = (h->inv_checks && genome && n > 0) ? genome->d_bin.p : nullptr;      /* (then d_win holds every tile's ref_position) */
	b->jr.L = genome ? score_windows_concat_len(genome->n_nibbles) : 0;
	b->seq_total = L.seq_total;
	b->n_rows = L.n_rows;
	/* segments: every tile's query checked against the read block and cut into the stage kernel's chunks, before anything is queued */
	SegPlan sp;
	if (segments) {
		int64_t sbad = 0;
		if (segments_plan(segs->n_reads, segs->offsets, n, segs->qry, [&](int32_t i) { return tiles[i].qry_len; },
				[&](int32_t i) { return (uint64_t) tin[(size_t) i].qry_off; }, sp, &sbad) != CVX_OK) {
			if (sbad < 0) set_err("cvx_submit_segments: the offsets of read %lld do not ascend (or span 2 GB)", (long long) (-1 - sbad));
			else set_err("cvx_submit_segments: tile %lld: read %d of %d, start %d, qry_len %d, flags %d", (long long) sbad, segs->qry[sbad].read,
					segs->n_reads, segs->qry[sbad].start, tiles[sbad].qry_len, segs->qry[sbad].flags);
			return CVX_ERR_ARG;
		}
	}
	RC_TRY(b->make_events());
	const size_t rows1 = (size_t) std::max<uint64_t>(L.arena_rows, 1);      /* closed-form corridors own no rows (RowView, cvx_types.h) */
	RC_TRY(b->h_delta.ensure((size_t) L.delta_total + 256));
	RC_TRY(b->d_delta.ensure((size_t) L.delta_total + 256));
	RC_TRY(b->d_seq.ensure((size_t) L.seq_total + 256));
	RC_TRY(b->d_rows.ensure(rows1));
	RC_TRY(ensure_tile_records(b, n));
	if (n) memcpy(b->h_tin.p, tin.data(), (size_t) n * sizeof(TileIn));

	/* which bytes travel when, and from where: build_upload_schedule (cvx_host_logic.h); here only its questions to the
	 * runtime (does a block of the caller's lie in page-locked memory?) and the issuing */
	const bool qry_pinned = L.qry_contig && in_pinned_block(tiles[0].qry, L.qry_bytes + 4);      /* (contiguous: n > 0) */
	const bool ref_pinned = L.ref_contig && in_pinned_block(tiles[0].ref, L.ref_bytes + 4);
	const uint8_t *read_block = segments && sp.read_bytes ? segs->arena + segs->offsets[0] : nullptr;
	const bool reads_pinned = read_block && in_pinned_block(read_block, sp.read_bytes + 4);
	UploadSchedule sch;
	build_upload_schedule(L, tin, n, qry_pinned, ref_pinned, std::min(h->pack_threads, PackPool::get().size()), sch, kPackThreadBytes, sp.read_bytes, reads_pinned);
	b->zero_copy_bytes = sch.zero_copy_bytes;
	if (sch.pack_seq) RC_TRY(b->h_seq.ensure((size_t) L.seq_total + 256));
	uint8_t *hseq = b->h_seq.as<uint8_t>();
	uint8_t *hdelta = b->h_delta.as<uint8_t>();
	if (sch.pack_seq) upload_zero_pads(L, hseq);
	if (sch.zero_bytes) {
		RC_TRY(b->h_zero.ensure((size_t) sch.zero_bytes));
		if (b->zero_cap != b->h_zero.cap) { memset(b->h_zero.p, 0, b->h_zero.cap); b->zero_cap = b->h_zero.cap; }
	}
	hipStream_t st = h->s_io;
	/* segments: the read block first -- as it lies in the caller's page-locked arena, or through the job's staging, each piece
	 * copied there in front of its record (its DMA runs under the copy of the next, and under the packing below) */
	if (!sch.read_copies.empty()) {
		RC_TRY(b->d_reads.ensure((size_t) sp.read_bytes + 256));
		if (!sch.zc_reads) RC_TRY(b->h_reads.ensure((size_t) sp.read_bytes + 256));
		auto stage_piece = [&](const UploadCopy &c) {
			uint8_t *hs = b->h_reads.as<uint8_t>() + c.src_off;
			const uint64_t have = std::min<uint64_t>(c.len, sp.read_bytes - c.src_off);      /* (the last record is rounded up to whole dwords) */
			memcpy(hs, read_block + c.src_off, (size_t) have);
			memset(hs + have, 0, (size_t) (c.len - have));
		};
		if (sch.read_threads > 1) PackPool::get().run((int) sch.read_copies.size(), [&](int k) { stage_piece(sch.read_copies[(size_t) k]); });
		for (const UploadCopy &c : sch.read_copies) {
			const uint8_t *src = read_block + c.src_off;
			if (c.src == kFromReadStaging) {
				if (sch.read_threads <= 1) stage_piece(c);
				src = b->h_reads.as<uint8_t>() + c.src_off;
			}
			HIP_TRY(hipMemcpyAsync(b->d_reads.p + c.dst_off, src, (size_t) c.len, hipMemcpyHostToDevice, st));
		}
	}
	const void *const from[] = { hseq, hdelta, b->h_zero.p, n && !segments ? tiles[0].qry : nullptr, n ? tiles[0].ref : nullptr };      /* UploadSrc */
	auto issue = [&](size_t r0, size_t r1) -> int {
		for (size_t r = r0; r < r1; ++r) {
			const UploadCopy &c = sch.copies[r];
			uint8_t *dst = (c.dst == kToSeq ? b->d_seq.p : b->d_delta.p) + c.dst_off;
			if (c.src == kClearOnDevice) HIP_TRY(hipMemsetAsync(dst, 0, (size_t) c.len, st));
			else HIP_TRY(hipMemcpyAsync(dst, static_cast<const uint8_t *>(from[c.src]) + c.src_off, (size_t) c.len, hipMemcpyHostToDevice, st));
		}
		return CVX_OK;
	};
	RC_TRY(issue(0, sch.n_leading));
	/* piece p's copies are queued before piece p + 1 is packed: they run under that packing */
	std::vector<RowOverflow> overflow;
	for (const UploadPiece &pc : sch.pieces) {
		upload_pack_piece(sch, pc, tiles, tin, L, hseq, hdelta, overflow);
		RC_TRY(issue(pc.rec0, pc.rec1));
	}
	if (n) HIP_TRY(hipMemcpyAsync(b->d_tin.p, b->h_tin.p, (size_t) n * sizeof(TileIn), hipMemcpyHostToDevice, st));
	if (n) {
		/* the misfits' rows (none in any corridor the reference builds), then the rows arena on the device */
		const uint64_t n_x = misfit_rows(overflow);
		b->n_rowsx = n_x;
		if (n_x) {
			RC_TRY(b->h_rowsx.ensure((size_t) n_x * sizeof(RowDesc)));
			RC_TRY(b->d_rowsx.ensure((size_t) n_x));
			RowDesc *hx = b->h_rowsx.as<RowDesc>();
			place_misfits(overflow, tin, L.rsrc, hx);
			HIP_TRY(hipMemcpyAsync(b->d_rowsx.p, hx, (size_t) n_x * sizeof(RowDesc), hipMemcpyHostToDevice, st));
		}
		memcpy(b->h_rsrc.p, L.rsrc.data(), (size_t) n * sizeof(RowSrc));
		HIP_TRY(hipMemcpyAsync(b->d_rsrc.p, b->h_rsrc.p, (size_t) n * sizeof(RowSrc), hipMemcpyHostToDevice, st));
		/* rows arena: only for the tiles whose corridors came as arrays; closed forms are evaluated where they are needed */
		if (L.arena_rows) HIP_TRY(launch_expand_rows(b->d_rsrc.p, b->d_tin.p, b->d_delta.p, b->d_rowsx.p, b->d_rows.p, n, false, st));
	}
	if ((windows || segments) && n) RC_TRY(issue(sch.n_staged, sch.copies.size()));      /* the pads the device clears itself */
	if (segments && n) {
		/* the queries: written from the read block straight into the arena, behind the block's copy and the pad clears and in
		 * front of the event the plan waits for; nothing of them ever lies on the host */
		const size_t dbytes = (size_t) n * sizeof(SegDesc), cbytes = sp.chunks.size() * sizeof(SegChunk);
		RC_TRY(b->h_segs.ensure(dbytes + cbytes + 64));
		RC_TRY(b->d_segs.ensure(dbytes + cbytes + 64));
		memcpy(b->h_segs.p, sp.desc.data(), dbytes);
		if (cbytes) memcpy(b->h_segs.as<uint8_t>() + dbytes, sp.chunks.data(), cbytes);
		HIP_TRY(hipMemcpyAsync(b->d_segs.p, b->h_segs.p, (dbytes + cbytes + 3) / 4 * 4, hipMemcpyHostToDevice, st));
		HIP_TRY(launch_stage_segments(b->d_reads.p, reinterpret_cast<const SegDesc *>(b->d_segs.p), reinterpret_cast<const SegChunk *>(b->d_segs.p + dbytes),
				(int) sp.chunks.size(), b->d_seq.p, st));
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

/* ---- stage 3's helpers */
/* the kernels' arguments of a batch; a fill launch adds its own list, chain fields and priority */
void kernel_args(const cvx_context *h, const cvx_batch_s *b, const ChainBlk *chain_blk, FillArgs &a, BacktrackArgs &ba) {
	a.seq = ba.seq = b->seq();
	a.rows = ba.rows = reinterpret_cast<const RowDesc2 *>(b->d_rows.p);
	a.rsrc = ba.rsrc = b->d_rsrc.p;
	a.tin = ba.tin = b->d_tin.p;
	a.trun = ba.trun = b->d_trun.p;
	a.tout = ba.tout = b->d_tout.p;
	ba.dirs = a.dirs = b->d_dirs.p;
	a.ops = ba.ops = b->d_regions.p;
	a.list = nullptr; a.list_n = 0;
	a.redo_count = b->d_counters.p;
	a.late_min_groups = h->tune_late_min;
	a.late_shift = h->tune_late_shift;
	a.pen_table = h->tune_pen_table;
	a.tasks = nullptr; a.chain_ticket = nullptr; a.bnd = nullptr; a.chain_out = nullptr; a.bnd_epoch = 0; a.chain_prio = 0;
	a.sp = h->sp;
	a.twin = h->scalar_twin ? 1 : 0;
	ba.chain_blk = chain_blk;
	ba.n_tiles = b->n;
}

/* the walk of lists[at, at + count) on `ws` with the lanes `w` gives it (walk_plan, cvx_host_logic.h); the long head runs
 * beside the bulk on `side` when there is one (the one walk of a whole batch), in front of it on `ws` otherwise */
int issue_walk(cvx_batch_s *b, const BacktrackArgs &ba, const WalkPlan &w, size_t at, int count, hipStream_t ws, hipStream_t side) {
	if (count <= 0) return CVX_OK;
	const int32_t *list = b->d_lists.p + at;
	const bool fork = w.n_long > 0 && side != nullptr;
	if (fork) {
		HIP_TRY(hipEventRecord(b->ev_bt0, ws));
		HIP_TRY(hipStreamWaitEvent(side, b->ev_bt0, 0));
	}
	if (w.n_long > 0) HIP_TRY(launch_backtrack(ba, list, w.n_long, w.long_lanes, fork ? side : ws));
	if (fork) HIP_TRY(hipEventRecord(b->ev_bt1, side));
	HIP_TRY(launch_backtrack(ba, list + w.n_long, count - w.n_long, w.bulk_lanes, ws));
	if (fork) HIP_TRY(hipStreamWaitEvent(ws, b->ev_bt1, 0));
	return CVX_OK;
}

/* chained tiles: tasks of every chain class, block table and tile lists in one upload on `st` (layout: build_schedule) */
int upload_chain(cvx_batch_s *b, const HostPlan &hp, const ComputeSchedule &sch, hipStream_t st) {
	RC_TRY(b->h_chain.ensure(sch.chain_bytes));
	uint8_t *hc = b->h_chain.as<uint8_t>();
	for (size_t c = 0; c < hp.chain_tasks.size(); ++c)
		if (!hp.chain_tasks[c].empty()) memcpy(hc + sch.chain_task_off[c], hp.chain_tasks[c].data(), hp.chain_tasks[c].size() * sizeof(ChainTask));
	memcpy(hc + sch.chain_blk_off, hp.chain_blk.data(), hp.chain_blk.size() * sizeof(ChainBlk));
	for (size_t c = 0; c < hp.chain_tiles.size(); ++c)
		if (!hp.chain_tiles[c].empty()) memcpy(hc + sch.chain_tile_off[c], hp.chain_tiles[c].data(), hp.chain_tiles[c].size() * sizeof(int32_t));
	RC_TRY(b->d_chain.ensure(sch.chain_bytes));
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
	HIP_TRY(hipMemcpyAsync(b->d_chain.p, hc, sch.chain_bytes, hipMemcpyHostToDevice, st));
	return CVX_OK;
}

/* a job without tiles: one zero offset per result stage, and the stage's events on the streams a job's kernels would have run on */
int compute_empty(cvx_context *h, cvx_batch_s *b, hipStream_t S_main, hipStream_t S_post) {
	if (b->jt.on) RC_TRY(b->jt.set_empty());
	if (b->jr.on) RC_TRY(b->jr.set_empty());
	HIP_TRY(hipEventRecord(b->ev[4], S_main));
	hipStream_t ps = h->overlap_post ? S_post : S_main;
	HIP_TRY(hipStreamWaitEvent(ps, b->ev[4], 0));
	HIP_TRY(hipEventRecord(b->ev[2], ps));
	HIP_TRY(hipEventRecord(b->ev[3], ps));
	HIP_TRY(hipEventRecord(b->ev_res, ps));
	b->state = kComputed;
	return CVX_OK;
}

/* the handle's knobs as the host planning (host_plan_rows) and the launch schedule (build_schedule) take them */
PlanTuning plan_tuning(const cvx_context *h) {
	PlanTuning tune;
	tune.min_slots = h->tune_min_slots; tune.max_slots = h->tune_max_slots; tune.force_wrap = h->tune_force_wrap; tune.chain_m = h->tune_chain_m;
	tune.force_generic = h->force_generic ? 1 : 0;
	tune.long_steps = h->tune_long_steps; tune.small_batch = h->tune_small_batch; tune.long_need = h->tune_long_need;
	tune.no_gangs = h->tune_gangs ? 0 : 1;
	return tune;
}

ScheduleTuning schedule_tuning(cvx_context *h, const HostPlan &hp) {
	ScheduleTuning stune;
	stune.exact_steps = h->tune_exact_steps; stune.bt_group = h->bt_group; stune.bt_per_class = h->bt_per_class; stune.overlap_post = h->overlap_post;
	stune.wide_prio = h->tune_wide_prio; stune.gang_prio = h->tune_gang_prio; stune.chain_prio = h->tune_chain_prio; stune.chain_lds_kb = h->tune_chain_lds_kb;
	/* the tail split: only with the low-priority stream to put the tails on; the automatic rule sizes a class's tail by the occupancy of
	 * the kernel its two-phase pass will launch, asked once per class and handle */
	stune.tail_tiles = h->s_tail ? h->tail_split : 0;
	stune.tail_rounds = h->tail_rounds;
	if (stune.tail_tiles == kTailAuto) {
		for (size_t c = 0; c < hp.cls.size(); ++c) {
			if (hp.cls[c].empty() || kClasses[c / 2].gang > 1) continue;
			if (h->fill_waves[c] == 0) h->fill_waves[c] = fill_two_phase_waves_per_simd(kClasses[c / 2].m, (c & 1) != 0, h->tune_pen_table != 0, h->scalar_twin);
			stune.tail_waves_per_simd[c] = std::max(0, h->fill_waves[c]);
		}
	}
	return stune;
}

/* the tiles the catch-all kernel takes: where each one's slot state lies in the scratch arena, on `st` */
int upload_generic_scratch(cvx_batch_s *b, const HostPlan &hp, hipStream_t st) {
	const std::vector<int32_t> &generic = hp.generic;
	if (generic.empty()) return CVX_OK;
	RC_TRY(b->h_goff.ensure((generic.size() + 1) * sizeof(uint64_t)));
	uint64_t *goff = b->h_goff.as<uint64_t>();
	goff[0] = 0;
	for (size_t g = 0; g < generic.size(); ++g)
		goff[g + 1] = goff[g] + (uint64_t) generic_scratch_bytes(hp.trun[(size_t) generic[g]].ring);
	RC_TRY(b->d_gscratch.ensure((size_t) goff[generic.size()] + 256));
	RC_TRY(b->d_gscratch_off.ensure(generic.size() + 1));
	HIP_TRY(hipMemcpyAsync(b->d_gscratch_off.p, goff, (generic.size() + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
	return CVX_OK;
}

/* one fill launch of the schedule on its stream `ls`, between its events `le` (LaunchEvent): behind the input copies the kernels of
 * its kind -- a split class's tail beside them on the handle's low-priority stream -- and, when every class is walked behind its own
 * fill, its walk */
int issue_fill_launch(cvx_context *h, cvx_batch_s *b, const ComputeSchedule &sch, const FillLaunch &L, const Event *le,
		const FillArgs &fa, const BacktrackArgs &ba, hipStream_t ls) {
	const bool wrap = L.wrap != 0;
	HIP_TRY(hipStreamWaitEvent(ls, b->ev[4], 0));
	HIP_TRY(hipEventRecord(le[kLevStart], ls));
	FillArgs a = fa;
	a.chain_prio = L.prio;
	if (L.kind == CVX_LAUNCH_CHAINED) {
		a.list_n = L.count;
		a.tasks = reinterpret_cast<const ChainTask *>(b->d_chain.p + sch.chain_task_off[L.slot]);
		a.chain_ticket = b->d_counters.p + 8 + L.slot;
		a.bnd = b->d_bnd.p;
		a.bnd_epoch = b->bnd_epoch;
		a.chain_out = b->d_chain_out.p;
		HIP_TRY(launch_fill(L.m, 1, wrap, kModeChain, a, L.pad_lds, ls));
		HIP_TRY(launch_chain_reduce(reinterpret_cast<const int32_t *>(b->d_chain.p + sch.chain_tile_off[L.slot]), L.info.n_tiles,
				b->d_trun.p, b->d_chain_out.p, b->d_tout.p, ls));
		HIP_TRY(hipEventRecord(le[kLevTwoPhase], ls));
	} else if (L.kind == CVX_LAUNCH_CATCH_ALL) {
		a.list = b->d_lists.p + L.list_off;
		a.list_n = L.count;
		HIP_TRY(launch_fill_generic(a, h->sse_variant, b->d_gscratch.p, b->d_gscratch_off.p, ls));
		HIP_TRY(hipEventRecord(le[kLevTwoPhase], ls));
	} else {
		/* the very long tiles of the class, exact from the first step (flagged kPadRedo), before everything else */
		a.list = b->d_lists.p + L.list_off;
		a.list_n = L.n_direct;
		if (a.list_n > 0) HIP_TRY(launch_fill(L.m, L.gang, wrap, kModeExact, a, 0, ls));
		a.list += L.n_direct;
		a.list_n = L.count - L.n_direct - L.tail_count;      /* (a split class: the head; its tail follows below) */
		if (a.list_n > 0) HIP_TRY(launch_fill(L.m, L.gang, wrap, kModeTwoPhase, a, 0, ls));
		HIP_TRY(hipEventRecord(le[kLevTwoPhase], ls));
		/* exact-tracking pass over the tiles the two-phase pass flagged (usually none) */
		if (a.list_n > 0) HIP_TRY(launch_fill(L.m, L.gang, wrap, kModeExact, a, 0, ls));
		if (L.tail_count > 0) {
			/* The tail of a split class: the same two passes over the last tail_count entries of the class's list, on the low-priority
			 * stream behind the input copies.  The device takes its workgroups where the head's launch leaves wave slots free -- from
			 * the moment the head has nothing left to dispatch -- and while the tail drains, the head's walk (below, on `ls`) has
			 * the issue slots the tail no longer uses.  Streams, events and queue priority order all of it; the kernels are the
			 * head's and know nothing of the split.  (The flag the exact pass reads is per tile and redo_count is a statistic: the
			 * head's exact pass may run beside the tail's two-phase pass.)
			 * The tail waits for the head's START event, not just for the inputs: both streams would otherwise leave the same
			 * barrier at the same moment, and in most batches the tail's workgroups -- exactly one resident round -- were then
			 * dispatched first and the head filled in behind them (the tail's start event 0.02 ms BEFORE the head's in two batches
			 * of three, the step 116.3 ms instead of 114.6; profiles/r16_tail_split.txt).  Behind the start event the head's
			 * dispatch is already under way when the low-priority queue is looked at, and the tail begins one tile's duration
			 * before the head ends, every time.  CVX_TUNE_TAIL_GATE=0: the inputs only. */
			FillArgs ta = a;
			ta.list = a.list + a.list_n;
			ta.list_n = L.tail_count;
			HIP_TRY(hipStreamWaitEvent(h->s_tail, h->tail_gate ? le[kLevStart] : b->ev[4], 0));
			HIP_TRY(hipEventRecord(le[kLevTailStart], h->s_tail));
			HIP_TRY(launch_fill(L.m, L.gang, wrap, kModeTwoPhase, ta, 0, h->s_tail));
			HIP_TRY(hipEventRecord(le[kLevTailTwoPhase], h->s_tail));
			HIP_TRY(launch_fill(L.m, L.gang, wrap, kModeExact, ta, 0, h->s_tail));
			HIP_TRY(hipEventRecord(le[kLevTailExact], h->s_tail));
		}
	}
	HIP_TRY(hipEventRecord(le[kLevExact], ls));
	if (sch.per_class) {
		const int n_head = L.bt_count - L.bt_tail_count;
		RC_TRY(issue_walk(b, ba, L.walk, L.bt_off, n_head, ls, nullptr));
		if (L.tail_count > 0) {
			/* the tail's walk behind the tail's fill, on `ls`: whatever is queued on `ls` after this launch -- the next batch's fill --
			 * stays behind all of this batch's class */
			HIP_TRY(hipStreamWaitEvent(ls, le[kLevTailExact], 0));
			RC_TRY(issue_walk(b, ba, L.walk_tail, L.bt_off + (size_t) n_head, L.bt_tail_count, ls, nullptr));
		}
	}
	HIP_TRY(hipEventRecord(le[kLevWalked], ls));      /* what everything after the fills waits for */
	return CVX_OK;
}

}  // namespace

/* ---- stage 3: host planning, then every kernel of the batch on `main` (+ aux); nothing waits.  In order:
 *   the stream set, the wait for the plan records, the run's fresh state and the result stages the handle asks for
 *   (an empty job ends here: compute_empty)
 *   host planning and the launch schedule (cvx_host_logic.h), the arenas sized by them
 *   the input copies on `main`: catch-all scratch offsets, chain tables, TileRun / TileOut, the lists; event 4
 *   the fill launches as scheduled (issue_fill_launch), each with its own events
 *   the join on `main` (or `post`); event 2
 *   the walk (unless every class had its own), finalize, compaction
 *   a ladder job's next rung, in front of the result stages when there are any; the regions and the text; event 3
 *   the result records to the host; ev_res */
int stage_compute(cvx_context *h, cvx_batch_s *b, bool streaming) {
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
	b->begin_run();
	b->jr.on = h->nm_regions;
	b->jr.checks_on = b->jr.on && b->jr.bin != nullptr && n > 0;
	b->jt.on = h->job_text;
	if (n == 0) return compute_empty(h, b, S_main, S_post);

	/* host planning: kernel class, arena offsets, work lists, then the launch schedule (cvx_host_logic.h) */
	HostPlan hp;
	const PlanTuning tune = plan_tuning(h);
	/* (a tile that gets chained needs its rows on the host: rebuilt from the step stream the batch still owns) */
	const RowSrc *rsrc = b->h_rsrc.as<RowSrc>();
	host_plan_rows(n, b->plan(), b->tin(), [&](int i, std::vector<RowDesc> &tmp) -> const RowDesc * {
		tmp.resize((size_t) std::max(b->tin()[(size_t) i].H, 1));
		expand_rows_host(rsrc[(size_t) i], b->tin()[(size_t) i].H, b->h_delta.as<uint8_t>(), b->h_rowsx.as<RowDesc>(), tmp.data());
		return tmp.data();
	}, true, tune, hp);
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
	ComputeSchedule sch;
	build_schedule(hp, b->plan(), b->tin(), n, b->n_rows, h->num_cus, schedule_tuning(h, hp), b->h_lists.as<int32_t>(), sch);
	memcpy(b->h_trun.p, hp.trun.data(), (size_t) n * sizeof(TileRun));
	memcpy(b->h_tout.p, hp.tout.data(), (size_t) n * sizeof(TileOut));      /* (with the direct-exact tiles flagged kPadRedo) */
	RC_TRY(upload_generic_scratch(b, hp, st));
	if (hp.n_chained) RC_TRY(upload_chain(b, hp, sch, st));
	HIP_TRY(hipMemcpyAsync(b->d_trun.p, b->h_trun.p, (size_t) n * sizeof(TileRun), hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemcpyAsync(b->d_tout.p, b->h_tout.p, (size_t) n * sizeof(TileOut), hipMemcpyHostToDevice, st));
	if (sch.n_listed) HIP_TRY(hipMemcpyAsync(b->d_lists.p, b->h_lists.p, sch.n_listed * sizeof(int32_t), hipMemcpyHostToDevice, st));
	/* (the batch's counters are zero: cleared when the arena was allocated and again by finalize_scan_kernel,
	 * their last reader -- a memset here would be a tiny kernel that has to find a free wave slot among
	 * the previous batch's 24 576 backtrack waves before this batch's fills may start: measured 7 ms) */
	HIP_TRY(hipEventRecord(b->ev[4], st));        /* inputs of the fills are in place */

	/* the fill launches, as scheduled: each on its stream behind the input copies, its own walk behind it (per_class) */
	FillArgs fa;
	BacktrackArgs ba;
	kernel_args(h, b, hp.n_chained ? reinterpret_cast<const ChainBlk *>(b->d_chain.p + sch.chain_blk_off) : nullptr, fa, ba);
	static_assert(kAuxStreams == 2, "StreamSlot names two side streams");
	hipStream_t fill_streams[kStreamSlots];
	fill_streams[kOnSide0] = S_aux[0]; fill_streams[kOnPost] = S_post; fill_streams[kOnMain] = st; fill_streams[kOnSide1] = S_aux[1];
	const int launches = (int) sch.launches.size();
	while (b->lev.size() < (size_t) launches * kLevPerLaunch) {
		Event e;
		HIP_TRY(e.make());
		b->lev.push_back(std::move(e));
	}
	for (int i = 0; i < launches; ++i) {
		const FillLaunch &L = sch.launches[(size_t) i];
		b->launches.push_back(L.info);
		b->launch_tail.push_back(L.tail_count);
		RC_TRY(issue_fill_launch(h, b, sch, L, &b->lev[(size_t) i * kLevPerLaunch], fa, ba, fill_streams[L.stream]));
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
	for (int i = 0; i < launches; ++i) HIP_TRY(hipStreamWaitEvent(st, b->lev[(size_t) i * kLevPerLaunch + kLevWalked], 0));
	HIP_TRY(hipEventRecord(b->ev[2], st));

	/* backtrack (unless every class was walked behind its own fill), device-side result records + prefix sums, ops compaction */
	if (!sch.per_class) RC_TRY(issue_walk(b, ba, sch.walk, sch.bt_begin, sch.n_walk, st, S_aux[0]));
	ResultRec *d_rec = reinterpret_cast<ResultRec *>(b->d_res.p);
	BatchSummary *d_sum = reinterpret_cast<BatchSummary *>(b->d_res.p + (size_t) n * sizeof(ResultRec));
	HIP_TRY(launch_finalize(b->d_tout.p, b->d_plan.p, b->d_dstoff.p, b->d_dstoff.p + n, d_rec, d_sum, b->d_counters.p, n, b->dense_cap, st));
	HIP_TRY(launch_compact(b->d_regions.p, b->d_trun.p, b->d_tout.p, b->d_dstoff.p, b->d_dense.p, n, b->dense_cap, st));
	if (b->jr.on || b->jt.on) {
		/* A rung of a ladder job whose handle runs stages behind the compaction: the climb reads result statuses only, so the
		 * decision kernel, the next rung's plan and their read-back go in FRONT of this rung's regions, checks and text -- the
		 * host has the next rung's plan in hand while the device still writes this rung's strings. */
		cvx_batch_s *root = b->ladder ? b : b->ladder_root;
		if (root && root->ladder && !root->ladder->next && !root->ladder->done) {
			HIP_TRY(hipEventRecord(b->ev_rec, st));
			RC_TRY(ladder_queue_next(h, root, b, (int) root->ladder->rungs.size(), true));
		}
	}
	if (b->jr.on) RC_TRY(b->jr.queue(b, st));      /* (inside the compute stage's timing: ev[3] below) */
	if (b->jt.on) RC_TRY(b->jt.queue(b, st, false, h->tune_job_text_cap));      /* (as is this) */
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
	if (b->state < kComputed) { set_err("internal: results requested from a batch whose kernels were never queued (state %d)", b->state); return CVX_ERR_ARG; }
	HIP_TRY(hipEventSynchronize(b->ev_res));
	if (b->n == 0) { b->ops_total = 0; b->state = kFinished; return CVX_OK; }
	const BatchSummary *s = b->summary();
	b->ops_total = s->ops_total;
	b->jr.take_total(b->n);
	b->jt.take_total(b->n, h->scalar_twin);
	const int launches = b->timing.n_fill_launches;
	for (int i = 0; i < launches; ++i) {
		const Event *le = &b->lev[(size_t) i * kLevPerLaunch];
		b->launches[(size_t) i].ms = ev_ms(le[kLevStart], le[kLevTwoPhase]);
		/* a split class: one record, from the head's start to the later of the two two-phase ends */
		if (b->launch_tail[(size_t) i] > 0) b->launches[(size_t) i].ms = std::max(b->launches[(size_t) i].ms, ev_ms(le[kLevStart], le[kLevTailTwoPhase]));
	}
	b->timing.plan_ms = ev_ms(b->ev[0], b->ev[1]);
	/* fill = until the last fill class has finished its exact pass; backtrack = what is left of the compute stage (when every
	 * class is walked behind its own fill, the walks of the early classes lie inside `fill`: the two still add up) */
	float fill_end = 0.0f;
	for (int i = 0; i < launches; ++i) {
		const Event *le = &b->lev[(size_t) i * kLevPerLaunch];
		fill_end = std::max(fill_end, ev_ms(b->ev[4], le[kLevExact]));
		if (b->launch_tail[(size_t) i] > 0) {      /* (the head's walk then lies inside `fill`: it runs while the tail still fills) */
			fill_end = std::max(fill_end, ev_ms(b->ev[4], le[kLevTailExact]));
			if (h->tail_trace)
				fprintf(stderr, "cvx tail split: launch %d m=%d tiles=%d tail=%d  head two-phase end %.3f exact end %.3f  tail start %.3f two-phase end %.3f exact end %.3f  walked %.3f ms after the launch's start\n",
						i, b->launches[(size_t) i].slots_per_lane, b->launches[(size_t) i].n_tiles, b->launch_tail[(size_t) i],
						ev_ms(le[kLevStart], le[kLevTwoPhase]), ev_ms(le[kLevStart], le[kLevExact]), ev_ms(le[kLevStart], le[kLevTailStart]),
						ev_ms(le[kLevStart], le[kLevTailTwoPhase]), ev_ms(le[kLevStart], le[kLevTailExact]), ev_ms(le[kLevStart], le[kLevWalked]));
		}
	}
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
	/* the result stages' arenas ride in front of the dense ops, under the one wait below */
	RC_TRY(b->jr.fetch(h, b));
	RC_TRY(b->jt.fetch(h, b));
	if (b->ops_total) {
		RC_TRY(b->h_ops.ensure((size_t) b->ops_total * sizeof(uint32_t)));
		/* The wait below is for the whole io stream, on purpose: it already carries the upload and corridor analysis of the
		 * job submitted last, and returning only when those are done paces the caller -- it submits its next batch one
		 * step later, so that exactly one corridor analysis runs beside each fill (beside a fill it takes most of the
		 * fill's duration; two of them queued under one fill finish late and the next fill starts late: measured 150
		 * instead of 124 ms per step with an event right behind the copy). */
		HIP_TRY(hipMemcpyAsync(b->h_ops.p, b->d_dense.p, (size_t) b->ops_total * sizeof(uint32_t), hipMemcpyDeviceToHost, h->s_io));
		/* Round 4 tried to drop the pacing for closed-form batches (their corridor analysis reads nothing: 2.3 ms alone): over
		 * 3 steps of 24 576 tiles the event-only form measured the same, over the driver's 20 steps of 49 152 tiles it costs
		 * 146.5 instead of 118.7 ms per step (gpurun_out/r04g/pacing.txt) -- the analysis is starved beside a fill whatever it
		 * reads (70-100 ms), and two of them queued under one fill still delay the fill after next.  The stream wait stays. */
		HIP_TRY(hipStreamSynchronize(h->s_io));
	}
	b->have_ops = true;
	return CVX_OK;
}

namespace {

/* queue the compute stage of every submitted batch whose plan records have arrived (all of them,
 * up to `upto`, when `block`): keeps the device one batch ahead of the host */
int pump(cvx_context *h, bool block, const cvx_batch_s *upto) {
	if (!h->climbing.empty()) ladder_pump(h);
	while (!h->pending.empty()) {
		cvx_batch_s *b = h->pending.front();
		const int fired = block ? 1 : event_fired(b->ev_in);
		if (fired == 0) break;
		h->pending.erase(h->pending.begin());
		if (fired < 0) { (void) fail_job(b, CVX_ERR_HIP); continue; }
		/* a failure (say, the direction arena of a multi-GB batch does not fit beside the batches in flight) belongs
		 * to THIS job: it is recorded on it and reported by its own cvx_wait, never against another job's call */
		const int rc = stage_compute(h, b, true);
		if (rc != CVX_OK) (void) fail_job(b, rc);
		else if (b->ladder) {      /* rung 1 of a ladder job is queued: its decision kernel and the next rung's plan go right behind it */
			h->climbing.push_back(b);
			ladder_advance(h, b, false);
		}
		if (upto && b == upto) break;
	}
	return CVX_OK;
}

/* what cvx_stage_segments and cvx_stage_segments_host share: the arguments checked, the strings laid out back to back
 * (*used, qry_off) and planned; CVX_ERR_CAPACITY when out is too small for them */
int stage_segments_plan(const char *who, int32_t n_reads, const uint8_t *arena, const uint64_t *offsets, int32_t n, const cvx_read_segment *seg,
		const int32_t *len, const uint8_t *out, uint64_t cap, uint64_t *qry_off, uint64_t *used, SegPlan &sp) {
	if (!used || n_reads < 0 || n < 0 || !offsets || (n_reads > 0 && !arena) || (n > 0 && (!seg || !len || !qry_off)) || (cap > 0 && !out)) {
		set_err("%s: bad argument", who);
		return CVX_ERR_ARG;
	}
	*used = 0;
	int64_t bad = 0;
	std::vector<uint64_t> dst((size_t) n + 1, 0);
	for (int32_t i = 0; i < n; ++i) dst[(size_t) i + 1] = dst[(size_t) i] + (uint64_t) std::max(len[i], 0);
	if (segments_plan(n_reads, offsets, n, seg, [&](int32_t i) { return len[i]; }, [&](int32_t i) { return dst[(size_t) i]; }, sp, &bad) != CVX_OK) {
		if (bad < 0) set_err("%s: the offsets of read %lld do not ascend (or span 2 GB)", who, (long long) (-1 - bad));
		else set_err("%s: string %lld: read %d of %d, start %d, length %d, flags %d", who, (long long) bad, seg[bad].read, n_reads, seg[bad].start, len[bad], seg[bad].flags);
		return CVX_ERR_ARG;
	}
	*used = sp.seg_bytes;
	for (int32_t i = 0; i < n; ++i) qry_off[i] = dst[(size_t) i];
	if (cap < sp.seg_bytes) { set_err("%s: %llu bytes needed, %llu given", who, (unsigned long long) sp.seg_bytes, (unsigned long long) cap); return CVX_ERR_CAPACITY; }
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
	*t = (b->ladder && b->ladder->merged) ? b->ladder->timing : b->timing;
	return CVX_OK;
	ABI_GUARD_END
}

int cvx_batch_launch_info(cvx_batch b, int32_t i, cvx_launch_info *info) {
	ABI_GUARD_BEGIN
	const std::vector<cvx_launch_info> *ls = b ? ((b->ladder && b->ladder->merged) ? &b->ladder->launches : &b->launches) : nullptr;
	if (!b || !info || b->state < kFinished || i < 0 || (size_t) i >= ls->size()) { set_err("cvx_batch_launch_info: bad index"); return CVX_ERR_ARG; }
	*info = (*ls)[(size_t) i];
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

int cvx_batch_summary(cvx_batch b, uint64_t *ops_total, int32_t *n_valid, int32_t *n_redone) {
	ABI_GUARD_BEGIN
	if (!b || !ops_total || !n_valid || !n_redone || b->state < kFinished) { set_err("cvx_batch_summary: NULL argument / batch not run"); return CVX_ERR_ARG; }
	*ops_total = 0; *n_valid = 0; *n_redone = 0;
	if (b->n == 0) return CVX_OK;
	const BatchSummary *s = b->summary();
	*ops_total = s->ops_total; *n_valid = s->n_valid; *n_redone = s->n_redone;
	return CVX_OK;
	ABI_GUARD_END
}

int cvx_batch_plan(cvx_batch b, int32_t first, int32_t count, cvx_tile_plan *out) {
	ABI_GUARD_BEGIN
	static_assert(sizeof(cvx_tile_plan) == sizeof(TilePlan), "cvx_tile_plan mirrors TilePlan");
	if (!b || b->state < kFinished || first < 0 || count < 0 || (int64_t) first + count > b->n || (count > 0 && !out)) { set_err("cvx_batch_plan: bad range / batch not run"); return CVX_ERR_ARG; }
	if (count) memcpy(out, b->plan() + first, (size_t) count * sizeof(TilePlan));
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

}  /* extern "C" */

/* ------------------------------------------------------------------ streaming form */

int submit_common(cvx_handle h, int32_t n, const cvx_tile *tiles, const cvx_genome_s *genome, const uint64_t *ref_position, cvx_job *out,
		const SegmentsIn *segs, const cvx_ladder *ladders, int max_rungs) {
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
	int rc = stage_upload(h, b, n, tiles, genome, ref_position, segs);
	const auto t3 = std::chrono::steady_clock::now();
	if (rc == CVX_OK && ladders) {
		/* a ladder job: the tiles' ladders go up behind the batch's inputs, in front of the event its compute stage waits for */
		LadderState *L = new (std::nothrow) LadderState();
		if (!L) rc = CVX_ERR_OOM;
		else {
			L->max_rungs = max_rungs;
			L->rungs.push_back(b);
			b->ladder = L;
			const size_t bytes = (size_t) std::max(n, 1) * sizeof(cvx_ladder);
			rc = b->h_lad.ensure(bytes);
			if (rc == CVX_OK) rc = b->d_lad.ensure((size_t) std::max(n, 1));
			if (rc == CVX_OK && n) {
				memcpy(b->h_lad.p, ladders, (size_t) n * sizeof(cvx_ladder));
				hipError_t e = hipMemcpyAsync(b->d_lad.p, b->h_lad.p, (size_t) n * sizeof(cvx_ladder), hipMemcpyHostToDevice, h->s_io);
				if (e != hipSuccess) { set_err("cvx_submit_ladder: %s", hipGetErrorString(e)); rc = CVX_ERR_HIP; }
			}
		}
	}
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

extern "C" {

int cvx_submit(cvx_handle h, int32_t n, const cvx_tile *tiles, cvx_job *out) {
	ABI_GUARD_BEGIN return submit_common(h, n, tiles, nullptr, nullptr, out); ABI_GUARD_END
}

int cvx_submit_windows(cvx_handle h, cvx_genome g, int32_t n, const cvx_tile *tiles, const uint64_t *ref_position, cvx_job *out) {
	ABI_GUARD_BEGIN
	if (!g) { set_err("cvx_submit_windows: NULL genome"); return CVX_ERR_ARG; }
	return submit_common(h, n, tiles, g, ref_position, out);
	ABI_GUARD_END
}

int cvx_submit_segments(cvx_handle h, cvx_genome g, int32_t n, const cvx_tile *tiles, const uint64_t *ref_position,
		int32_t n_reads, const uint8_t *arena, const uint64_t *offsets, const cvx_read_segment *qry, cvx_job *out) {
	ABI_GUARD_BEGIN
	if (n_reads < 0 || !offsets || (n_reads > 0 && !arena) || (n > 0 && !qry) || (!g && ref_position)) { set_err("cvx_submit_segments: bad argument"); return CVX_ERR_ARG; }
	const SegmentsIn segs = { n_reads, arena, offsets, qry };
	return submit_common(h, n, tiles, g, ref_position, out, &segs);
	ABI_GUARD_END
}

int cvx_job_zero_copy_bytes(cvx_job j, uint64_t *bytes) {
	ABI_GUARD_BEGIN
	if (!j || !bytes || j->state < kUploaded) { set_err("cvx_job_zero_copy_bytes: not a submitted job"); return CVX_ERR_ARG; }
	*bytes = j->zero_copy_bytes;
	return CVX_OK;
	ABI_GUARD_END
}

/* the kernel alone: the strings back to back in a device arena of their own, and back (nothing here is on the path of a job,
 * so the buffers are the call's own) */
static int stage_segments_run(cvx_handle h, const SegPlan &sp, const uint8_t *arena, const uint64_t *offsets, int32_t n, uint8_t *out) {
	static const char who[] = "cvx_stage_segments";
	const size_t dbytes = (size_t) n * sizeof(SegDesc), cbytes = sp.chunks.size() * sizeof(SegChunk);
	DevBuf<uint8_t> d_reads, d_segs, d_out;
	Event e0, e1;
	RC_TRY(d_reads.ensure((size_t) sp.read_bytes + 256));
	RC_TRY(d_segs.ensure(dbytes + cbytes + 64));
	RC_TRY(d_out.ensure((size_t) sp.seg_bytes + 256));
	hipStream_t st = h->s_main;
	HIP_TRY_IN(who, e0.make());
	HIP_TRY_IN(who, e1.make());
	HIP_TRY_IN(who, hipMemcpyAsync(d_reads.p, arena + offsets[0], (size_t) sp.read_bytes, hipMemcpyHostToDevice, st));
	HIP_TRY_IN(who, hipMemcpyAsync(d_segs.p, sp.desc.data(), dbytes, hipMemcpyHostToDevice, st));
	HIP_TRY_IN(who, hipMemcpyAsync(d_segs.p + dbytes, sp.chunks.data(), cbytes, hipMemcpyHostToDevice, st));
	HIP_TRY_IN(who, hipEventRecord(e0, st));
	HIP_TRY_IN(who, launch_stage_segments(d_reads.p, reinterpret_cast<const SegDesc *>(d_segs.p), reinterpret_cast<const SegChunk *>(d_segs.p + dbytes),
			(int) sp.chunks.size(), d_out.p, st));
	HIP_TRY_IN(who, hipEventRecord(e1, st));
	HIP_TRY_IN(who, hipMemcpyAsync(out, d_out.p, (size_t) sp.seg_bytes, hipMemcpyDeviceToHost, st));
	HIP_TRY_IN(who, hipStreamSynchronize(st));
	h->segments_kernel_ms = ev_ms(e0, e1);
	return CVX_OK;
}

int cvx_stage_segments(cvx_handle h, int32_t n_reads, const uint8_t *arena, const uint64_t *offsets, int32_t n,
		const cvx_read_segment *seg, const int32_t *len, uint8_t *out, uint64_t cap, uint64_t *qry_off, uint64_t *used) {
	ABI_GUARD_BEGIN
	if (!h) { set_err("cvx_stage_segments: bad argument"); return CVX_ERR_ARG; }
	SegPlan sp;
	RC_TRY(stage_segments_plan("cvx_stage_segments", n_reads, arena, offsets, n, seg, len, out, cap, qry_off, used, sp));
	if (sp.chunks.empty()) return CVX_OK;
	HIP_TRY(hipSetDevice(h->device));
	RC_TRY(ensure_streams(h));
	const int rc = stage_segments_run(h, sp, arena, offsets, n, out);
	if (rc == CVX_ERR_HIP) (void) hipGetLastError();      /* (a HIP call of the run failed: the next call starts clean) */
	return rc;
	ABI_GUARD_END
}

int cvx_stage_segments_host(int32_t n_reads, const uint8_t *arena, const uint64_t *offsets, int32_t n,
		const cvx_read_segment *seg, const int32_t *len, uint8_t *out, uint64_t cap, uint64_t *qry_off, uint64_t *used) {
	ABI_GUARD_BEGIN
	SegPlan sp;
	RC_TRY(stage_segments_plan("cvx_stage_segments_host", n_reads, arena, offsets, n, seg, len, out, cap, qry_off, used, sp));
	if (sp.seg_bytes > 0) stage_segments_host(arena + offsets[0], sp.desc, out);
	return CVX_OK;
	ABI_GUARD_END
}

int cvx_wait(cvx_handle h, cvx_job j, const cvx_result **results, const uint32_t **ops, uint64_t *n_ops) {
	ABI_GUARD_BEGIN
	if (!h || !j || !j->in_flight) { set_err("cvx_wait: not a submitted job"); return CVX_ERR_ARG; }
	HIP_TRY(hipSetDevice(h->device));
	/* A job that failed (now or in an earlier call) stays valid until cvx_job_release and keeps answering with its
	 * own error; nothing of another job is ever returned in its place. */
	if (j->state != kFailed && j->state < kComputed) (void) pump(h, true, j);
	if (j->ladder) {
		/* a ladder job: the rungs still to come, each behind the blocking wait for its list and plan records, then all their results merged */
		if (j->state != kFailed) ladder_advance(h, j, true);
		if (j->state != kFailed) { const int rc = ladder_finish(h, j); if (rc != CVX_OK) (void) fail_job(j, rc); }
	} else {
		if (j->state != kFailed && j->state < kFinished) { const int rc = stage_results(h, j); if (rc != CVX_OK) (void) fail_job(j, rc); }
		if (j->state != kFailed) { const int rc = stage_ops(h, j); if (rc != CVX_OK) (void) fail_job(j, rc); }
	}
	if (j->state == kFailed) { g_err = j->fail_msg; return j->fail_rc; }
	(void) pump(h, false, nullptr);      /* later jobs whose inputs have arrived meanwhile */
	if (results) *results = reinterpret_cast<const cvx_result *>(j->ladder ? j->h_lres.as<ResultRec>() : j->res());
	if (ops) *ops = j->ladder ? j->h_lops.as<uint32_t>() : j->h_ops.as<uint32_t>();
	if (n_ops) *n_ops = j->ladder ? j->ladder->ops_total : j->ops_total;
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
	if (j->state < kComputed) return CVX_OK;
	/* a ladder job: done when no rung is to come and the last one's records are on the host */
	if (j->ladder && !j->ladder->done) return CVX_OK;
	const int fired = event_fired(j->ladder ? j->ladder->rungs.back()->ev_res : j->ev_res);
	if (fired < 0) return CVX_ERR_HIP;
	*done = fired;
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
		unlist_job(h, j, kListPending);
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
	static const char who[] = "cvx_corridor_rows";
	std::vector<RowDesc> rows((size_t) H);
	DevBuf<RowSrc> d_rs;
	DevBuf<TileIn> d_ti;
	DevBuf<RowDesc> d_rows;
	RC_TRY(d_rs.ensure(1));
	RC_TRY(d_ti.ensure(1));
	RC_TRY(d_rows.ensure((size_t) H));
	HIP_TRY_IN(who, hipMemcpy(d_rs.p, &rs, sizeof(rs), hipMemcpyHostToDevice));
	HIP_TRY_IN(who, hipMemcpy(d_ti.p, &ti, sizeof(ti), hipMemcpyHostToDevice));
	HIP_TRY_IN(who, launch_expand_rows(d_rs.p, d_ti.p, nullptr, nullptr, d_rows.p, 1, true, h->s_main));
	HIP_TRY_IN(who, hipStreamSynchronize(h->s_main));
	HIP_TRY_IN(who, hipMemcpy(rows.data(), d_rows.p, (size_t) H * sizeof(RowDesc), hipMemcpyDeviceToHost));
	for (int y = 0; y < H; ++y) { offset[y] = rows[(size_t) y].off; length[y] = rows[(size_t) y].len; }
	return CVX_OK;
	ABI_GUARD_END
}

int cvx_pack_probe(int32_t n, const cvx_tile *tiles, int32_t iters, int32_t assume_page_locked, double *ms_per_iter, uint64_t *bytes_touched) {
	ABI_GUARD_BEGIN
	if (n < 0 || (n > 0 && !tiles) || iters <= 0 || !ms_per_iter) { set_err("cvx_pack_probe: bad argument"); return CVX_ERR_ARG; }
	/* what stage_upload does on the host, minus every HIP call: layout, the upload schedule, its pieces packed into
	 * (ordinary) staging on the process's pack threads.  Nothing is aligned -- this measures the submit side, it computes nothing. */
	std::vector<uint8_t> hseq, hdelta;
	uint64_t touched = 0;
	const auto c0 = std::chrono::steady_clock::now();
	for (int it = 0; it < iters; ++it) {
		UploadLayout L;
		std::vector<TileIn> tin;
		int bad = -1;
		const int lrc = upload_layout(n, tiles, tin, L, &bad, false);
		if (lrc != kLayoutOk) { set_err("cvx_pack_probe: tile %d malformed / batch too large", bad); return CVX_ERR_ARG; }
		UploadSchedule sch;
		build_upload_schedule(L, tin, n, assume_page_locked != 0, assume_page_locked != 0, PackPool::get().size(), sch);
		if (hseq.size() < L.seq_total + 256) hseq.resize((size_t) L.seq_total + 256);
		if (hdelta.size() < L.delta_total + 256) hdelta.resize((size_t) L.delta_total + 256);
		std::vector<RowOverflow> overflow;
		for (const UploadPiece &pc : sch.pieces) upload_pack_piece(sch, pc, tiles, tin, L, hseq.data(), hdelta.data(), overflow);
		touched = 2 * ((sch.zc_qry ? 0 : L.qry_bytes) + (sch.zc_ref ? 0 : L.ref_bytes)) + L.delta_total * 9ull + (uint64_t) n * (sizeof(TileIn) + sizeof(RowSrc) + sizeof(cvx_tile));
	}
	const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - c0).count();
	*ms_per_iter = dt * 1e3 / iters;
	if (bytes_touched) *bytes_touched = touched;
	return CVX_OK;
	ABI_GUARD_END
}

}  /* extern "C" */
