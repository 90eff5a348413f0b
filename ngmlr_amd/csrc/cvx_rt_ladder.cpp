/*
 * cvx_rt_ladder.cpp -- ladder jobs (cvx_submit_ladder, cvx_submit_ladder_ex): a rung is the plan -> schedule -> fill -> walk ->
 * records cycle of a job run again, over the tiles ladder_next_kernel found climbing.  Rung r + 1 is a batch of its own from the
 * handle's pool (its own plan, lists, direction words, result block, ops: nothing of rung r is overwritten, so nothing has to wait
 * for rung r's readers) that reads rung 1's sequence arena and goes through the pipeline's compute, results and ops stages
 * (cvx_rt_align.cpp; what the two files call of each other: cvx_rt_align.h).  Order: the kernel waits, on the device, for the
 * event behind rung r's result records; the host waits for nothing but the event behind the next rung's list and plan records --
 * queried from pump, blocking only inside cvx_wait.
 */
#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

#include "cvx_ladder.h"
#include "cvx_ladder_logic.h"
#include "cvx_ladder_merge.h"
#include "cvx_rt_align.h"

/* a ladder job leaves: its later rungs' batches go where the job goes (the pool, with their arenas, or the allocator) */
void ladder_release(cvx_context *h, cvx_batch_s *root) {
	LadderState *L = root->ladder;
	if (!L) return;
	unlist_job(h, root, kListClimbing);
	root->ladder = nullptr;
	if (L->next) L->rungs.push_back(L->next);
	for (size_t r = 1; r < L->rungs.size(); ++r) {
		cvx_batch_s *c = L->rungs[r];
		c->ladder_root = nullptr;
		if (root->state == kFailed) c->state = kFailed;
		recycle_batch(h, c);
	}
	delete L;
}

/* a ladder job is deleted (cvx_destroy, a failed submit): the later rungs' batches go back to the allocator with it */
void ladder_drop(cvx_batch_s *root) {
	LadderState *L = root->ladder;
	root->ladder = nullptr;
	if (!L) return;
	if (L->next) L->rungs.push_back(L->next);
	for (size_t r = 1; r < L->rungs.size(); ++r) delete L->rungs[r];
	delete L;
}

/* behind rung `prev` (rung m, computed) of `root`: the decision kernel, the plan of the tiles it lists, and list, tile records,
 * corridors and plan records on their way to the host; L->next is the batch they belong to */
int ladder_queue_next(cvx_context *h, cvx_batch_s *root, cvx_batch_s *prev, int m, bool inline_) {
	LadderState *L = root->ladder;
	const int np = prev->n;
	if (np <= 0 || m >= L->max_rungs) { L->done = true; return CVX_OK; }
	cvx_batch_s *c = acquire_batch(h);
	if (!c) { set_err("cvx_submit_ladder: no memory for rung %d", m + 1); return CVX_ERR_OOM; }
	c->bind(h->marks);
	c->begin_job();      /* (n stays 0 until the list is back; the rung's compute stage sets its stages from the handle, like any job's) */
	c->jr.bin = root->jr.bin; c->jr.L = root->jr.L;      /* the job's genome: the rung's regions get their checks */
	c->ladder_root = root;
	L->next = c;      /* (from here on the batch leaves with the job, whatever fails) */
	RC_TRY(c->make_events());
	const size_t n1 = (size_t) np;
	RC_TRY(c->h_lhead.ensure((n1 + 1) * sizeof(int32_t)));
	RC_TRY(c->d_lhead.ensure(n1 + 1));
	RC_TRY(c->d_rows.ensure(1));      /* closed forms own no rows */
	RC_TRY(ensure_tile_records(c, np));
	if (c->jr.bin) RC_TRY(c->d_win.ensure(n1));
	hipStream_t st = h->s_main;
	/* rung m's records are final: behind their copy to the host, or (queued from inside rung m's compute stage, in front of its
	 * stages) behind the event right behind the records and the compaction */
	HIP_TRY(hipStreamWaitEvent(st, inline_ ? prev->ev_rec : prev->ev_res, 0));
	LadderNextArgs a;
	a.res = reinterpret_cast<const ResultRec *>(prev->d_res.p);
	a.prev_idx = prev == root ? nullptr : prev->d_lhead.p + 1;
	a.tin0 = root->d_tin.p;
	a.lad = root->d_lad.p;
	a.n_prev = np;
	a.m = m;
	a.rsrc = c->d_rsrc.p; a.tin = c->d_tin.p; a.head = c->d_lhead.p;
	a.win0 = c->jr.bin ? root->d_win.p : nullptr;
	a.win = c->jr.bin ? c->d_win.p : nullptr;
	HIP_TRY(launch_ladder_next(a, st));
	HIP_TRY(hipEventRecord(c->ev[0], st));
	HIP_TRY(launch_plan(c->d_rows.p, c->d_rsrc.p, c->d_tin.p, c->d_plan.p, np, root->n ? root->n_rows / (uint64_t) root->n : 0, h->max_matrix_mb, st));
	HIP_TRY(hipMemcpyAsync(c->h_plan.p, c->d_plan.p, n1 * sizeof(TilePlan), hipMemcpyDeviceToHost, st));
	HIP_TRY(hipEventRecord(c->ev[1], st));
	HIP_TRY(hipMemcpyAsync(c->h_lhead.p, c->d_lhead.p, (n1 + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, st));
	HIP_TRY(hipMemcpyAsync(c->h_tin.p, c->d_tin.p, n1 * sizeof(TileIn), hipMemcpyDeviceToHost, st));
	HIP_TRY(hipMemcpyAsync(c->h_rsrc.p, c->d_rsrc.p, n1 * sizeof(RowSrc), hipMemcpyDeviceToHost, st));
	HIP_TRY(hipEventRecord(c->ev_in, st));
	c->state = kPlanned;
	return CVX_OK;
}

/* the ladder of `root` as far as the device has answered (block: to its end); a failure is the job's */
void ladder_advance(cvx_context *h, cvx_batch_s *root, bool block) {
	LadderState *L = root->ladder;
	while (root->state != kFailed && !L->done) {
		int rc = CVX_OK;
		if (!L->next) {
			rc = ladder_queue_next(h, root, L->rungs.back(), (int) L->rungs.size(), false);
			if (rc != CVX_OK) { (void) fail_job(root, rc); break; }
			continue;
		}
		cvx_batch_s *c = L->next;
		if (!block) {
			const int fired = event_fired(c->ev_in);
			if (fired == 0) return;
			if (fired < 0) { (void) fail_job(root, CVX_ERR_HIP); break; }
		} else {
			hipError_t q = hipEventSynchronize(c->ev_in);
			if (q != hipSuccess) { set_err("hipEventSynchronize: %s", hipGetErrorString(q)); (void) fail_job(root, CVX_ERR_HIP); break; }
		}
		const int count = c->h_lhead.as<int32_t>()[0];
		L->next = nullptr;
		if (count <= 0) {      /* nobody climbs: the job ends (what was queued for the batch has run: its event is behind all of it) */
			c->ladder_root = nullptr;
			recycle_batch(h, c);
			L->done = true;
			break;
		}
		c->n = count;
		c->n_rows = 0;
		for (int i = 0; i < count; ++i) c->n_rows += (uint64_t) c->tin()[(size_t) i].H;
		L->rungs.push_back(c);
		rc = stage_compute(h, c, true);
		if (rc != CVX_OK) { (void) fail_job(root, rc); break; }
		if ((int) L->rungs.size() >= kLadderMaxRungs) L->done = true;
	}
	if (root->state == kFailed) L->done = true;
	if (L->done) unlist_job(h, root, kListClimbing);
}

/* every climbing job as far as it has come, without waiting */
void ladder_pump(cvx_context *h) {
	const std::vector<cvx_batch_s *> jobs = h->climbing;      /* (ladder_advance takes finished ladders off the list) */
	for (cvx_batch_s *root : jobs) ladder_advance(h, root, false);
}

namespace {

/* What the rungs' stages brought back (regions with their end states and checks, text records and strings; every rung's own
 * stage_results / stage_ops have run), merged for the job: per tile the reporting rung's, in tile order, offsets rebased into
 * one dense arena each (ladder_merge_plan, cvx_ladder_merge.h).  A twin handle's CVX_NOT_WRITTEN fields are already in every
 * rung's records (stage_results) and travel with them. */
int ladder_merge_stages(cvx_batch_s *root, const std::vector<int32_t> &rung_of, const std::vector<int32_t> &at) {
	LadderState *L = root->ladder;
	const int n = root->n;
	const int32_t n_rungs = (int32_t) L->rungs.size();
	std::vector<const uint64_t *> off((size_t) n_rungs);
	std::vector<const void *> rec((size_t) n_rungs);
	std::vector<int32_t> rn((size_t) n_rungs);
	std::vector<LadderSpan> spans;
	for (int32_t r = 0; r < n_rungs; ++r) rn[(size_t) r] = L->rungs[(size_t) r]->n;
	L->jr_rewrites = L->jt_rewrites = 0;
	if (root->jr.on) {
		for (int32_t r = 0; r < n_rungs; ++r) {
			const JobRegions &c = L->rungs[(size_t) r]->jr;
			if (!c.on) { set_err("internal: rung %d of a regions job ran without the finder", r + 1); return CVX_ERR_HIP; }
			off[(size_t) r] = c.h_off.as<uint64_t>();
			rec[(size_t) r] = c.h_open.p;
			L->jr_rewrites += c.rewrites;
		}
		L->jr_off.assign((size_t) n + 1, 0);
		if (!ladder_merge_plan(n, rung_of.data(), at.data(), n_rungs, off.data(), rn.data(), L->jr_off.data(), spans)) {
			set_err("internal: the region offsets of a ladder job's rungs do not merge");
			return CVX_ERR_HIP;
		}
		const uint64_t total = L->jr_off[(size_t) n];
		L->jr_reg.resize((size_t) total);
		L->jr_chk.resize(root->jr.checks_on ? (size_t) total : 0);
		for (const LadderSpan &s : spans) {
			const JobRegions &c = L->rungs[(size_t) s.rung]->jr;
			memcpy(L->jr_reg.data() + s.dst, c.h_reg.as<NmRegion>() + s.src, (size_t) s.len * sizeof(NmRegion));
			if (root->jr.checks_on) {
				if (!c.checks_on) { set_err("internal: rung %d of a checks job ran without the checks", s.rung + 1); return CVX_ERR_HIP; }
				memcpy(L->jr_chk.data() + s.dst, c.h_chk.as<InvCheck>() + s.src, (size_t) s.len * sizeof(InvCheck));
			}
		}
		L->jr_open.resize((size_t) n);
		ladder_merge_records(n, rung_of.data(), at.data(), rec.data(), sizeof(NmOpen), L->jr_open.data());
	}
	if (root->jt.on) {
		for (int32_t r = 0; r < n_rungs; ++r) {
			const JobText &c = L->rungs[(size_t) r]->jt;
			if (!c.on) { set_err("internal: rung %d of a text job ran without the text stage", r + 1); return CVX_ERR_HIP; }
			off[(size_t) r] = c.h_off.as<uint64_t>();
			rec[(size_t) r] = c.h_rec.p;
			L->jt_rewrites += c.rewrites;
		}
		L->jt_off.assign((size_t) n + 1, 0);
		if (!ladder_merge_plan(n, rung_of.data(), at.data(), n_rungs, off.data(), rn.data(), L->jt_off.data(), spans)) {
			set_err("internal: the text offsets of a ladder job's rungs do not merge");
			return CVX_ERR_HIP;
		}
		L->jt_text.assign((size_t) L->jt_off[(size_t) n] + 1, '\0');
		for (const LadderSpan &s : spans) memcpy(L->jt_text.data() + s.dst, L->rungs[(size_t) s.rung]->jt.h_text.as<char>() + s.src, (size_t) s.len);
		L->jt_rec.resize((size_t) n);
		ladder_merge_records(n, rung_of.data(), at.data(), rec.data(), sizeof(TextRec), L->jt_rec.data());
	}
	return CVX_OK;
}

}  // namespace

/* the job's answer, once its ladder is done: every rung's records and ops waited for, then merged on the host -- per tile the
 * record of the last rung it took part in, its ops copied into one arena in tile order (ops_begin rebased), the ladder record
 * beside it; timing summed, launches strung together */
int ladder_finish(cvx_context *h, cvx_batch_s *root) {
	LadderState *L = root->ladder;
	if (L->merged) return CVX_OK;
	for (cvx_batch_s *c : L->rungs) {
		if (c->state < kFinished) RC_TRY(stage_results(h, c));
		RC_TRY(stage_ops(h, c));
	}
	const int n = root->n;
	const size_t n1 = (size_t) std::max(n, 1);
	std::vector<int32_t> rung_of((size_t) n, 0), at((size_t) n);
	for (int i = 0; i < n; ++i) at[(size_t) i] = i;
	for (size_t r = 1; r < L->rungs.size(); ++r) {
		const cvx_batch_s *c = L->rungs[r];
		const int32_t *head = c->h_lhead.as<int32_t>();
		for (int j = 0; j < c->n; ++j) {
			const int32_t i = head[1 + j];
			if (i < 0 || i >= n) { set_err("internal: rung %zu lists tile %d of %d", r + 1, i, n); return CVX_ERR_HIP; }
			rung_of[(size_t) i] = (int32_t) r;
			at[(size_t) i] = j;
		}
	}
	uint64_t total = 0;
	for (int i = 0; i < n; ++i) total += (uint64_t) L->rungs[(size_t) rung_of[(size_t) i]]->res()[at[(size_t) i]].n_ops;
	RC_TRY(root->h_lres.ensure(n1 * sizeof(ResultRec)));
	RC_TRY(root->h_lout.ensure(n1 * sizeof(cvx_ladder_result)));
	RC_TRY(root->h_lops.ensure((size_t) std::max<uint64_t>(total, 1) * sizeof(uint32_t)));
	ResultRec *res = root->h_lres.as<ResultRec>();
	cvx_ladder_result *out = root->h_lout.as<cvx_ladder_result>();
	uint32_t *ops = root->h_lops.as<uint32_t>();
	const cvx_ladder *lad = root->h_lad.as<cvx_ladder>();
	uint64_t used = 0;
	for (int i = 0; i < n; ++i) {
		const cvx_batch_s *c = L->rungs[(size_t) rung_of[(size_t) i]];
		ResultRec r = c->res()[at[(size_t) i]];
		if (r.n_ops > 0) memcpy(ops + used, c->h_ops.as<uint32_t>() + r.ops_begin, (size_t) r.n_ops * sizeof(uint32_t));
		r.ops_begin = used;
		used += (uint64_t) std::max(r.n_ops, 0);
		res[i] = r;
		const TileIn &ti = root->tin()[(size_t) i];
		RowSrc f;
		ladder_form(lad[i].corridor, lad[i].left, lad[i].right, lad[i].flags, ti.W, ti.H, rung_of[(size_t) i] + 1, f);
		out[i].rung = out[i].attempts = rung_of[(size_t) i] + 1;
		out[i].width = f.width;
		out[i].reserved = 0;
	}
	L->ops_total = used;
	RC_TRY(ladder_merge_stages(root, rung_of, at));
	memset(&L->timing, 0, sizeof(L->timing));
	L->launches.clear();
	for (const cvx_batch_s *c : L->rungs) {
		const cvx_timing &t = c->timing;
		L->timing.plan_ms += t.plan_ms; L->timing.fill_ms += t.fill_ms; L->timing.backtrack_ms += t.backtrack_ms; L->timing.total_ms += t.total_ms;
		L->timing.cells += t.cells; L->timing.active_cells += t.active_cells; L->timing.dir_bytes += t.dir_bytes;
		L->timing.n_fill_launches += t.n_fill_launches; L->timing.n_tiles_fast += t.n_tiles_fast; L->timing.n_tiles_redone += t.n_tiles_redone;
		L->timing.n_tiles_chained += t.n_tiles_chained;
		L->timing.chain_task_ticks += t.chain_task_ticks; L->timing.chain_poll_ticks += t.chain_poll_ticks;
		L->launches.insert(L->launches.end(), c->launches.begin(), c->launches.end());
	}
	L->merged = true;
	return CVX_OK;
}

/* what cvx_submit_ladder and cvx_submit_ladder_ex share behind their own refusals: the ladders checked, rung 1's form written
 * into a copy of the tiles, the job submitted (segs: its queries are segments of a read block, cvx_submit_segments' rules) */
static int submit_ladder_common(const char *who, cvx_handle h, cvx_genome g, int32_t n, const cvx_tile *tiles, const uint64_t *ref_position,
		const cvx_ladder *ladders, const SegmentsIn *segs, cvx_job *out) {
	/* rung 1's corridor from the ladder, like every later rung's; every rung a tile can reach checked here, on the host,
	 * so that the kernel writes none the device would refuse */
	std::vector<cvx_tile> forms(tiles, tiles + n);
	int max_rungs = 0;
	for (int32_t i = 0; i < n; ++i) {
		cvx_tile &t = forms[(size_t) i];
		const cvx_ladder &l = ladders[i];
		if (!ladder_args_ok(l, t.ref_len, t.qry_len)) {
			set_err("%s: tile %d: corridor %d, left %g, right %g, flags %d, ref_len %d, qry_len %d", who, i, l.corridor, (double) l.left, (double) l.right, l.flags, t.ref_len, t.qry_len);
			return CVX_ERR_ARG;
		}
		const int len = ladder_length(l.corridor, l.flags, t.ref_len);
		max_rungs = std::max(max_rungs, len);
		for (int m = len; m >= 1; --m) {      /* (downwards: rung 1's form is the one left in the tile) */
			RowSrc f;
			ladder_form(l.corridor, l.left, l.right, l.flags, t.ref_len, t.qry_len, m, f);
			if (f.width < 0 || (f.fmt == kRowsAffine && !affine_form_ok(f.k, f.d, f.right, t.qry_len))) {
				set_err("%s: tile %d: the corridor of rung %d is out of range", who, i, m);
				return CVX_ERR_ARG;
			}
			t.corridor_kind = f.fmt == kRowsConst ? CVX_CORRIDOR_CONST : CVX_CORRIDOR_AFFINE;
			t.corridor_k = f.k; t.corridor_d = f.d; t.corridor_right = f.right;
			t.corridor_offset = f.off0; t.corridor_width = f.width;
		}
		t.row_offset = nullptr; t.row_length = nullptr; t.row_stride_bytes = 4;
	}
	static const cvx_ladder none = { 0, 0.0f, 0.0f, 0 };      /* (an empty job is a ladder job too) */
	return submit_common(h, n, forms.data(), g, ref_position, out, segs, ladders ? ladders : &none, max_rungs);
}

extern "C" {

int cvx_submit_ladder(cvx_handle h, cvx_genome g, int32_t n, const cvx_tile *tiles, const uint64_t *ref_position, const cvx_ladder *ladders, cvx_job *out) {
	ABI_GUARD_BEGIN
	if (!h || !out || n < 0 || (n > 0 && (!tiles || !ladders)) || (!g && ref_position)) { set_err("cvx_submit_ladder: bad argument"); return CVX_ERR_ARG; }
	if (h->nm_regions || h->job_text || h->inv_checks || h->service) {
		set_err("cvx_submit_ladder: not on a handle with CVX_CREATE_NM_REGIONS, _JOB_TEXT, _INV_CHECKS or _SERVICE (the first three: cvx_submit_ladder_ex)");
		return CVX_ERR_ARG;
	}
	return submit_ladder_common("cvx_submit_ladder", h, g, n, tiles, ref_position, ladders, nullptr, out);
	ABI_GUARD_END
}

int cvx_submit_ladder_ex(cvx_handle h, cvx_genome g, int32_t n, const cvx_tile *tiles, const uint64_t *ref_position, const cvx_ladder *ladders,
		int32_t n_reads, const uint8_t *arena, const uint64_t *offsets, const cvx_read_segment *qry, cvx_job *out) {
	ABI_GUARD_BEGIN
	static const char who[] = "cvx_submit_ladder_ex";
	if (out) *out = nullptr;
	if (!h || !out || n < 0 || (n > 0 && (!tiles || !ladders)) || (!g && ref_position)) { set_err("%s: bad argument", who); return CVX_ERR_ARG; }
	if (h->service) { set_err("%s: not on a CVX_CREATE_SERVICE handle", who); return CVX_ERR_ARG; }
	if (!qry) {
		/* the string form: nothing of a read block may come with it */
		if (n_reads != 0 || arena || offsets) { set_err("%s: a read block (n_reads %d, arena, offsets) without segments", who, n_reads); return CVX_ERR_ARG; }
		return submit_ladder_common(who, h, g, n, tiles, ref_position, ladders, nullptr, out);
	}
	if (n_reads < 0 || !offsets || (n_reads > 0 && !arena)) { set_err("%s: segments without their read block (n_reads %d)", who, n_reads); return CVX_ERR_ARG; }
	const SegmentsIn segs = { n_reads, arena, offsets, qry };
	return submit_ladder_common(who, h, g, n, tiles, ref_position, ladders, &segs, out);
	ABI_GUARD_END
}

int cvx_job_ladder(cvx_handle h, cvx_job j, const cvx_ladder_result **out) {
	ABI_GUARD_BEGIN
	if (!h || !j || !out || !j->ladder || !j->ladder->merged) { set_err("cvx_job_ladder: not a finished ladder job (cvx_submit_ladder, then cvx_wait)"); return CVX_ERR_ARG; }
	*out = j->h_lout.as<cvx_ladder_result>();
	return CVX_OK;
	ABI_GUARD_END
}

int cvx_job_ladder_info(cvx_job j, cvx_ladder_info *out) {
	ABI_GUARD_BEGIN
	if (!j || !out || !j->ladder || !j->ladder->merged) { set_err("cvx_job_ladder_info: not a finished ladder job (cvx_submit_ladder, then cvx_wait)"); return CVX_ERR_ARG; }
	memset(out, 0, sizeof(*out));
	const LadderState *L = j->ladder;
	out->rungs_run = (int32_t) L->rungs.size();
	for (size_t r = 0; r < L->rungs.size() && r < 5; ++r) out->tiles[r] = L->rungs[r]->n;
	out->seq_bytes_after_submit = L->seq_bytes_after_submit;
	return CVX_OK;
	ABI_GUARD_END
}

}  /* extern "C" */
