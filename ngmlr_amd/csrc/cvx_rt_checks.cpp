/*
 * cvx_rt_checks.cpp -- the inversion checks of low-identity regions (checkForSV's two scores, cvx_inv_checks.h) over regions the
 * caller holds: the kernel (cvx_inv_checks) and the rule on the host (cvx_inv_checks_host).  What a job of a CVX_CREATE_INV_CHECKS
 * handle brings back with its regions (cvx_job_checks) is queued and served by JobRegions, cvx_rt_stages.cpp.
 */
#include <cstring>
#include <vector>

#include "cvx_rt.h"

namespace {

/* what the two stand-alone entries ask of their arguments; *total = the regions of the call */
int checks_args(const char *who, int32_t n_tiles, const char *const *qrys, const int32_t *qry_len, const uint64_t *ref_position,
		const int32_t *position_offset, const uint64_t *region_off, const cvx_nm_region *regions, const cvx_inv_check *checks, uint64_t *total) {
	*total = 0;
	if (n_tiles < 0 || (n_tiles > 0 && (!qrys || !qry_len || !ref_position || !position_offset || !region_off))) { set_err("%s: bad argument", who); return CVX_ERR_ARG; }
	if (n_tiles == 0) return CVX_OK;
	if (region_off[0] != 0) { set_err("%s: region_off[0] is not 0", who); return CVX_ERR_ARG; }
	for (int32_t i = 0; i < n_tiles; ++i) {
		if (region_off[i + 1] < region_off[i]) { set_err("%s: the region offsets descend at tile %d", who, i); return CVX_ERR_ARG; }
		if (qry_len[i] < 0 || (qry_len[i] > 0 && !qrys[i])) { set_err("%s: tile %d: qry_len %d / NULL query", who, i, qry_len[i]); return CVX_ERR_ARG; }
	}
	*total = region_off[n_tiles];
	if (*total > 0 && (!regions || !checks)) { set_err("%s: NULL regions / checks", who); return CVX_ERR_ARG; }
	return CVX_OK;
}

/* the device side of cvx_inv_checks: the call's buffers and events belong to the entry, which waits for the device before they go */
struct InvChecksBufs {
	DevBuf<uint8_t> d_seq;
	DevBuf<TileIn> d_tin;
	DevBuf<WindowDesc> d_win;
	DevBuf<ResultRec> d_rec;
	DevBuf<unsigned long long> d_off;
	DevBuf<NmRegion> d_reg;
	DevBuf<InvCheck> d_chk;
	Event e0, e1;
};

int inv_checks_run(cvx_handle h, cvx_genome g, const std::vector<uint8_t> &seq, const std::vector<TileIn> &tin, const std::vector<WindowDesc> &win,
		const std::vector<ResultRec> &rec, const std::vector<unsigned long long> &off, const cvx_nm_region *regions, uint64_t total,
		cvx_inv_check *checks, double *kernel_ms, InvChecksBufs &b) {
	const size_t n1 = tin.size();
	RC_TRY(b.d_seq.ensure(seq.size()));
	RC_TRY(b.d_tin.ensure(n1));
	RC_TRY(b.d_win.ensure(n1));
	RC_TRY(b.d_rec.ensure(n1));
	RC_TRY(b.d_off.ensure(n1 + 1));
	RC_TRY(b.d_reg.ensure((size_t) total));
	RC_TRY(b.d_chk.ensure((size_t) total));
	HIP_TRY(b.e0.make());
	HIP_TRY(b.e1.make());
	hipStream_t st = h->s_main;
	HIP_TRY(hipMemcpyAsync(b.d_seq.p, seq.data(), seq.size(), hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemcpyAsync(b.d_tin.p, tin.data(), n1 * sizeof(TileIn), hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemcpyAsync(b.d_win.p, win.data(), n1 * sizeof(WindowDesc), hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemcpyAsync(b.d_rec.p, rec.data(), n1 * sizeof(ResultRec), hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemcpyAsync(b.d_off.p, off.data(), (n1 + 1) * sizeof(unsigned long long), hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemcpyAsync(b.d_reg.p, regions, (size_t) total * sizeof(NmRegion), hipMemcpyHostToDevice, st));
	InvCheckArgs a;
	memset(&a, 0, sizeof(a));
	a.bin = g->d_bin.p; a.L = score_windows_concat_len(g->n_nibbles);
	a.seq = b.d_seq.p; a.tin = b.d_tin.p; a.win = b.d_win.p; a.rec = b.d_rec.p;
	a.off = b.d_off.p; a.regions = b.d_reg.p; a.checks = b.d_chk.p;
	a.cap = total; a.n_tiles = (int32_t) n1;
	HIP_TRY(hipEventRecord(b.e0, st));
	HIP_TRY(launch_inv_checks(a, total, st));
	HIP_TRY(hipEventRecord(b.e1, st));
	HIP_TRY(hipMemcpyAsync(checks, b.d_chk.p, (size_t) total * sizeof(InvCheck), hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	if (kernel_ms) *kernel_ms = (double) ev_ms(b.e0, b.e1);
	return CVX_OK;
}

}  // namespace

extern "C" {

int cvx_inv_checks(cvx_handle h, cvx_genome g, int32_t n_tiles, const char *const *qrys, const int32_t *qry_len,
		const uint64_t *ref_position, const int32_t *position_offset,
		const uint64_t *region_off, const cvx_nm_region *regions, cvx_inv_check *checks, double *kernel_ms) {
	ABI_GUARD_BEGIN
	static_assert(sizeof(NmRegion) == sizeof(cvx_nm_region), "NmRegion mirrors cvx_nm_region");
	if (kernel_ms) *kernel_ms = 0.0;
	if (!h || !g) { set_err("cvx_inv_checks: NULL handle / genome"); return CVX_ERR_ARG; }
	if (g->device != h->device) { set_err("cvx_inv_checks: the genome lives on device %d, the handle on %d", g->device, h->device); return CVX_ERR_ARG; }
	uint64_t total = 0;
	RC_TRY(checks_args("cvx_inv_checks", n_tiles, qrys, qry_len, ref_position, position_offset, region_off, regions, checks, &total));
	if (total == 0) return CVX_OK;
	HIP_TRY(hipSetDevice(h->device));
	RC_TRY(ensure_streams(h));
	/* the queries back to back in an arena of the call's own, and the three per-tile records the job form reads, filled in with
	 * what the kernel looks at: nothing here is on the path of a job */
	const size_t n1 = (size_t) n_tiles;
	std::vector<TileIn> tin(n1);
	std::vector<WindowDesc> win(n1);
	std::vector<ResultRec> rec(n1);
	std::vector<unsigned long long> off(n1 + 1);
	uint64_t seq_bytes = 0;
	for (size_t i = 0; i < n1; ++i) {
		memset(&tin[i], 0, sizeof(TileIn));
		memset(&win[i], 0, sizeof(WindowDesc));
		memset(&rec[i], 0, sizeof(ResultRec));
		tin[i].qry_off = (uint32_t) seq_bytes;
		tin[i].H = qry_len[i];
		win[i].position = ref_position[i];
		rec[i].ref_position = position_offset[i];
		seq_bytes += (uint64_t) qry_len[i];
		if (seq_bytes > 0xffffffffull) { set_err("cvx_inv_checks: more than 4 GiB of queries in one call; split it"); return CVX_ERR_ARG; }
	}
	for (size_t i = 0; i <= n1; ++i) off[i] = region_off[i];
	std::vector<uint8_t> seq((size_t) seq_bytes + 4, 0);
	for (size_t i = 0; i < n1; ++i)
		if (qry_len[i] > 0) memcpy(seq.data() + tin[i].qry_off, qrys[i], (size_t) qry_len[i]);
	InvChecksBufs b;
	const int rc = inv_checks_run(h, g, seq, tin, win, rec, off, regions, total, checks, kernel_ms, b);
	if (rc != CVX_OK) (void) hipDeviceSynchronize();      /* nothing may still read the call's buffers when they go */
	return rc;
	ABI_GUARD_END
}

int cvx_inv_checks_host(const uint8_t *bin_ref, uint64_t n_nibbles, const uint64_t *start_table, int32_t n_starts,
		int32_t n_tiles, const char *const *qrys, const int32_t *qry_len,
		const uint64_t *ref_position, const int32_t *position_offset,
		const uint64_t *region_off, const cvx_nm_region *regions, cvx_inv_check *checks) {
	ABI_GUARD_BEGIN
	uint64_t L = 0;
	if (!bin_ref || cvx_genome_concat_len(n_nibbles, start_table, n_starts, &L) != CVX_OK) { set_err("cvx_inv_checks_host: bad argument"); return CVX_ERR_ARG; }
	uint64_t total = 0;
	RC_TRY(checks_args("cvx_inv_checks_host", n_tiles, qrys, qry_len, ref_position, position_offset, region_off, regions, checks, &total));
	for (int32_t i = 0; i < n_tiles; ++i)
		for (uint64_t r = region_off[i]; r < region_off[i + 1]; ++r) {
			const cvx_nm_region &g = regions[r];
			const InvCheck c = inv_check_host(bin_ref, L, (const uint8_t *) qrys[i], qry_len[i], ref_position[i], position_offset[i],
					g.ref_start, g.ref_stop, g.read_start, g.read_stop);
			checks[r].score_fwd = c.score_fwd; checks[r].score_rev = c.score_rev;
			checks[r].status = c.status; checks[r].window_chars = c.window_chars;
		}
	return CVX_OK;
	ABI_GUARD_END
}

}  /* extern "C" */
