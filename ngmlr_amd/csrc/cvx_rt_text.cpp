/*
 * cvx_rt_text.cpp -- the device-side text stage of finished alignment jobs over the kernels of cvx_text.hip, on
 * the handle's `text` stream: the CIGAR / MD strings and records (cvx_job_text, cvx_job_text_all), the per-position NM profile
 * of a job (cvx_job_nm_*) and of results the caller holds (cvx_nm_profile_ops), and that profile's low-identity regions found
 * on the device (cvx_job_nm_regions, cvx_nm_regions_ops).
 */
#include <cstring>
#include <vector>

#include "cvx_rt.h"

namespace {

/* what both text entries set up on `st`: the TextArgs over the job's arenas, the caller's soft-clip extensions (when given) on
 * the device, and room for the records, lengths and offsets of its tiles */
int text_setup(cvx_batch_s *j, const int32_t *ext_qstart, const int32_t *ext_qend, hipStream_t st, TextArgs &a) {
	const int n = j->n;
	const size_t n1 = (size_t) n;
	a = job_text_args(j);
	if (ext_qstart || ext_qend) {
		RC_TRY(j->h_ext.ensure(2 * n1 * sizeof(int32_t)));
		RC_TRY(j->d_ext.ensure(2 * n1));
		int32_t *he = j->h_ext.as<int32_t>();
		for (int i = 0; i < n; ++i) { he[i] = ext_qstart ? ext_qstart[i] : 0; he[n1 + (size_t) i] = ext_qend ? ext_qend[i] : 0; }
		HIP_TRY(hipMemcpyAsync(j->d_ext.p, he, 2 * n1 * sizeof(int32_t), hipMemcpyHostToDevice, st));
		a.ext_qstart = j->d_ext.p;
		a.ext_qend = j->d_ext.p + n1;
	}
	RC_TRY(j->d_trec.ensure(n1));
	RC_TRY(j->d_tlen.ensure(2 * n1 + 8));
	RC_TRY(j->h_trec.ensure(n1 * sizeof(TextRec)));
	RC_TRY(j->h_toff.ensure((n1 + 1) * sizeof(unsigned long long)));
	a.recs = j->d_trec.p;
	a.text_len = j->d_tlen.p; a.text_off = j->d_tlen.p + n1; a.text_total = j->d_tlen.p + 2 * n1;
	return CVX_OK;
}

/* results and an ops arena the caller holds, as the kernels read a job's: TileOut[] / TileRun[] over the arena, every valid tile's
 * range and op codes checked */
int held_ops_tiles(const char *who, int32_t n, const cvx_result *results, const uint32_t *ops_arena, uint64_t ops_total,
		std::vector<TileOut> &tout, std::vector<TileRun> &trun) {
	const size_t n1 = (size_t) n;
	tout.resize(n1);
	trun.resize(n1);
	for (size_t i = 0; i < n1; ++i) {
		const cvx_result &r = results[i];
		memset(&tout[i], 0, sizeof(TileOut));
		memset(&trun[i], 0, sizeof(TileRun));
		tout[i].status = r.status;
		tout[i].qstart = r.qstart;
		if (r.status != CVX_TILE_OK) continue;
		if (r.n_ops < 0 || r.ops_begin + (uint64_t) r.n_ops > ops_total) { set_err("%s: ops of tile %zu outside the arena", who, i); return CVX_ERR_ARG; }
		tout[i].n_ops = r.n_ops;
		trun[i].ops_off = r.ops_begin;
		for (int k = 0; k < r.n_ops; ++k) {
			const int type = (int) (ops_arena[r.ops_begin + (uint64_t) k] & 15u);
			if (type != CVX_OP_EQ && type != CVX_OP_X && type != CVX_OP_D && type != CVX_OP_I) { set_err("%s: op code %d in tile %zu", who, type, i); return CVX_ERR_ARG; }
		}
	}
	return CVX_OK;
}

}  // namespace

/* a scalar-twin handle's jobs: Convex::ConvexAlign writes neither Align::cigarOpCount nor Align::svType and has no N-clip block
 * (cvx_format_alignment_ex, CVX_FORMAT_SCALAR_TWIN); text_kernel computes them for every tile, the records leave without them */
static void twin_text_fields(const cvx_context *h, cvx_alignment_text *out, const int n) {
	if (!h->scalar_twin) return;
	for (int i = 0; i < n; ++i) { out[i].cigar_op_count = CVX_NOT_WRITTEN; out[i].sv_type = CVX_NOT_WRITTEN; }
}

extern "C" {

int cvx_job_text(cvx_handle h, cvx_job j, const int32_t *ext_qstart, const int32_t *ext_qend,
		cvx_alignment_text *out, uint64_t *text_off, const char **text, uint64_t *text_bytes) {
	ABI_GUARD_BEGIN
	static_assert(sizeof(TextRec) == sizeof(cvx_alignment_text), "TextRec mirrors cvx_alignment_text");
	if (!h || !j || j->state < kFinished) { set_err("cvx_job_text: job not finished (call cvx_wait first)"); return CVX_ERR_ARG; }
	if (j->ladder) { set_err("cvx_job_text: the stages of a finished job do not take a ladder job (cvx_submit_ladder)"); return CVX_ERR_ARG; }
	const int n = j->n;
	if (n > 0 && (!out || !text_off || !text)) { set_err("cvx_job_text: NULL output"); return CVX_ERR_ARG; }
	if (text_bytes) *text_bytes = 0;
	if (n == 0) { if (text) *text = ""; return CVX_OK; }
	HIP_TRY(hipSetDevice(h->device));
	hipStream_t st = h->s_text;
	const size_t n1 = (size_t) n;
	TextArgs a;
	RC_TRY(text_setup(j, ext_qstart, ext_qend, st, a));
	/* pass 1: lengths, fields, offsets; the total comes back with the offsets */
	HIP_TRY(launch_text_size(a, st));
	unsigned long long *hoff = j->h_toff.as<unsigned long long>();
	HIP_TRY(hipMemcpyAsync(hoff, a.text_off, (n1 + 1) * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
	HIP_TRY(hipMemcpyAsync(j->h_trec.p, j->d_trec.p, n1 * sizeof(TextRec), hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	const unsigned long long total = hoff[n1];
	/* pass 2: the strings */
	RC_TRY(j->d_text.ensure((size_t) total + 64));
	RC_TRY(j->h_text.ensure((size_t) total + 64));
	a.text = j->d_text.p;
	HIP_TRY(launch_text_write(a, st));
	HIP_TRY(hipMemcpyAsync(j->h_text.p, j->d_text.p, (size_t) ((total + 255) / 256 * 256 <= j->d_text.cap ? (total + 255) / 256 * 256 : total), hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	memcpy(out, j->h_trec.p, n1 * sizeof(TextRec));
	twin_text_fields(h, out, n);
	for (int i = 0; i < n; ++i) text_off[i] = hoff[i];
	*text = j->h_text.as<char>();
	if (text_bytes) *text_bytes = total;
	j->text_done = true;
	return CVX_OK;
	ABI_GUARD_END
}

/* ABI 9: cvx_job_text + cvx_job_nm_profile_resident of the whole job in two round trips to the device instead of four (sizes
 * of both, then strings and triples of both): what a dispatcher runs per finished launch */
int cvx_job_text_all(cvx_handle h, cvx_job j, const int32_t *ext_qstart, const int32_t *ext_qend,
		cvx_alignment_text *out, uint64_t *text_off, const char **text, uint64_t *text_bytes,
		uint64_t *nm_entry_off, const int32_t **triples) {
	ABI_GUARD_BEGIN
	if (!h || !j || j->state < kFinished) { set_err("cvx_job_text_all: job not finished (call cvx_wait first)"); return CVX_ERR_ARG; }
	if (j->ladder) { set_err("cvx_job_text_all: the stages of a finished job do not take a ladder job (cvx_submit_ladder)"); return CVX_ERR_ARG; }
	const int n = j->n;
	if (!text || !triples || (n > 0 && (!out || !text_off || !nm_entry_off))) { set_err("cvx_job_text_all: NULL output"); return CVX_ERR_ARG; }
	if (text_bytes) *text_bytes = 0;
	*triples = nullptr;
	if (n == 0) { *text = ""; return CVX_OK; }
	HIP_TRY(hipSetDevice(h->device));
	hipStream_t st = h->s_text;
	const size_t n1 = (size_t) n;
	TextArgs a;
	RC_TRY(text_setup(j, ext_qstart, ext_qend, st, a));
	RC_TRY(j->d_nmoff.ensure(2 * n1 + 8));
	RC_TRY(j->h_nmoff.ensure((n1 + 1) * sizeof(unsigned long long)));
	/* round trip 1: lengths, fields and offsets of the strings; entry counts and offsets of the profile */
	HIP_TRY(launch_text_size(a, st));
	unsigned long long *d_len = j->d_nmoff.p, *d_off = j->d_nmoff.p + n1;
	HIP_TRY(launch_nm_offsets(a, 0, n, d_len, d_off, d_off + n1, st));
	unsigned long long *hoff = j->h_toff.as<unsigned long long>(), *hnm = j->h_nmoff.as<unsigned long long>();
	HIP_TRY(hipMemcpyAsync(hoff, a.text_off, (n1 + 1) * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
	HIP_TRY(hipMemcpyAsync(hnm, d_off, (n1 + 1) * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
	HIP_TRY(hipMemcpyAsync(j->h_trec.p, j->d_trec.p, n1 * sizeof(TextRec), hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	const unsigned long long total = hoff[n1], entries = hnm[n1];
	/* round trip 2: the strings and the triples */
	RC_TRY(j->d_text.ensure((size_t) total + 64));
	RC_TRY(j->h_text.ensure((size_t) total + 64));
	RC_TRY(j->d_nm.ensure(3 * (size_t) entries + 16));
	RC_TRY(j->h_nm.ensure((3 * (size_t) entries + 16) * sizeof(int32_t)));
	a.text = j->d_text.p;
	HIP_TRY(launch_text_write(a, st));
	HIP_TRY(hipMemcpyAsync(j->h_text.p, j->d_text.p, (size_t) ((total + 255) / 256 * 256 <= j->d_text.cap ? (total + 255) / 256 * 256 : total), hipMemcpyDeviceToHost, st));
	HIP_TRY(launch_nm_profile(a, 0, n, d_off, j->d_nm.p, st));
	if (entries > 0) HIP_TRY(hipMemcpyAsync(j->h_nm.p, j->d_nm.p, 3 * (size_t) entries * sizeof(int32_t), hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	memcpy(out, j->h_trec.p, n1 * sizeof(TextRec));
	twin_text_fields(h, out, n);
	for (int i = 0; i < n; ++i) text_off[i] = hoff[i];
	for (int i = 0; i <= n; ++i) nm_entry_off[i] = hnm[i];
	*text = j->h_text.as<char>();
	*triples = j->h_nm.as<int32_t>();
	if (text_bytes) *text_bytes = total;
	j->text_done = true;
	return CVX_OK;
	ABI_GUARD_END
}

static int nm_profile_common(cvx_handle h, cvx_job j, int32_t first, int32_t count, uint64_t *entry_off,
		int32_t *triples, uint64_t cap_entries, double *kernel_ms, bool sizes_only, const int32_t **resident = nullptr) {
	if (kernel_ms) *kernel_ms = 0.0;
	if (!h || !j || j->state < kFinished) { set_err("cvx_job_nm_profile: job not finished (call cvx_wait first)"); return CVX_ERR_ARG; }
	if (j->ladder) { set_err("cvx_job_nm_profile: the stages of a finished job do not take a ladder job (cvx_submit_ladder)"); return CVX_ERR_ARG; }
	if (!j->text_done) { set_err("cvx_job_nm_profile: call cvx_job_text first (it counts the entries)"); return CVX_ERR_ARG; }
	if (first < 0 || count < 0 || (int64_t) first + count > j->n || (count > 0 && !entry_off)) { set_err("cvx_job_nm_profile: bad tile range / NULL offsets"); return CVX_ERR_ARG; }
	if (count == 0) return CVX_OK;
	HIP_TRY(hipSetDevice(h->device));
	hipStream_t st = h->s_text;
	const size_t c1 = (size_t) count;
	RC_TRY(j->d_nmoff.ensure(2 * c1 + 8));
	RC_TRY(j->h_nmoff.ensure((c1 + 1) * sizeof(unsigned long long)));
	HIP_TRY(j->ev_nm0.make());
	HIP_TRY(j->ev_nm1.make());
	TextArgs a = job_text_args(j);
	a.recs = j->d_trec.p;
	unsigned long long *d_len = j->d_nmoff.p, *d_off = j->d_nmoff.p + c1;      /* the total lands right behind the offsets */
	HIP_TRY(launch_nm_offsets(a, first, count, d_len, d_off, d_off + c1, st));
	unsigned long long *hoff = j->h_nmoff.as<unsigned long long>();
	HIP_TRY(hipMemcpyAsync(hoff, d_off, (c1 + 1) * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	for (size_t i = 0; i <= c1; ++i) entry_off[i] = hoff[i];
	const unsigned long long total = hoff[c1];
	if (sizes_only) return CVX_OK;      /* the entry offsets alone: no 12-byte-per-column arena, no profile kernel */
	if (triples && total > cap_entries) { set_err("cvx_job_nm_profile: %llu entries, room for %llu", total, (unsigned long long) cap_entries); return CVX_ERR_CAPACITY; }
	RC_TRY(j->d_nm.ensure(3 * (size_t) total + 16));
	if (resident) {
		RC_TRY(j->h_nm.ensure((3 * (size_t) total + 16) * sizeof(int32_t)));
		triples = j->h_nm.as<int32_t>();
		*resident = triples;
	}
	HIP_TRY(hipEventRecord(j->ev_nm0, st));
	HIP_TRY(launch_nm_profile(a, first, count, d_off, j->d_nm.p, st));
	HIP_TRY(hipEventRecord(j->ev_nm1, st));
	if (triples && total > 0) HIP_TRY(hipMemcpyAsync(triples, j->d_nm.p, 3 * (size_t) total * sizeof(int32_t), hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	if (kernel_ms) { float ms = 0.0f; HIP_TRY(hipEventElapsedTime(&ms, j->ev_nm0, j->ev_nm1)); *kernel_ms = ms; }
	return CVX_OK;
}

int cvx_job_nm_profile(cvx_handle h, cvx_job j, int32_t first, int32_t count, uint64_t *entry_off,
		int32_t *triples, uint64_t cap_entries, double *kernel_ms) {
	ABI_GUARD_BEGIN return nm_profile_common(h, j, first, count, entry_off, triples, cap_entries, kernel_ms, false); ABI_GUARD_END
}

int cvx_job_nm_profile_resident(cvx_handle h, cvx_job j, int32_t first, int32_t count, uint64_t *entry_off,
		const int32_t **triples, double *kernel_ms) {
	ABI_GUARD_BEGIN
	if (!triples) { set_err("cvx_job_nm_profile_resident: NULL argument"); return CVX_ERR_ARG; }
	*triples = nullptr;
	return nm_profile_common(h, j, first, count, entry_off, nullptr, 0, kernel_ms, false, triples);
	ABI_GUARD_END
}

int cvx_job_nm_sizes(cvx_handle h, cvx_job j, int32_t first, int32_t count, uint64_t *entry_off) {
	ABI_GUARD_BEGIN return nm_profile_common(h, j, first, count, entry_off, nullptr, 0, nullptr, true); ABI_GUARD_END
}

int cvx_nm_profile_ops(cvx_handle h, int32_t n, const cvx_result *results, const uint32_t *ops_arena, uint64_t ops_total,
		uint64_t *entry_off, int32_t *triples, uint64_t cap_entries) {
	ABI_GUARD_BEGIN
	if (!h || n < 0 || (n > 0 && (!results || !entry_off)) || (ops_total > 0 && !ops_arena)) { set_err("cvx_nm_profile_ops: bad argument"); return CVX_ERR_ARG; }
	if (n == 0) return CVX_OK;
	HIP_TRY(hipSetDevice(h->device));
	RC_TRY(ensure_streams(h));
	const size_t n1 = (size_t) n;
	std::vector<TileOut> tout;
	std::vector<TileRun> trun;
	RC_TRY(held_ops_tiles("cvx_nm_profile_ops", n, results, ops_arena, ops_total, tout, trun));
	std::vector<unsigned long long> off(n1 + 1, 0ull);
	for (size_t i = 0; i < n1; ++i) {
		const cvx_result &r = results[i];
		unsigned long long cnt = 0;
		if (r.status == CVX_TILE_OK) {
			/* entries per op, as addPosition admits them (src/ConvexAlignFast.cpp:76-98) */
			long long pr = 0, pq = r.qstart;
			for (int k = 0; k < r.n_ops; ++k) {
				const uint32_t w = ops_arena[r.ops_begin + (uint64_t) k];
				const long long len = (long long) (w >> 4);
				const int type = (int) (w & 15u);
				if (type == CVX_OP_EQ || type == CVX_OP_X) {
					const long long mn = pr < pq ? pr : pq, skip = 17 - mn > 0 ? 17 - mn : 0;
					cnt += (unsigned long long) (len - skip > 0 ? len - skip : 0);
					pr += len; pq += len;
				} else if (type == CVX_OP_D) {
					if (pq > 16) { const long long skip = 17 - pr > 0 ? 17 - pr : 0; cnt += (unsigned long long) (len - skip > 0 ? len - skip : 0); }
					pr += len;
				} else pq += len;      /* (CVX_OP_I: held_ops_tiles let nothing else through) */
			}
		}
		off[i + 1] = off[i] + cnt;
	}
	for (size_t i = 0; i <= n1; ++i) entry_off[i] = off[i];
	const unsigned long long total = off[n1];
	if (!triples) return CVX_OK;                      /* sizes only */
	if (total > cap_entries) { set_err("cvx_nm_profile_ops: %llu entries, room for %llu", total, (unsigned long long) cap_entries); return CVX_ERR_CAPACITY; }
	DevBuf<int32_t> d_ops, d_tri;
	DevBuf<TileOut> d_tout;
	DevBuf<TileRun> d_trun;
	DevBuf<unsigned long long> d_off;
	RC_TRY(d_ops.ensure((size_t) ops_total + 16));
	RC_TRY(d_tri.ensure(3 * (size_t) total + 16));
	RC_TRY(d_tout.ensure(n1));
	RC_TRY(d_trun.ensure(n1));
	RC_TRY(d_off.ensure(n1 + 1));
	hipStream_t st = h->s_text;
	if (ops_total) HIP_TRY(hipMemcpyAsync(d_ops.p, ops_arena, (size_t) ops_total * sizeof(uint32_t), hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemcpyAsync(d_tout.p, tout.data(), n1 * sizeof(TileOut), hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemcpyAsync(d_trun.p, trun.data(), n1 * sizeof(TileRun), hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemcpyAsync(d_off.p, off.data(), (n1 + 1) * sizeof(unsigned long long), hipMemcpyHostToDevice, st));
	TextArgs a;
	memset(&a, 0, sizeof(a));
	a.tout = d_tout.p; a.trun = d_trun.p; a.ops = d_ops.p; a.n_tiles = n;
	HIP_TRY(launch_nm_profile(a, 0, n, d_off.p, d_tri.p, st));
	if (total) HIP_TRY(hipMemcpyAsync(triples, d_tri.p, 3 * (size_t) total * sizeof(int32_t), hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	return CVX_OK;
	ABI_GUARD_END
}

/* ---- the profile's low-identity regions (nm_regions_kernel): the peak finder of detectMisalignment, src/AlignmentBuffer.cpp:1316-1395 */

int cvx_job_nm_regions(cvx_handle h, cvx_job j, int32_t first, int32_t count, uint64_t *region_off,
		const cvx_nm_region **regions, cvx_nm_open *open, double *kernel_ms) {
	ABI_GUARD_BEGIN
	static_assert(sizeof(NmRegion) == sizeof(cvx_nm_region) && sizeof(NmOpen) == sizeof(cvx_nm_open), "NmRegion / NmOpen mirror cvx_nm_region / cvx_nm_open");
	if (kernel_ms) *kernel_ms = 0.0;
	if (regions) *regions = nullptr;
	if (!h || !j || j->state < kFinished) { set_err("cvx_job_nm_regions: job not finished (call cvx_wait first)"); return CVX_ERR_ARG; }
	if (j->ladder) { set_err("cvx_job_nm_regions: the stages of a finished job do not take a ladder job (cvx_submit_ladder)"); return CVX_ERR_ARG; }
	if (!j->text_done) { set_err("cvx_job_nm_regions: call cvx_job_text first"); return CVX_ERR_ARG; }
	if (first < 0 || count < 0 || (int64_t) first + count > j->n || (count > 0 && (!region_off || !regions))) { set_err("cvx_job_nm_regions: bad tile range / NULL output"); return CVX_ERR_ARG; }
	if (count == 0) return CVX_OK;
	HIP_TRY(hipSetDevice(h->device));
	hipStream_t st = h->s_text;
	const size_t c1 = (size_t) count;
	RC_TRY(j->d_nmroff.ensure(2 * c1 + 8));
	RC_TRY(j->d_nmopen.ensure(c1));
	RC_TRY(j->d_nmstage.ensure(c1 * (size_t) kNmStage));
	RC_TRY(j->h_nmroff.ensure((c1 + 1) * sizeof(unsigned long long)));
	if (open) RC_TRY(j->h_nmopen.ensure(c1 * sizeof(NmOpen)));
	HIP_TRY(j->ev_nm0.make());
	HIP_TRY(j->ev_nm1.make());
	const TextArgs a = job_text_args(j);
	/* pass 1: the regions per tile, their offsets (the total right behind them), the end states */
	unsigned long long *d_len = j->d_nmroff.p, *d_off = j->d_nmroff.p + c1;
	HIP_TRY(hipEventRecord(j->ev_nm0, st));
	HIP_TRY(launch_nm_regions_count(a, first, count, d_len, d_off, d_off + c1, j->d_nmopen.p, j->d_nmstage.p, st));
	HIP_TRY(hipEventRecord(j->ev_nm1, st));
	unsigned long long *hoff = j->h_nmroff.as<unsigned long long>();
	HIP_TRY(hipMemcpyAsync(hoff, d_off, (c1 + 1) * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
	if (open) HIP_TRY(hipMemcpyAsync(j->h_nmopen.p, j->d_nmopen.p, c1 * sizeof(NmOpen), hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	float ms1 = 0.0f, ms2 = 0.0f;
	HIP_TRY(hipEventElapsedTime(&ms1, j->ev_nm0, j->ev_nm1));
	const unsigned long long total = hoff[c1];
	/* pass 2: the regions, dense and in tile order */
	RC_TRY(j->d_nmreg.ensure((size_t) total + 4));
	RC_TRY(j->h_nmreg.ensure(((size_t) total + 4) * sizeof(NmRegion)));
	if (total > 0) {
		HIP_TRY(hipEventRecord(j->ev_nm0, st));
		HIP_TRY(launch_nm_regions_write(a, first, count, d_len, d_off, j->d_nmstage.p, j->d_nmreg.p, st));
		HIP_TRY(hipEventRecord(j->ev_nm1, st));
		HIP_TRY(hipMemcpyAsync(j->h_nmreg.p, j->d_nmreg.p, (size_t) total * sizeof(NmRegion), hipMemcpyDeviceToHost, st));
		HIP_TRY(hipStreamSynchronize(st));
		HIP_TRY(hipEventElapsedTime(&ms2, j->ev_nm0, j->ev_nm1));
	}
	for (size_t i = 0; i <= c1; ++i) region_off[i] = hoff[i];
	if (open) memcpy(open, j->h_nmopen.p, c1 * sizeof(NmOpen));
	*regions = j->h_nmreg.as<cvx_nm_region>();
	if (kernel_ms) *kernel_ms = (double) ms1 + (double) ms2;
	return CVX_OK;
	ABI_GUARD_END
}

int cvx_nm_regions_ops(cvx_handle h, int32_t n, const cvx_result *results, const uint32_t *ops_arena, uint64_t ops_total,
		uint64_t *region_off, cvx_nm_region *regions, uint64_t cap_regions, cvx_nm_open *open) {
	ABI_GUARD_BEGIN
	if (!h || n < 0 || (n > 0 && (!results || !region_off)) || (ops_total > 0 && !ops_arena)) { set_err("cvx_nm_regions_ops: bad argument"); return CVX_ERR_ARG; }
	if (n == 0) return CVX_OK;
	HIP_TRY(hipSetDevice(h->device));
	RC_TRY(ensure_streams(h));
	const size_t n1 = (size_t) n;
	std::vector<TileOut> tout;
	std::vector<TileRun> trun;
	RC_TRY(held_ops_tiles("cvx_nm_regions_ops", n, results, ops_arena, ops_total, tout, trun));
	std::vector<unsigned long long> off(n1 + 1, 0ull);      /* (in front of the device buffers: they wait for the device as they go, and then nothing copies into it any more) */
	DevBuf<int32_t> d_ops;
	DevBuf<TileOut> d_tout;
	DevBuf<TileRun> d_trun;
	DevBuf<unsigned long long> d_off;
	DevBuf<NmOpen> d_open;
	DevBuf<NmRegion> d_stage, d_reg;
	RC_TRY(d_ops.ensure((size_t) ops_total + 16));
	RC_TRY(d_tout.ensure(n1));
	RC_TRY(d_trun.ensure(n1));
	RC_TRY(d_off.ensure(2 * n1 + 8));
	RC_TRY(d_open.ensure(n1));
	RC_TRY(d_stage.ensure(n1 * (size_t) kNmStage));
	hipStream_t st = h->s_text;
	if (ops_total) HIP_TRY(hipMemcpyAsync(d_ops.p, ops_arena, (size_t) ops_total * sizeof(uint32_t), hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemcpyAsync(d_tout.p, tout.data(), n1 * sizeof(TileOut), hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemcpyAsync(d_trun.p, trun.data(), n1 * sizeof(TileRun), hipMemcpyHostToDevice, st));
	TextArgs a;
	memset(&a, 0, sizeof(a));
	a.tout = d_tout.p; a.trun = d_trun.p; a.ops = d_ops.p; a.n_tiles = n;
	unsigned long long *d_len = d_off.p, *d_o = d_off.p + n1;
	HIP_TRY(launch_nm_regions_count(a, 0, n, d_len, d_o, d_o + n1, d_open.p, d_stage.p, st));
	HIP_TRY(hipMemcpyAsync(off.data(), d_o, (n1 + 1) * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
	if (open) HIP_TRY(hipMemcpyAsync(open, d_open.p, n1 * sizeof(NmOpen), hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	for (size_t i = 0; i <= n1; ++i) region_off[i] = off[i];
	const unsigned long long total = off[n1];
	if (!regions) return CVX_OK;                      /* sizes only */
	if (total > cap_regions) { set_err("cvx_nm_regions_ops: %llu regions, room for %llu", total, (unsigned long long) cap_regions); return CVX_ERR_CAPACITY; }
	if (total == 0) return CVX_OK;
	RC_TRY(d_reg.ensure((size_t) total + 4));
	HIP_TRY(launch_nm_regions_write(a, 0, n, d_len, d_o, d_stage.p, d_reg.p, st));
	HIP_TRY(hipMemcpyAsync(regions, d_reg.p, (size_t) total * sizeof(NmRegion), hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	return CVX_OK;
	ABI_GUARD_END
}

}  /* extern "C" */
