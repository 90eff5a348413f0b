/*
 * cvx_rt_search.cpp -- the search side of libcvxalign.so: the reference genome resident in HBM and the decode of
 * its windows (cvx_genome.hip), ngmlr's k-mer table on the device, uploaded or built there (cvx_index.hip), and the candidate
 * search of a batch of reads over it (cvx_search.hip).
 */
#include <algorithm>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "cvx_index_build.h"
#include "cvx_rt.h"
#include "cvx_score_cands.h"
#include "cvx_score_stage.h"
#include "cvx_search_plan.h"

/* Per-handle state of the candidate search: staging and device buffers live as long as the handle, so that the steady
 * state of a caller that searches batch after batch (ngmlr's CS threads: a few hundred sub-reads per call) allocates
 * nothing, copies through page-locked memory and sleeps on a blocking event while the device works. */
struct cvx_search_state {
	PinBuf h_seq, h_meta, h_out;       /* reads; offsets + lengths + list offsets + work list + dense begins; results coming back */
	DevBuf<uint8_t> d_seq;
	DevBuf<uint64_t> d_off, d_listoff, d_begin, d_srcoff;
	PinBuf h_srcoff;
	DevBuf<int32_t> d_len, d_ncand, d_work, d_miss;
	DevBuf<unsigned long long> d_events;
	DevBuf<float> d_maxhit, d_scores;
	DevBuf<uint32_t> d_rlist, d_undo;
	DevBuf<unsigned int> d_ticket;
	size_t tables_clean_words = 0;     /* this much of d_keys is known to hold nothing but empty slots (search_wave_hbm_kernel's tables) */
	DevBuf<SearchCandidate> d_cand, d_dense;
	DevBuf<uint64_t> d_keys;
	Event done;
	/* kernel time of the last call (cvx_stage_kernel_ms): an event pair around every kernel launch of the call, summed when it ends */
	std::vector<int32_t> attempts;     /* per read of the last call: table sizes tried (cvx_search_last_attempts) */
	std::vector<Event> kev;
	size_t kev_used = 0;
	float kernel_ms = 0.0f;
	/* cvx_search_score_arena: one descriptor, pair, score and status per candidate, the strings of all of them, and the scores and
	 * status words on their way back; the plan + stage + score kernels of the last such call between ev_f0 and ev_f1 */
	DevBuf<ScoreWinDesc> d_fdesc;
	DevBuf<ScorePair> d_fpairs;
	DevBuf<uint8_t> d_fseq;
	DevBuf<float> d_fout;
	DevBuf<int32_t> d_fstatus;
	PinBuf h_fout;
	Event ev_f0, ev_f1;
	float fused_ms = 0.0f;
	int kmark(hipStream_t st) {
		if (kev_used == kev.size()) { Event e; HIP_TRY(e.make()); kev.push_back(std::move(e)); }
		HIP_TRY(hipEventRecord(kev[kev_used++], st));
		return CVX_OK;
	}
};

/* what cvx_search_score_arena adds to a search: the scoring of every candidate behind the compaction (checked by the entry) */
struct SearchScoreArgs {
	const cvx_genome_s *g;
	int32_t buffer_len, window_lead, max_cmrs;
	uint64_t max_read_bytes;         /* the longest read of the call, its NUL included */
	float *sw_scores;
	int32_t *sw_status;              /* may be NULL */
};

namespace {
/* everything queued on `st` so far is done; the calling thread sleeps meanwhile (hipStreamSynchronize spins) */
int search_wait(cvx_search_state *ss, hipStream_t st) {
	HIP_TRY(ss->done.make(hipEventBlockingSync | hipEventDisableTiming));
	HIP_TRY(hipEventRecord(ss->done, st));
	HIP_TRY(hipEventSynchronize(ss->done));
	return CVX_OK;
}
}  // namespace

namespace cvx {
void search_state_free(cvx_search_state *ss) { delete ss; }

float search_kernel_ms(const cvx_search_state *ss) { return ss ? ss->kernel_ms : 0.0f; }
float search_score_kernel_ms(const cvx_search_state *ss) { return ss ? ss->fused_ms : 0.0f; }
}  // namespace cvx

extern "C" {

/* ------------------------------------------------------------------ resident genome (decode half) */

int cvx_genome_upload(cvx_handle h, const uint8_t *bin_ref, uint64_t n_nibbles, const uint64_t *start_table, int32_t n_starts, cvx_genome *out) {
	ABI_GUARD_BEGIN
	if (!h || !out || !bin_ref || !start_table || n_starts < 2 || n_nibbles < 2) { set_err("cvx_genome_upload: bad argument"); return CVX_ERR_ARG; }
	*out = nullptr;
	for (int32_t i = 1; i < n_starts; ++i)
		if (start_table[i] <= start_table[i - 1]) { set_err("cvx_genome_upload: start table not ascending at %d", i); return CVX_ERR_ARG; }
	HIP_TRY(hipSetDevice(h->device));
	std::unique_ptr<cvx_genome_s> g(new (std::nothrow) cvx_genome_s());
	if (!g) return CVX_ERR_OOM;
	g->device = h->device;
	g->n_nibbles = n_nibbles;
	g->n_starts = n_starts;
	/* a window may start or end in the last spacer: decode() reads up to a byte past the last nibble pair */
	const size_t bytes = (size_t) ((n_nibbles + 1) / 2);
	RC_TRY(g->d_bin.ensure(bytes + 64));
	RC_TRY(g->d_starts.ensure((size_t) n_starts));
	HIP_TRY_IN("cvx_genome_upload", hipMemset(g->d_bin.p, 0x44, g->d_bin.cap));        /* beyond the genome: N */
	HIP_TRY_IN("cvx_genome_upload", hipMemcpy(g->d_bin.p, bin_ref, bytes, hipMemcpyHostToDevice));
	HIP_TRY_IN("cvx_genome_upload", hipMemcpy(g->d_starts.p, start_table, (size_t) n_starts * sizeof(uint64_t), hipMemcpyHostToDevice));
	*out = g.release();      /* (the unique_ptr's: the caller owns the genome from here) */
	return CVX_OK;
	ABI_GUARD_END
}

void cvx_genome_free(cvx_handle h, cvx_genome g) {
	ABI_GUARD_BEGIN
	if (!g) return;
	if (h) { (void) hipSetDevice(h->device); (void) hipDeviceSynchronize(); }
	delete g;
	ABI_GUARD_END_VOID
}

int cvx_genome_decode(cvx_handle h, cvx_genome g, int32_t n, const uint64_t *position, const int32_t *length,
		const uint64_t *out_offset, char *out) {
	ABI_GUARD_BEGIN
	if (!h || !g || n < 0 || (n > 0 && (!position || !length || !out_offset || !out))) { set_err("cvx_genome_decode: bad argument"); return CVX_ERR_ARG; }
	if (n == 0) return CVX_OK;
	HIP_TRY(hipSetDevice(h->device));
	std::vector<WindowDesc> win((size_t) n);
	uint64_t total = 0;
	for (int i = 0; i < n; ++i) {
		if (length[i] < 1) { set_err("cvx_genome_decode: window %d has length %d", i, length[i]); return CVX_ERR_ARG; }
		win[(size_t) i].position = position[i];
		win[(size_t) i].dst_off = total;
		win[(size_t) i].n_chars = (int64_t) length[i] - 1;           /* the reference's last byte is the NUL */
		total += (uint64_t) length[i];
	}
	static const char who[] = "cvx_genome_decode";
	std::vector<uint8_t> host((size_t) total);      /* (in front of the device buffers: they wait for the device as they go, and then nothing copies into it any more) */
	DevBuf<uint8_t> d_out;
	DevBuf<WindowDesc> d_win;
	Event k0, k1;                    /* the kernel alone, on its own stream */
	RC_TRY(d_out.ensure((size_t) total + 64));
	RC_TRY(d_win.ensure((size_t) n));
	hipStream_t st = h->s_main;
	HIP_TRY_IN(who, hipMemsetAsync(d_out.p, 0, (size_t) total, st));   /* the NUL that ends every window */
	HIP_TRY_IN(who, hipMemcpyAsync(d_win.p, win.data(), (size_t) n * sizeof(WindowDesc), hipMemcpyHostToDevice, st));
	HIP_TRY_IN(who, k0.make());
	HIP_TRY_IN(who, k1.make());
	HIP_TRY_IN(who, hipEventRecord(k0, st));
	HIP_TRY_IN(who, launch_decode_windows(g->d_bin.p, g->d_starts.p, g->n_starts, d_win.p, n, d_out.p, st));
	HIP_TRY_IN(who, hipEventRecord(k1, st));
	HIP_TRY_IN(who, hipMemcpyAsync(host.data(), d_out.p, (size_t) total, hipMemcpyDeviceToHost, st));
	HIP_TRY_IN(who, hipStreamSynchronize(st));
	h->decode_kernel_ms = ev_ms(k0, k1);
	for (int i = 0; i < n; ++i) memcpy(out + out_offset[i], host.data() + win[(size_t) i].dst_off, (size_t) length[i]);
	return CVX_OK;
	ABI_GUARD_END
}

/* ------------------------------------------------------------------ candidate search (search half) */

struct cvx_index_s {             /* one unit of ngmlr's CompactPrefixTable, resident in HBM (cvx_search.hip) */
	int device = 0;
	int32_t k = 0;
	uint64_t n_index = 0;        /* 4^k + 2 */
	uint64_t unit_offset = 0;
	uint32_t n_locs = 0;
	DevBuf<uint2> d_rows;            /* (row start, row length | used << 31) per prefix: SearchArgs::rows */
	DevBuf<uint32_t> d_locs;
};

/* a table cvx_index_build_device(CVX_INDEX_KEEP_RESIDENT) left on its device: the next cvx_index_upload of these very host
 * arrays on that device takes it over instead of reading 4^k records on the host and copying a gigabyte back up */
struct ResidentTable {
	std::mutex mtx;
	int device = -1;
	int32_t k = 0;
	const void *index = nullptr;
	const uint32_t *locs = nullptr;
	uint64_t n_locs = 0;
	void *d_rows = nullptr;
	uint32_t *d_locs = nullptr;
	void drop() {      /* (mtx held) */
		if (device >= 0 && (d_rows || d_locs)) { (void) hipSetDevice(device); if (d_rows) (void) hipFree(d_rows); if (d_locs) (void) hipFree(d_locs); }
		device = -1; d_rows = nullptr; d_locs = nullptr; index = nullptr; locs = nullptr;
	}
} g_resident_table;

int cvx_index_upload(cvx_handle h, int32_t k, const void *index, const uint32_t *locs, uint32_t n_locs, uint64_t unit_offset, cvx_index *out) {
	ABI_GUARD_BEGIN
	if (!h || !out || !index || (n_locs > 0 && !locs) || k < 4 || k > 15) { set_err("cvx_index_upload: bad argument (kmer_len 4..15)"); return CVX_ERR_ARG; }
	*out = nullptr;
	HIP_TRY(hipSetDevice(h->device));
	const uint64_t n_index = (1ull << (2 * k)) + 2ull;
	{
		std::lock_guard<std::mutex> lk(g_resident_table.mtx);
		ResidentTable &r = g_resident_table;
		if (r.device == h->device && r.k == k && r.index == index && r.locs == locs && r.n_locs == n_locs && r.d_rows && r.d_locs) {
			cvx_index_s *ix = new (std::nothrow) cvx_index_s();
			if (!ix) return CVX_ERR_OOM;
			ix->device = h->device; ix->k = k; ix->n_index = n_index; ix->unit_offset = unit_offset; ix->n_locs = n_locs;
			ix->d_rows.p = static_cast<uint2 *>(r.d_rows); ix->d_rows.cap = (size_t) n_index - 1;
			ix->d_locs.p = r.d_locs; ix->d_locs.cap = (size_t) n_locs + 1;
			r.device = -1; r.d_rows = nullptr; r.d_locs = nullptr; r.index = nullptr; r.locs = nullptr;
			*out = ix;
			return CVX_OK;
		}
	}
	/* the 5-byte Index records (uint m_TabIndex; char m_RevCompIndex, #pragma pack(1): src/PrefixTable.h:15-31) as one 8-byte
	 * record per prefix: where GetRefEntry's row starts (m_TabIndex - 1), how long it is (the next record's m_TabIndex - this
	 * one's, PrefixTable.cpp:476-532) and Index::used() */
	const uint8_t *p = static_cast<const uint8_t *>(index);
	auto tab_at = [&](uint64_t i) { uint32_t t; memcpy(&t, p + 5 * i, 4); return t; };
	std::vector<uint2> rows;
	try { rows.resize((size_t) n_index - 1); } catch (const std::bad_alloc &) { set_err("cvx_index_upload: out of host memory"); return CVX_ERR_OOM; }
	for (uint64_t i = 0; i + 1 < n_index; ++i) {
		const uint32_t t0 = tab_at(i), t1 = tab_at(i + 1);
		const bool used = p[5 * i + 4] != 0;                  /* Index::used() */
		if (used && (t0 == 0 || t1 < t0 || (uint64_t) t1 - 1 > n_locs || t1 - t0 > 0x7FFFFFFFu)) {
			set_err("cvx_index_upload: index entry %llu points outside the %u locations", (unsigned long long) i, n_locs);
			return CVX_ERR_ARG;
		}
		rows[(size_t) i] = make_uint2(used ? t0 - 1u : 0u, used ? ((t1 - t0) | 0x80000000u) : 0u);
	}
	std::unique_ptr<cvx_index_s> ix(new (std::nothrow) cvx_index_s());
	if (!ix) return CVX_ERR_OOM;
	ix->device = h->device; ix->k = k; ix->n_index = n_index; ix->unit_offset = unit_offset; ix->n_locs = n_locs;
	RC_TRY(ix->d_rows.ensure(rows.size()));
	RC_TRY(ix->d_locs.ensure((size_t) n_locs + 1));
	HIP_TRY_IN("cvx_index_upload", hipMemcpy(ix->d_rows.p, rows.data(), rows.size() * sizeof(uint2), hipMemcpyHostToDevice));
	if (n_locs) HIP_TRY_IN("cvx_index_upload", hipMemcpy(ix->d_locs.p, locs, (size_t) n_locs * 4, hipMemcpyHostToDevice));
	*out = ix.release();      /* (the unique_ptr's: the caller owns the table from here) */
	return CVX_OK;
	ABI_GUARD_END
}

int cvx_index_build_device(int32_t device_id, const uint8_t *bin_ref, uint64_t n_nibbles, const uint64_t *start_table, const uint64_t *seq_lengths, int32_t n_seqs,
		int32_t kmer_len, int32_t ref_skip, int32_t bin_shift, void *ref_table_index, uint32_t *ref_table, uint64_t ref_table_capacity,
		uint64_t *n_locations, uint32_t flags) {
	ABI_GUARD_BEGIN
	if (!bin_ref || !start_table || !seq_lengths || n_seqs <= 0 || kmer_len < 4 || kmer_len > 15 || ref_skip < 0 || bin_shift < 0 || bin_shift > 30 ||
			!ref_table_index || !n_locations) { set_err("cvx_index_build_device: bad argument (kmer_len 4..15, bin_shift 0..30)"); return CVX_ERR_ARG; }
	for (int32_t s = 0; s < n_seqs; ++s) {
		if ((start_table[s] & 1ull) || start_table[s] + seq_lengths[s] > n_nibbles) { set_err("cvx_index_build_device: sequence %d does not start on a byte or leaves the genome", s); return CVX_ERR_ARG; }
		if (s > 0 && start_table[s] < start_table[s - 1]) { set_err("cvx_index_build_device: sequences out of order (a row lists its locations in walk order)"); return CVX_ERR_ARG; }
	}
	int ndev = 0;
	if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { (void) hipGetLastError(); set_err("cvx_index_build_device: no HIP device"); return CVX_ERR_NO_DEVICE; }
	if (device_id < 0 || device_id >= ndev) { set_err("cvx_index_build_device: device %d of %d", device_id, ndev); return CVX_ERR_ARG; }
	HIP_TRY(hipSetDevice(device_id));
	hipStream_t st = nullptr;
	HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
	char err[320];
	err[0] = 0;
	const bool keep = (flags & CVX_INDEX_KEEP_RESIDENT) != 0u;
	void *d_rows = nullptr;
	uint32_t *d_locs = nullptr;
	const int rc = index_build_device(bin_ref, n_nibbles, start_table, seq_lengths, n_seqs, kmer_len, ref_skip, bin_shift, ref_table_index, ref_table,
			ref_table_capacity, n_locations, st, err, sizeof(err), keep ? &d_rows : nullptr, keep ? &d_locs : nullptr);
	(void) hipStreamSynchronize(st);
	(void) hipStreamDestroy(st);
	if (rc != CVX_OK) set_err("cvx_index_build_device: %s", err);
	if (keep) {
		std::lock_guard<std::mutex> lk(g_resident_table.mtx);
		g_resident_table.drop();                                  /* one table waits at a time */
		if (rc == CVX_OK && d_rows && d_locs) {
			g_resident_table.device = device_id; g_resident_table.k = kmer_len; g_resident_table.index = ref_table_index; g_resident_table.locs = ref_table;
			g_resident_table.n_locs = *n_locations; g_resident_table.d_rows = d_rows; g_resident_table.d_locs = d_locs;
		}
	}
	return rc;
	ABI_GUARD_END
}

void cvx_index_free(cvx_handle h, cvx_index ix) {
	ABI_GUARD_BEGIN
	if (!ix) return;
	if (h) { (void) hipSetDevice(h->device); (void) hipDeviceSynchronize(); }
	delete ix;
	ABI_GUARD_END_VOID
}

} /* extern "C" */

namespace {

/* One call of the search: what its stages share, and the stages in the order search_common runs them.  Every decision -- layouts,
 * map sizes, the ladder, launches, budgets, regions, offsets -- is cvx_search_plan.h's; a stage issues what the plan says.
 *
 * A read starts on the wave-per-read kernel with its vote map in LDS (cvx_search.hip), in the smallest map that certainly holds
 * it.  A read that does not fit its map after all (more than 3 072 bins; a bin beyond 32 bits; longer than the sequence buffer) is
 * redone -- the same attempt, then the rest of the ladder -- by the same kernel over the real table in HBM, which needs the vote
 * count to size its lists.  Candidates of read i lie at d_cand + h_srcoff[i]: the slots of its map for an LDS-map read, the sparse
 * region behind all of those (two slots per vote) for the others. */
struct SearchCall {
	cvx_search_state *const ss;
	const hipStream_t st;
	const int32_t n;
	const size_t n1;
	const SearchTuning tune;
	bool classify = false;           /* votes counted first, reads sorted into launches by map size */
	SearchArgs a;
	SearchMeta m;                    /* typed views into ss->h_meta, ss->h_out and ss->h_srcoff */
	SearchOut o;
	uint64_t *h_srcoff = nullptr;    /* where each read's candidates lie in d_cand */
	const uint8_t *src = nullptr;    /* the caller's read block (the arena form) */
	bool zero_copy = false;          /* ... which lies in memory from cvx_host_alloc and travels as it is */
	uint64_t bytes = 0;              /* the reads with a NUL behind each */
	uint64_t fixed_total = 0;        /* candidate slots of all LDS-map reads */
	uint64_t total = 0;              /* votes of the reads that took an HBM form so far: their rList / candidate regions */
	uint64_t need = 0;               /* candidates of the call */
	bool counted = false;            /* o.events holds every read's votes */
	std::vector<uint8_t> has_region, map_log2;      /* per read; map_log2 0: not an LDS-map read */
	std::vector<int32_t> work_wave, work_hbm, next_wave, next_hbm, hbm_now;      /* reads of this attempt and of the next, per form */
	std::string tr;                  /* CVX_SEARCH_TRACE: who ran where, for how long */
	std::chrono::steady_clock::time_point tr0;

	SearchCall(cvx_handle h, int32_t n_) : ss(h->search), st(h->s_main), n(n_), n1((size_t) n_), tune(search_tuning_env()) { memset(&a, 0, sizeof(a)); }

	double tr_ms() const { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tr0).count(); }
	__attribute__((format(printf, 2, 3))) void note(const char *fmt, ...) {      /* (tune.trace) */
		char b[160];
		va_list ap;
		va_start(ap, fmt);
		vsnprintf(b, sizeof(b), fmt, ap);
		va_end(ap);
		tr += b;
	}

	/* the reads, a NUL behind each (the N-run scan of PrefixIteration relies on the terminator), in page-locked staging.  A block that
	 * lies in memory from cvx_host_alloc travels as it is: the host touches no base (the 64 bytes behind the last read that the kernels
	 * may read are cleared on the device) */
	int stage_reads(const char *const *seqs, const int32_t *lens, const uint8_t *arena, const uint64_t *offsets) {
		const int32_t bad = arena ? search_arena_reads_check(n, arena, offsets, &bytes) : search_string_reads_check(n, seqs, lens, &bytes);
		if (bad >= 0 && arena) { set_err("cvx_search_batch_arena: read %d is not [offsets[i], offsets[i + 1] - 1) followed by a NUL", bad); return CVX_ERR_ARG; }
		if (bad >= 0) { set_err("cvx_search_batch: bad read %d", bad); return CVX_ERR_ARG; }
		src = arena ? arena + offsets[0] : nullptr;
		zero_copy = arena && in_pinned_block(reinterpret_cast<const char *>(src), bytes + 4);
		if (!zero_copy) RC_TRY(ss->h_seq.ensure((size_t) bytes + 64));
		RC_TRY(ss->h_meta.ensure(search_meta_bytes(n1)));
		RC_TRY(ss->h_out.ensure(search_out_bytes(n1)));
		m = search_meta_view(ss->h_meta.p, n1);
		o = search_out_view(ss->h_out.p, n1);
		uint8_t *hseq = zero_copy ? nullptr : ss->h_seq.as<uint8_t>();
		if (arena) {
			search_arena_reads_layout(n, offsets, m.off, m.len);
			if (!zero_copy) memcpy(hseq, src, (size_t) bytes);
		} else {
			search_string_reads_layout(n, lens, m.off, m.len);
			for (int i = 0; i < n; ++i) { memcpy(hseq + m.off[i], seqs[i], (size_t) lens[i]); hseq[m.off[i] + (uint64_t) lens[i]] = 0; }
		}
		if (!zero_copy) memset(hseq + bytes, 0, 64);
		return CVX_OK;
	}

	/* the device's side of the call -- its per-read arrays, the kernels' arguments -- and the reads and their layout on their way up */
	int upload(const cvx_index_s *ix, float sensitivity, float min_hits, int32_t bin_shift) {
		RC_TRY(ss->d_seq.ensure((size_t) bytes + 64));
		RC_TRY(ss->d_off.ensure(n1)); RC_TRY(ss->d_listoff.ensure(n1)); RC_TRY(ss->d_begin.ensure(n1 + 1));
		RC_TRY(ss->d_len.ensure(n1)); RC_TRY(ss->d_ncand.ensure(n1)); RC_TRY(ss->d_work.ensure(n1)); RC_TRY(ss->d_miss.ensure(n1));
		RC_TRY(ss->d_events.ensure(n1)); RC_TRY(ss->d_maxhit.ensure(n1));
		a.rows = ix->d_rows.p; a.locs = ix->d_locs.p; a.unit_offset = ix->unit_offset; a.k = ix->k;
		a.seq = ss->d_seq.p; a.seq_off = ss->d_off.p; a.seq_len = ss->d_len.p; a.n = n;
		a.events = ss->d_events.p; a.list_off = ss->d_listoff.p; a.n_cand = ss->d_ncand.p; a.max_hit = ss->d_maxhit.p; a.kmer_misses = ss->d_miss.p;
		a.sensitivity = sensitivity; a.min_hits = min_hits; a.bin_shift = bin_shift;
		if (zero_copy) {
			HIP_TRY(hipMemsetAsync(ss->d_seq.p + bytes / 4 * 4, 0, 68, st));      /* what lies behind the block, first: the copy below is rounded up to whole dwords */
			HIP_TRY(hipMemcpyAsync(ss->d_seq.p, src, (size_t) ((bytes + 3) / 4 * 4), hipMemcpyHostToDevice, st));
		} else {
			HIP_TRY(hipMemcpyAsync(ss->d_seq.p, ss->h_seq.p, (size_t) ((bytes + 63) / 4 * 4), hipMemcpyHostToDevice, st));
		}
		HIP_TRY(hipMemcpyAsync(ss->d_off.p, m.off, n1 * 8, hipMemcpyHostToDevice, st));
		HIP_TRY(hipMemcpyAsync(ss->d_len.p, m.len, n1 * 4, hipMemcpyHostToDevice, st));
		HIP_TRY(hipMemsetAsync(ss->d_miss.p, 0, n1 * 4, st));
		HIP_TRY(hipMemsetAsync(ss->d_maxhit.p, 0, n1 * 4, st));
		classify = search_classify(tune, n, ix->n_locs, ix->n_index);
		ss->kev_used = 0;
		ss->kernel_ms = 0.0f;
		return CVX_OK;
	}

	/* votes per read (all reads: the pass is cheap): map sizes, sizes of the HBM kernel's lists */
	int count_votes() {
		RC_TRY(ss->kmark(st));
		HIP_TRY(launch_search_count(a, st));
		RC_TRY(ss->kmark(st));
		HIP_TRY(hipMemcpyAsync(o.events, ss->d_events.p, n1 * 8, hipMemcpyDeviceToHost, st));
		RC_TRY(search_wait(ss, st));
		counted = true;
		return CVX_OK;
	}

	/* every read's map and where its candidates lie; the arena for the LDS-map reads' */
	int assign_maps() {
		has_region.assign(n1, 0);
		map_log2.assign(n1, 0);
		RC_TRY(ss->d_srcoff.ensure(n1));
		RC_TRY(ss->h_srcoff.ensure(n1 * 8));
		h_srcoff = ss->h_srcoff.as<uint64_t>();
		fixed_total = search_assign_maps(tune, classify, n, m.len, o.events, map_log2.data(), h_srcoff);
		RC_TRY(ss->d_cand.ensure((size_t) fixed_total + 64));
		HIP_TRY(hipMemcpyAsync(ss->d_srcoff.p, h_srcoff, n1 * 8, hipMemcpyHostToDevice, st));
		return CVX_OK;
	}

	/* one attempt of the reads on the LDS form: one launch per map size, back to back (the work list holds the sizes' reads one
	 * after the other), then their flags: done, out of budget (the next attempt), or not for this map (the HBM form, this attempt) */
	int wave_attempt(int bits) {
		SearchWaveLaunch launches[kSearchWaveSizes];
		const int n_launches = search_wave_launches(tune, bits, work_wave, map_log2.data(), m.len, m.work, launches);
		a.cand = ss->d_cand.p; a.cand_off = ss->d_srcoff.p;
		for (int k = 0; k < n_launches; ++k) {
			const SearchWaveLaunch &w = launches[k];
			HIP_TRY(hipMemcpyAsync(ss->d_work.p + w.first, m.work + w.first, w.count * 4, hipMemcpyHostToDevice, st));
			a.work = ss->d_work.p + w.first;
			a.n_work = (int32_t) w.count;
			RC_TRY(ss->kmark(st));
			HIP_TRY(launch_search_wave(a, w.log2, w.seq_cap, w.slot8, st));
			RC_TRY(ss->kmark(st));
			if (tune.trace) note(" [2^%d-slot maps: %zu reads]", w.log2, w.count);
		}
		a.work = ss->d_work.p;
		HIP_TRY(hipMemcpyAsync(o.ncand, ss->d_ncand.p, n1 * 4, hipMemcpyDeviceToHost, st));
		RC_TRY(search_wait(ss, st));
		for (int32_t i : work_wave) {
			if (o.ncand[i] == kSearchNeedsHbm) hbm_now.push_back(i);
			else if (o.ncand[i] < 0) next_wave.push_back(i);
		}
		if (tune.trace) note(" [bits %d wave %zu -> %zu to hbm, %zu retry, at %.2f ms]", bits, work_wave.size(), hbm_now.size() - work_hbm.size(), next_wave.size(), tr_ms());
		return CVX_OK;
	}

	/* regions for the reads of hbm_now that have none yet; the candidate arena grows without losing the lists already in it */
	int give_regions() {
		if (!search_give_regions(hbm_now, o.events, has_region.data(), m.list_off, &total)) return CVX_OK;
		RC_TRY(ss->d_rlist.ensure((size_t) total + 64));
		if (ss->d_cand.cap < search_cand_needed(fixed_total, total)) {
			DevBuf<SearchCandidate> bigger;
			RC_TRY(bigger.ensure(search_cand_grown(fixed_total, total)));
			HIP_TRY_IN("cvx_search_batch", hipMemcpyAsync(bigger.p, ss->d_cand.p, ss->d_cand.cap * sizeof(SearchCandidate), hipMemcpyDeviceToDevice, st));
			RC_TRY(search_wait(ss, st));
			ss->d_cand = std::move(bigger);      /* (frees the old arena: the copy out of it is done) */
		}
		HIP_TRY(hipMemcpyAsync(ss->d_listoff.p, m.list_off, n1 * 8, hipMemcpyHostToDevice, st));
		return CVX_OK;
	}

	/* hbm_now in one launch of the wave-per-read kernel over tables in HBM.  The tables belong to the waves and are empty between
	 * launches -- a wave frees the slots a read opened when the read is done -- so they are cleared when they are allocated, when the
	 * table size changes and after a launch that failed, not per read */
	int launch_hbm_tables(int bits) {
		RC_TRY(ss->d_undo.ensure((size_t) total + 64));
		a.undo = ss->d_undo.p;
		const size_t n_tables = search_hbm_tables(hbm_now.size(), bits), need_words = search_hbm_table_words(n_tables, bits);
		if (ss->d_keys.cap < need_words) { RC_TRY(ss->d_keys.ensure(need_words)); ss->tables_clean_words = 0; }
		if (ss->tables_clean_words < need_words) {
			HIP_TRY(hipMemsetAsync(ss->d_keys.p, 0xFF, ss->d_keys.cap * 8, st));      /* (scores of a free slot are never read) */
			ss->tables_clean_words = ss->d_keys.cap;
		}
		RC_TRY(ss->d_ticket.ensure(16));
		HIP_TRY(hipMemsetAsync(ss->d_ticket.p, 0, 4, st));
		a.keys = ss->d_keys.p;
		memcpy(m.work, hbm_now.data(), hbm_now.size() * 4);
		HIP_TRY(hipMemcpyAsync(ss->d_work.p, m.work, hbm_now.size() * 4, hipMemcpyHostToDevice, st));
		a.n_work = (int32_t) hbm_now.size();
		ss->tables_clean_words = 0;                     /* until the launch is known to have ended (hbm_attempt) */
		RC_TRY(ss->kmark(st));
		HIP_TRY(launch_search_wave_hbm(a, (int) n_tables, ss->d_ticket.p, st));
		RC_TRY(ss->kmark(st));
		return CVX_OK;
	}

	/* hbm_now on the lane-per-read kernel, a table per read: in chunks of as many reads as the table budget holds */
	int launch_lane_chunks(int bits) {
		const size_t chunk = search_lane_chunk(hbm_now.size(), bits);
		ss->tables_clean_words = 0;                         /* the lane-per-read kernel leaves its tables as they are */
		RC_TRY(ss->d_keys.ensure(search_lane_keys(chunk, bits)));
		RC_TRY(ss->d_scores.ensure(search_lane_scores(chunk, bits)));
		a.keys = ss->d_keys.p; a.scores = ss->d_scores.p;
		for (size_t w0 = 0; w0 < hbm_now.size(); w0 += chunk) {
			const size_t k = std::min(chunk, hbm_now.size() - w0);
			memcpy(m.work, hbm_now.data() + w0, k * 4);
			HIP_TRY(hipMemcpyAsync(ss->d_work.p, m.work, k * 4, hipMemcpyHostToDevice, st));
			HIP_TRY(hipMemsetAsync(ss->d_keys.p, 0xFF, search_lane_keys(k, bits) * 8, st));          /* every slot empty */
			a.n_work = (int32_t) k;
			RC_TRY(ss->kmark(st));
			HIP_TRY(launch_search(a, st));
			RC_TRY(ss->kmark(st));
			if (w0 + chunk < hbm_now.size()) RC_TRY(search_wait(ss, st));      /* (the work list is reused by the next chunk) */
		}
		return CVX_OK;
	}

	/* one attempt of the reads on an HBM form -- those of the last attempt and those the LDS form has just sent -- and their flags */
	int hbm_attempt(int bits) {
		a.work = ss->d_work.p;
		if (!counted) RC_TRY(count_votes());
		RC_TRY(give_regions());
		for (int32_t i : hbm_now) h_srcoff[i] = search_hbm_src_off(fixed_total, m.list_off[i]);
		a.rlist = ss->d_rlist.p; a.cand = ss->d_cand.p + fixed_total;
		RC_TRY(tune.lane_serial ? launch_lane_chunks(bits) : launch_hbm_tables(bits));
		HIP_TRY(hipMemcpyAsync(o.ncand, ss->d_ncand.p, n1 * 4, hipMemcpyDeviceToHost, st));
		RC_TRY(search_wait(ss, st));
		if (!tune.lane_serial) ss->tables_clean_words = ss->d_keys.cap;      /* the launch ended: every wave left its table empty */
		for (int32_t i : hbm_now) if (o.ncand[i] < 0) next_hbm.push_back(i);
		if (tune.trace) note(" [bits %d hbm %zu (%llu votes in the call) -> %zu retry, at %.2f ms]", bits, hbm_now.size(), (unsigned long long) total, next_hbm.size(), tr_ms());
		return CVX_OK;
	}

	/* the retry ladder (search_ladder_bits): every attempt takes the reads the one before left without a list, each on its form; a
	 * read that leaves the ladder without a list keeps -1 (one still flagged for the HBM form cannot remain: it was redone in its attempt) */
	int climb(int32_t first_bits) {
		tr0 = std::chrono::steady_clock::now();
		for (int i = 0; i < n; ++i) (map_log2[(size_t) i] ? work_wave : work_hbm).push_back(i);
		ss->attempts.assign(n1, 0);
		for (int attempt = 0; !work_wave.empty() || !work_hbm.empty(); ++attempt) {
			const int bits = search_ladder_bits(first_bits, attempt);
			if (bits > kSearchLadderMaxBits) break;
			for (int32_t i : work_wave) ss->attempts[(size_t) i] += 1;
			for (int32_t i : work_hbm) ss->attempts[(size_t) i] += 1;
			a.bits = bits;
			a.hpoc_factor = search_ladder_factor(attempt);
			next_wave.clear(); next_hbm.clear();
			hbm_now = work_hbm;
			if (!work_wave.empty()) RC_TRY(wave_attempt(bits));
			if (!hbm_now.empty()) RC_TRY(hbm_attempt(bits));
			work_wave.swap(next_wave);
			work_hbm.swap(next_hbm);
		}
		return CVX_OK;
	}

	/* the dense candidate list in read order, compacted on the device: only the entries come back (the sparse arena is two slots per vote) */
	int compact() {
		RC_TRY(ss->d_dense.ensure((size_t) need + 64));
		HIP_TRY(hipMemcpyAsync(ss->d_begin.p, m.begin, (n1 + 1) * 8, hipMemcpyHostToDevice, st));
		HIP_TRY(hipMemcpyAsync(ss->d_srcoff.p, h_srcoff, n1 * 8, hipMemcpyHostToDevice, st));
		RC_TRY(ss->kmark(st));
		HIP_TRY(launch_search_compact(ss->d_cand.p, ss->d_srcoff.p, ss->d_ncand.p, ss->d_begin.p, ss->d_dense.p, n, st));
		RC_TRY(ss->kmark(st));
		return CVX_OK;
	}

	/* The scoring of every candidate, queued behind the compaction: the lists are planned where they lie (d_dense), the strings come
	 * from the resident genome and from the read block the vote has just used, and both launchers run over all `need` slots -- a
	 * candidate that is not scored is two empty strings there.  Nothing is uploaded. */
	int queue_scoring(const SearchScoreArgs &fs) {
		const CandWinSlots slots = cand_windows_slots(fs.buffer_len, fs.max_read_bytes, need);
		RC_TRY(ss->d_fdesc.ensure((size_t) need)); RC_TRY(ss->d_fpairs.ensure((size_t) need));
		RC_TRY(ss->d_fout.ensure((size_t) need)); RC_TRY(ss->d_fstatus.ensure((size_t) need));
		RC_TRY(ss->d_fseq.ensure((size_t) slots.seq_bytes + 256));
		RC_TRY(ss->h_fout.ensure((size_t) need * 8));
		HIP_TRY(ss->ev_f0.make());
		HIP_TRY(ss->ev_f1.make());
		HIP_TRY(hipEventRecord(ss->ev_f0, st));
		HIP_TRY(launch_plan_candidate_windows(ss->d_dense.p, ss->d_begin.p, ss->d_ncand.p, ss->d_off.p, ss->d_len.p, n, need,
				score_windows_concat_len(fs.g->n_nibbles), fs.buffer_len, fs.window_lead, fs.max_cmrs, slots, ss->d_fdesc.p, ss->d_fstatus.p, st));
		HIP_TRY(launch_stage_score_windows(fs.g->d_bin.p, ss->d_seq.p, ss->d_fdesc.p, (int) need, ss->d_fseq.p, ss->d_fpairs.p, st));
		HIP_TRY(launch_score_diag(ss->d_fseq.p, ss->d_fpairs.p, ss->d_fout.p, (int) need, st));
		HIP_TRY(hipEventRecord(ss->ev_f1, st));
		return CVX_OK;
	}

	/* what the call hands back: the lists dense in the caller's arena (and their scores), the per-read counts, offsets and extras */
	int bring_back(const SearchScoreArgs *fs, int32_t *n_candidates, uint64_t *cand_begin, cvx_candidate *cands, uint64_t cand_capacity, uint64_t *cand_used,
			float *max_hit, int32_t *kmer_misses) {
		need = search_dense_offsets(n, o.ncand, m.begin, cand_begin, n_candidates);
		if (cand_used) *cand_used = need;
		/* (the launchers behind the compaction count slots in an int; refused here, where nothing of the call is queued any more) */
		if (fs && need > 0x7fffffffull) { set_err("cvx_search_score_arena: %llu candidates in one call", (unsigned long long) need); return CVX_ERR_ARG; }
		if (max_hit || kmer_misses) {
			HIP_TRY(hipMemcpyAsync(o.maxhit, ss->d_maxhit.p, n1 * 4, hipMemcpyDeviceToHost, st));
			HIP_TRY(hipMemcpyAsync(o.miss, ss->d_miss.p, n1 * 4, hipMemcpyDeviceToHost, st));
		}
		if (need > cand_capacity || (need > 0 && !cands)) {
			if (max_hit || kmer_misses) RC_TRY(search_wait(ss, st));
			set_err("cvx_search_batch: candidate arena too small (%llu needed, %llu given)", (unsigned long long) need, (unsigned long long) cand_capacity);
			return CVX_ERR_CAPACITY;
		}
		if (need) {
			RC_TRY(compact());
			if (fs) RC_TRY(queue_scoring(*fs));
			/* (straight into the caller's memory: pageable unless it came from cvx_host_alloc, then the copy is staged by the runtime) */
			HIP_TRY(hipMemcpyAsync(cands, ss->d_dense.p, (size_t) need * sizeof(SearchCandidate), hipMemcpyDeviceToHost, st));
			if (fs) {
				HIP_TRY(hipMemcpyAsync(ss->h_fout.p, ss->d_fout.p, (size_t) need * 4, hipMemcpyDeviceToHost, st));
				HIP_TRY(hipMemcpyAsync(ss->h_fout.as<uint8_t>() + (size_t) need * 4, ss->d_fstatus.p, (size_t) need * 4, hipMemcpyDeviceToHost, st));
			}
		}
		RC_TRY(search_wait(ss, st));
		for (size_t q = 0; q + 1 < ss->kev_used; q += 2) ss->kernel_ms += ev_ms(ss->kev[q], ss->kev[q + 1]);
		if (fs && need) {
			ss->fused_ms = ev_ms(ss->ev_f0, ss->ev_f1);
			const float *out = ss->h_fout.as<float>();
			const int32_t *status = reinterpret_cast<const int32_t *>(out + need);
			for (uint64_t q = 0; q < need; ++q) fs->sw_scores[q] = status[q] == kCandScored ? out[q] : -1.0f;
			if (fs->sw_status) memcpy(fs->sw_status, status, (size_t) need * 4);
		}
		if (tune.trace) fprintf(stderr, "cvx_search_batch: %d reads, %llu bases, %llu candidates, %.2f ms:%s\n", n, (unsigned long long) bytes - (unsigned long long) n, (unsigned long long) need, tr_ms(), tr.c_str());
		if (max_hit) memcpy(max_hit, o.maxhit, n1 * 4);
		if (kmer_misses) memcpy(kmer_misses, o.miss, n1 * 4);
		return CVX_OK;
	}
};

}  // namespace

/* the reads either as n NUL-terminated strings (seqs / lens) or back to back in one block (arena / offsets: read i =
 * arena[offsets[i] .. offsets[i + 1] - 1) with a NUL at offsets[i + 1] - 1) */
static int search_common(cvx_handle h, cvx_index ix, int32_t n, const char *const *seqs, const int32_t *lens, const uint8_t *arena, const uint64_t *offsets,
		float sensitivity, float min_hits, int32_t bin_shift, int32_t first_bits,
		int32_t *n_candidates, uint64_t *cand_begin, cvx_candidate *cands, uint64_t cand_capacity, uint64_t *cand_used,
		float *max_hit, int32_t *kmer_misses, const SearchScoreArgs *fs = nullptr) {
	static_assert(sizeof(SearchCandidate) == sizeof(cvx_candidate), "SearchCandidate mirrors cvx_candidate");
	/* bin_shift >= 1: the "bin is listed" flag lives in bit 63 of the vote table's key, and with a shift of 0 a vote near the
	 * start of the genome (location - offset in the read < 0) would set that bit itself; ngmlr's bin size is 4 */
	if (!h || !ix || n < 0 || (n > 0 && ((!arena && (!seqs || !lens)) || (arena && !offsets) || !n_candidates || !cand_begin)) || bin_shift < 1 || bin_shift > 30 ||
			(first_bits != 0 && (first_bits < 8 || first_bits > 20))) {
		set_err("cvx_search_batch: bad argument (bin_shift 1..30, first_bits 0 or 8..20)"); return CVX_ERR_ARG;
	}
	if (ix->device != h->device) { set_err("cvx_search_batch: the index lives on device %d, the handle on %d", ix->device, h->device); return CVX_ERR_ARG; }
	if (cand_used) *cand_used = 0;
	if (fs && h->search) h->search->fused_ms = 0.0f;      /* (CVX_STAGE_SEARCH_SCORE is this call's from here on, also when it launches nothing) */
	if (n == 0) return CVX_OK;
	HIP_TRY(hipSetDevice(h->device));
	if (!h->search) { h->search = new (std::nothrow) cvx_search_state(); if (!h->search) return CVX_ERR_OOM; }
	SearchCall c(h, n);
	RC_TRY(c.stage_reads(seqs, lens, arena, offsets));
	RC_TRY(c.upload(ix, sensitivity, min_hits, bin_shift));
	if (c.classify) RC_TRY(c.count_votes());
	RC_TRY(c.assign_maps());
	RC_TRY(c.climb(first_bits));
	return c.bring_back(fs, n_candidates, cand_begin, cands, cand_capacity, cand_used, max_hit, kmer_misses);
}

extern "C" {

int cvx_search_batch_ex(cvx_handle h, cvx_index ix, int32_t n, const char *const *seqs, const int32_t *lens,
		float sensitivity, float min_hits, int32_t bin_shift, int32_t first_bits,
		int32_t *n_candidates, uint64_t *cand_begin, cvx_candidate *cands, uint64_t cand_capacity, uint64_t *cand_used,
		float *max_hit, int32_t *kmer_misses) {
	ABI_GUARD_BEGIN return search_common(h, ix, n, seqs, lens, nullptr, nullptr, sensitivity, min_hits, bin_shift, first_bits, n_candidates, cand_begin, cands, cand_capacity, cand_used, max_hit, kmer_misses); ABI_GUARD_END
}

int cvx_search_batch_arena(cvx_handle h, cvx_index ix, int32_t n, const uint8_t *arena, const uint64_t *offsets,
		float sensitivity, float min_hits, int32_t bin_shift, int32_t first_bits,
		int32_t *n_candidates, uint64_t *cand_begin, cvx_candidate *cands, uint64_t cand_capacity, uint64_t *cand_used,
		float *max_hit, int32_t *kmer_misses) {
	ABI_GUARD_BEGIN
	if (n > 0 && (!arena || !offsets)) { set_err("cvx_search_batch_arena: NULL arena"); return CVX_ERR_ARG; }
	return search_common(h, ix, n, nullptr, nullptr, arena ? arena : reinterpret_cast<const uint8_t *>(""), offsets, sensitivity, min_hits, bin_shift, first_bits, n_candidates, cand_begin, cands, cand_capacity, cand_used, max_hit, kmer_misses);
	ABI_GUARD_END
}

int cvx_search_score_arena(cvx_handle h, cvx_index ix, cvx_genome g, int32_t n, const uint8_t *arena, const uint64_t *offsets,
		float sensitivity, float min_hits, int32_t bin_shift, int32_t first_bits,
		int32_t buffer_len, int32_t window_lead, int32_t max_cmrs,
		int32_t *n_candidates, uint64_t *cand_begin, cvx_candidate *cands, uint64_t cand_capacity, uint64_t *cand_used,
		float *max_hit, int32_t *kmer_misses, float *sw_scores, int32_t *sw_status) {
	ABI_GUARD_BEGIN
	if (!h || !g || (n > 0 && (!arena || !offsets))) { set_err("cvx_search_score_arena: NULL handle, genome or arena"); return CVX_ERR_ARG; }
	if (g->device != h->device) { set_err("cvx_search_score_arena: the genome lies on device %d, the handle on %d", g->device, h->device); return CVX_ERR_ARG; }
	/* The shape score_diag_kernel takes: reads of at most 511 characters (its exactness needs min(Q, R) <= 512 with the NULs) and a
	 * window of at most 2 048 characters.  score_class draws its line at 2 048 bytes WITH the NUL, and one window of buffer_len
	 * 2 048 is a byte longer: the 'x' tail behind an odd position gives 2 048 characters.  The two-call path scores that pair with
	 * the wave kernel; here it goes to score_diag_kernel like the rest, which holds it -- its row of reference codes is
	 * kDiagMaxRef + 64 = 2 112 bytes (cvx_score.hip) and the result is exact whatever R is -- and returns the same float
	 * (tests/test_gpu_search_score.py pins that shape against the two calls, tests/cpp/cand_windows_logic_test.cpp its slot). */
	if (buffer_len < 3 || buffer_len > 2048 || max_cmrs < 1 || window_lead < 0) {
		set_err("cvx_search_score_arena: buffer_len %d (3..2048), window_lead %d (>= 0), max_cmrs %d (>= 1)", buffer_len, window_lead, max_cmrs); return CVX_ERR_ARG;
	}
	if (cand_capacity > 0 && !sw_scores) { set_err("cvx_search_score_arena: NULL sw_scores"); return CVX_ERR_ARG; }
	SearchScoreArgs fs = {g, buffer_len, window_lead, max_cmrs, 1, sw_scores, sw_status};
	for (int32_t i = 0; i < n; ++i) {
		if (offsets[i + 1] <= offsets[i]) continue;      /* (refused by the search, with its own message) */
		const uint64_t rb = offsets[i + 1] - offsets[i];
		if (rb > 512) { set_err("cvx_search_score_arena: read %d has %llu characters (at most 511: the diagonal kernel's shape)", i, (unsigned long long) rb - 1); return CVX_ERR_ARG; }
		fs.max_read_bytes = std::max(fs.max_read_bytes, rb);
	}
	return search_common(h, ix, n, nullptr, nullptr, arena ? arena : reinterpret_cast<const uint8_t *>(""), offsets, sensitivity, min_hits, bin_shift, first_bits,
			n_candidates, cand_begin, cands, cand_capacity, cand_used, max_hit, kmer_misses, &fs);
	ABI_GUARD_END
}

int cvx_search_last_attempts(cvx_handle h, int32_t n, int32_t *attempts) {
	ABI_GUARD_BEGIN
	if (!h || n < 0 || (n > 0 && !attempts)) { set_err("cvx_search_last_attempts: bad argument"); return CVX_ERR_ARG; }
	if (!h->search || (size_t) n > h->search->attempts.size()) { set_err("cvx_search_last_attempts: the handle's last search had fewer than %d reads", n); return CVX_ERR_ARG; }
	if (n) memcpy(attempts, h->search->attempts.data(), (size_t) n * sizeof(int32_t));
	return CVX_OK;
	ABI_GUARD_END
}

int cvx_search_batch(cvx_handle h, cvx_index ix, int32_t n, const char *const *seqs, const int32_t *lens,
		float sensitivity, float min_hits, int32_t bin_shift,
		int32_t *n_candidates, uint64_t *cand_begin, cvx_candidate *cands, uint64_t cand_capacity, uint64_t *cand_used) {
	ABI_GUARD_BEGIN return cvx_search_batch_ex(h, ix, n, seqs, lens, sensitivity, min_hits, bin_shift, 0, n_candidates, cand_begin, cands, cand_capacity, cand_used, nullptr, nullptr); ABI_GUARD_END
}

}  /* extern "C" */
