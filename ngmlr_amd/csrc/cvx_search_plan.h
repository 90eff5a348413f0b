/*
 * cvx_search_plan.h -- the host half of the candidate search (cvx_search_batch and its siblings): what one call decides before and
 * between its launches -- the knobs it runs under, the layout of its staging blocks and of the reads, which LDS map a read gets
 * and where its candidates lie, the reference's retry ladder (CS.cpp:345-394), one attempt's launches by map size, the table
 * budget of the HBM forms, the regions handed to the reads that get there, and the dense offsets of the lists that come back.
 * cvx_rt_search.cpp only issues what these functions say.
 * Header-only and free of HIP calls -- it compiles with a plain C++ compiler over a stand-in for the runtime's types -- so that
 * the CPU suite can exercise it (tests/cpp/search_plan_test.cpp).
 */
#ifndef CVX_SEARCH_PLAN_H
#define CVX_SEARCH_PLAN_H

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <vector>

#include "cvx_launch.h"

namespace cvx {

/* ------------------------------------------------------------------ the knobs of one call */

/* CVX_TUNE_SEARCH_WAVE = 1 (the default): a read starts on the wave-per-read kernel with its vote map in LDS; = 2 sends every read
 * to the HBM-table form, = 0 to the lane-per-read kernel (one serial chain of votes per read; an independent implementation:
 * tests, A/B).  CVX_TUNE_SEARCH_CLASSIFY: reads per call from which the votes are counted first (2 048).
 * CVX_TUNE_SEARCH_LOG2 = 9..12 forces one map size (tests: a small one sends most reads through the fall-back).
 * CVX_TUNE_SEARCH_SLOT8 = 0 / 1: the 8-byte map never / wherever its 16-bit virtual slots allow.  CVX_SEARCH_TRACE: one line per
 * call on stderr. */
struct SearchTuning {
	bool use_wave = true, lane_serial = false;
	int classify_min = 2048;
	int forced_log2 = 0;         /* 0: not forced */
	int slot8 = -1;              /* -1: unset */
	bool trace = false;
};
/* each argument: the variable's text, NULL when it is not set */
inline SearchTuning search_tuning(const char *wave, const char *classify, const char *log2, const char *slot8, const char *trace) {
	SearchTuning t;
	const int wave_mode = wave ? atoi(wave) : 1;
	t.use_wave = wave_mode == 1;
	t.lane_serial = wave_mode == 0;
	t.classify_min = classify ? atoi(classify) : 2048;
	t.forced_log2 = log2 ? std::min(kSearchWaveLog2Max, std::max(kSearchWaveLog2Min, atoi(log2))) : 0;
	t.slot8 = slot8 ? (atoi(slot8) != 0 ? 1 : 0) : -1;
	t.trace = trace != nullptr;
	return t;
}
/* (read per call, not per process: the parity tests switch the variables inside one process) */
inline SearchTuning search_tuning_env() {
	return search_tuning(getenv("CVX_TUNE_SEARCH_WAVE"), getenv("CVX_TUNE_SEARCH_CLASSIFY"), getenv("CVX_TUNE_SEARCH_LOG2"),
			getenv("CVX_TUNE_SEARCH_SLOT8"), getenv("CVX_SEARCH_TRACE"));
}

/* A call of classify_min reads or more counts every read's votes first (one cheap kernel and one round trip) and sorts the reads
 * into launches by map size, so that as many reads as possible share a CU; a smaller call takes the default map for every read
 * without counting (its reads do not fill the device anyway).  A table with three locations per k-mer and more -- a genome of
 * 600 Mbp and up at ngmlr's defaults -- gives a 256-base read 1 500 votes and more: the one-size map of a small call would not
 * hold it, so its reads are counted and sorted as well. */
inline bool search_classify(const SearchTuning &t, int32_t n, uint64_t n_locs, uint64_t n_index) {
	const bool big_table = n_locs >= 3ull * (n_index - 2ull);
	return t.use_wave && !t.forced_log2 && (n >= t.classify_min || big_table);
}

/* ------------------------------------------------------------------ the two staging blocks */

/* meta: [off u64 n][list_off u64 n][begin u64 n + 1][len i32 n][work i32 n] */
struct SearchMeta {
	uint64_t *off, *list_off, *begin;
	int32_t *len, *work;
};
inline size_t search_meta_bytes(size_t n) { return n * (8 + 8 + 8 + 4 + 4) + 8 + 64; }
inline SearchMeta search_meta_view(void *block, size_t n) {
	SearchMeta m;
	m.off = static_cast<uint64_t *>(block);
	m.list_off = m.off + n;
	m.begin = m.list_off + n;
	m.len = reinterpret_cast<int32_t *>(m.begin + n + 1);
	m.work = m.len + n;
	return m;
}
/* out: [events u64 n][ncand i32 n][miss i32 n][maxhit f32 n] (the dense candidates have a buffer of their own) */
struct SearchOut {
	unsigned long long *events;
	int32_t *ncand, *miss;
	float *maxhit;
};
inline size_t search_out_bytes(size_t n) { return n * (8 + 4 + 4 + 4) + 64; }
inline SearchOut search_out_view(void *block, size_t n) {
	SearchOut o;
	o.events = static_cast<unsigned long long *>(block);
	o.ncand = reinterpret_cast<int32_t *>(o.events + n);
	o.miss = o.ncand + n;
	o.maxhit = reinterpret_cast<float *>(o.miss + n);
	return o;
}

/* ------------------------------------------------------------------ the reads */

/* The reads either back to back in one block (read i = arena[offsets[i] .. offsets[i + 1] - 1) with a NUL at offsets[i + 1] - 1)
 * or as n strings (seqs / lens).  The checks return the first read that is not of that form, -1 when all are, and then *bytes =
 * the reads with a NUL behind each; the layouts give read i's first byte in that block and its length without the NUL. */
inline int32_t search_arena_reads_check(int32_t n, const uint8_t *arena, const uint64_t *offsets, uint64_t *bytes) {
	for (int32_t i = 0; i < n; ++i)
		if (offsets[i + 1] <= offsets[i] || offsets[i + 1] - offsets[i] > 0x7FFFFFFFull || arena[offsets[i + 1] - 1] != 0) return i;
	*bytes = offsets[n] - offsets[0];
	return -1;
}
inline void search_arena_reads_layout(int32_t n, const uint64_t *offsets, uint64_t *off, int32_t *len) {
	for (int32_t i = 0; i < n; ++i) { off[i] = offsets[i] - offsets[0]; len[i] = (int32_t) (offsets[i + 1] - offsets[i] - 1); }
}
inline int32_t search_string_reads_check(int32_t n, const char *const *seqs, const int32_t *lens, uint64_t *bytes) {
	uint64_t total = 0;
	for (int32_t i = 0; i < n; ++i) {
		if (!seqs[i] || lens[i] < 0) return i;
		total += (uint64_t) lens[i] + 1;
	}
	*bytes = total;
	return -1;
}
inline void search_string_reads_layout(int32_t n, const int32_t *lens, uint64_t *off, int32_t *len) {
	uint64_t at = 0;
	for (int32_t i = 0; i < n; ++i) { off[i] = at; len[i] = lens[i]; at += (uint64_t) lens[i] + 1; }
}

/* ------------------------------------------------------------------ LDS maps and candidate slots */

/* A read starts in the smallest LDS map that certainly holds it: the forced size, else search_wave_log2 of its votes when the call
 * is classified -- 6 KB of LDS for a read of <= 384 votes, 24 KB for <= 1 536, 48 KB above -- else the default.  map_log2[i] = 0:
 * not an LDS-map read (the wave form is off, or the read with its NUL is longer than the kernel's sequence buffer).  Candidates
 * of read i lie at src_off[i] of the candidate arena: two per bin its map can hold (or per vote, when the call is classified and
 * that is fewer); a read without a map gets none here and keeps the running offset (search_hbm_src_off once it has a region).
 * votes is read only when classify.  Returns fixed_total, the slots of all LDS-map reads. */
inline uint64_t search_assign_maps(const SearchTuning &t, bool classify, int32_t n, const int32_t *len, const unsigned long long *votes,
		uint8_t *map_log2, uint64_t *src_off) {
	uint64_t fixed_total = 0;
	for (int32_t i = 0; i < n; ++i) {
		src_off[i] = fixed_total;
		map_log2[i] = 0;
		if (!t.use_wave || len[i] + 1 > kSearchWaveSeq) continue;
		const int l = t.forced_log2 ? t.forced_log2 : classify ? search_wave_log2(votes[i]) : kSearchWaveLog2Default;
		map_log2[i] = (uint8_t) l;
		uint64_t bins = (uint64_t) search_wave_entries(l);
		if (classify && votes[i] < bins) bins = votes[i];
		fixed_total += 2 * bins;
	}
	return fixed_total;
}

/* ------------------------------------------------------------------ the retry ladder */

/* The reference's ladder (CS.cpp:345-394): the current table size with a probe budget of a third of the table, then that + 2, + 3,
 * ... up to 2^20 entries with 0.777; first_bits = CS::c_SrchTableBitLen (0: 16, what a thread starts with; the reference adapts
 * it per batch, CS.cpp:482-489 -- the size only decides WHEN an attempt runs out of budget, a successful attempt returns the same
 * list at every size).  The ladder ends with the first attempt whose bits exceed kSearchLadderMaxBits. */
static const int kSearchLadderMaxBits = 20;
inline int search_ladder_bits(int first_bits, int attempt) {
	const int bits0 = first_bits ? first_bits : 16;
	return attempt == 0 ? bits0 : bits0 + 1 + attempt;
}
inline float search_ladder_factor(int attempt) { return attempt == 0 ? 0.333f : 0.777f; }

/* ------------------------------------------------------------------ one attempt's LDS launches */

static const int kSearchWaveSizes = kSearchWaveLog2Max - kSearchWaveLog2Min + 1;
struct SearchWaveLaunch {
	int log2;                /* the map size of this launch's reads */
	size_t first, count;     /* its part of the work list */
	int longest;             /* its longest read, without the NUL */
	int seq_cap;             /* bytes of LDS for the read: launch_search_wave's seq_cap */
	bool slot8;              /* the 8-byte map */
};
/* One launch per map size: `work` gets the reads of work_wave grouped by ascending map size, read order kept inside a group, and
 * out one record per size that has reads.  The 8-byte map where it applies: the reference's default table size or below, not the
 * largest map, and sub-reads (a count of 255 is out of reach of a read's 256 k-mers unless a row repeats inside a bin) -- the last
 * of which CVX_TUNE_SEARCH_SLOT8 = 1 drops; = 0: never.  Returns the number of launches. */
inline int search_wave_launches(const SearchTuning &t, int bits, const std::vector<int32_t> &work_wave, const uint8_t *map_log2,
		const int32_t *len, int32_t *work, SearchWaveLaunch out[kSearchWaveSizes]) {
	int n_out = 0;
	size_t at = 0;
	for (int l = kSearchWaveLog2Min; l <= kSearchWaveLog2Max; ++l) {
		const size_t first = at;
		int longest = 0;
		for (int32_t i : work_wave) if (map_log2[i] == l) { work[at++] = i; longest = std::max(longest, len[i]); }
		if (at == first) continue;
		const bool fits = bits <= 16 && l < kSearchWaveLog2Max;
		SearchWaveLaunch &w = out[n_out++];
		w.log2 = l; w.first = first; w.count = at - first; w.longest = longest;
		w.seq_cap = (longest + 65 + 63) / 64 * 64;
		w.slot8 = t.slot8 < 0 ? fits && longest <= 268 : t.slot8 != 0 && fits;
	}
	return n_out;
}

/* ------------------------------------------------------------------ the table budget of the HBM forms */

/* The wave-per-read kernel's tables belong to the waves: as many as can be resident (or as 8 GB hold), each 2^bits entries of 16
 * bytes = two 8-byte words.  The lane-per-read kernel takes a table of 2^bits keys and twice as many scores per read of a chunk,
 * and as many reads per chunk as 8 GB of such tables hold. */
inline size_t search_table_budget(int bits) { return ((size_t) 8 << 30) / (((size_t) 1 << bits) * 16); }
inline size_t search_hbm_tables(size_t n_reads, int bits) { return std::max<size_t>(1, std::min(std::min<size_t>(n_reads, 8192), search_table_budget(bits))); }
inline size_t search_hbm_table_words(size_t n_tables, int bits) { return n_tables * ((size_t) 1 << bits) * 2; }
inline size_t search_lane_chunk(size_t n_reads, int bits) { return std::max<size_t>(1, std::min(n_reads, search_table_budget(bits))); }
inline size_t search_lane_keys(size_t n_reads, int bits) { return n_reads * ((size_t) 1 << bits); }
inline size_t search_lane_scores(size_t n_reads, int bits) { return 2 * search_lane_keys(n_reads, bits); }

/* ------------------------------------------------------------------ regions of the reads on the HBM forms */

/* Regions only for the reads that really go to an HBM form, handed out when a read first gets there and kept for its retries
 * (sizing them by the votes of all n reads cost a repeat-rich call gigabytes per handle): list_off[i] = the votes of the reads that
 * got one before it, *total grows by its own.  The rList and undo regions start there, the candidates at search_hbm_src_off.
 * true: at least one read got a region (the device's copy of list_off is stale, the arenas may be too small). */
inline bool search_give_regions(const std::vector<int32_t> &reads, const unsigned long long *votes, uint8_t *has_region, uint64_t *list_off, uint64_t *total) {
	bool grew = false;
	for (int32_t i : reads) {
		if (has_region[i]) continue;
		has_region[i] = 1;
		list_off[i] = *total;
		*total += votes[i];
		grew = true;
	}
	return grew;
}
/* the sparse region behind the slots of all LDS-map reads: two slots per vote */
inline uint64_t search_hbm_src_off(uint64_t fixed_total, uint64_t list_off) { return fixed_total + 2 * list_off; }
/* the candidate arena: what it has to hold, and what it grows to when it does not (it grows under live lists: by half the votes more) */
inline size_t search_cand_needed(uint64_t fixed_total, uint64_t total) { return (size_t) (fixed_total + 2 * total) + 64; }
inline size_t search_cand_grown(uint64_t fixed_total, uint64_t total) { return (size_t) (fixed_total + 2 * total) + (size_t) total / 2 + 64; }

/* ------------------------------------------------------------------ what comes back */

/* The dense candidate list in read order: begin[n + 1] (the last one plan_candidate_windows_kernel's end of the last list),
 * and the caller's cand_begin[n] and n_candidates[n].  A read without a list (-1; kSearchNeedsHbm cannot remain: such a read was
 * redone in its attempt) adds nothing.  Returns the candidates of the call. */
inline uint64_t search_dense_offsets(int32_t n, const int32_t *ncand, uint64_t *begin, uint64_t *cand_begin, int32_t *n_candidates) {
	uint64_t need = 0;
	for (int32_t i = 0; i < n; ++i) {
		begin[i] = need; cand_begin[i] = need; n_candidates[i] = ncand[i];
		if (ncand[i] > 0) need += (uint64_t) ncand[i];
	}
	begin[n] = need;
	return need;
}

}  // namespace cvx

#endif
