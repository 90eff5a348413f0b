/*
 * cvx_score_windows.h -- the host half of scoring against the resident genome (cvx_score_windows*, cvx_stage_windows*): from
 * (position, buffer_len, read, strand) per pair to string lengths, shape classes, slot order and arena offsets, and the same
 * strings built on the host.  Restates the preparation loop of ScoreBuffer::DoRun / scoreShortRead (reference
 * src/ScoreBuffer.cpp:94-121, :245-265): _SequenceProvider::DecodeRefSequence (src/SequenceProvider.cpp:567-625) for the window,
 * MappedRead::computeReverseSeq (src/MappedRead.cpp:35-73) for the query.
 * Header-only and free of HIP -- it compiles with a plain C++ compiler -- so that the CPU suite can exercise it
 * (tests/cpp/score_windows_logic_test.cpp).
 */
#ifndef CVX_SCORE_WINDOWS_H
#define CVX_SCORE_WINDOWS_H

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "cvx_align.h"

/* score_window_shape is the one statement of the window rule: plan_candidate_windows_kernel (cvx_score_cands.hip) calls it on the
 * device.  A plain C++ compiler sees no qualifier. */
#if defined(__HIPCC__)
#define CVX_HOST_DEVICE __host__ __device__
#else
#define CVX_HOST_DEVICE
#endif

namespace cvx {

/* shape classes of cvx_score_submit, in launch order */
enum { kScDiag = 0, kScWave1, kScWave2, kScWave4, kScWave8, kScWave16, kScRows, kScClasses };

/* score_wave_rows of cvx_score_wave.h -- rows per lane score_wave_kernel uses for a shorter side of short_len characters (NUL
 * included): 1, 2, 4, 8 or 16, 0 = too long -- said again here because that header brings the HIP runtime's with it (and its
 * text is part of the build id); cvx_rt_score.cpp and the logic test hold the two against each other */
inline int score_class_wave_rows(int64_t short_len) {
	for (int k = 1; k <= 16; k *= 2)
		if (short_len <= 64 * k) return k;
	return 0;
}

inline int score_class(size_t rl, size_t ql, bool no_diag) {
	if (ql <= 512 && rl <= 2048 && !no_diag) return kScDiag;             /* cvx_score_batch's condition, per pair */
	switch (score_class_wave_rows((int64_t) std::min(rl, ql))) {
	case 1: return kScWave1;
	case 2: return kScWave2;
	case 4: return kScWave4;
	case 8: return kScWave8;
	case 16: return kScWave16;
	default: return kScRows;
	}
}

/* GetConcatRefLen() (src/SequenceProvider.cpp:638-640): binRefIndex - 1, binRefIndex being the genome's nibble count (:386) */
inline uint64_t score_windows_concat_len(uint64_t n_nibbles) { return n_nibbles - 1; }

/* what DecodeRefSequence(buf, 0, position, buffer_len) writes, in closed form (nothing of the genome is looked at) */
struct ScoreWinShape {
	bool failed;           /* position >= L: the call returns false */
	int32_t n_plain;       /* leading characters that are the nibbles position, position + 1, ... */
	int32_t ref_chars;     /* strlen of the window: n_plain, the 'x' of an odd len, the `end` 'x' behind the genome */
};
CVX_HOST_DEVICE inline ScoreWinShape score_window_shape(uint64_t position, int32_t buffer_len, uint64_t L) {
	ScoreWinShape s = {true, 0, 0};
	if (position >= L) return s;
	uint64_t len = (uint64_t) buffer_len - 2, end = 0;                   /* (buffer_len >= 3) */
	if (len > L - position) { end = len - (L - position); len -= end; }   /* position + len > L, without the overflow */
	const uint64_t n_dec = (position & 1ull) + 2ull * ((len + 1) / 2);
	s.failed = false;
	s.n_plain = (int32_t) (n_dec - (len & 1ull));
	s.ref_chars = (int32_t) (n_dec + end);
	return s;
}

/* one slot of a call, as stage_score_windows_kernel reads it */
struct ScoreWinDesc {
	uint64_t position;     /* first nibble of the window */
	uint64_t ref_off;      /* the window's first byte in the job's sequence arena; its NUL at ref_off + ref_chars */
	uint64_t qry_off;      /* = ref_off + ref_chars + 1; the query's NUL at qry_off + read_len */
	uint64_t read_off;     /* the read's first byte in the uploaded read block */
	uint64_t scratch_off;  /* ScorePair::scratch_off */
	int32_t n_plain, ref_chars;
	int32_t read_len;
	int32_t reverse;
};
static_assert(sizeof(ScoreWinDesc) == 56, "ScoreWinDesc layout");

/* A call laid out: the pairs in slot order -- by shape class, as score_job_enqueue orders them; the pairs whose decode fails
 * behind all others, staged (an empty window) but in no class -- and the bytes each slot owns in the sequence arena. */
struct ScoreWinPlan {
	std::vector<int32_t> order;        /* slot -> the caller's index */
	std::vector<int> cls;              /* per caller's index; kScClasses = failed */
	std::vector<ScoreWinDesc> desc;    /* per slot */
	size_t first[kScClasses + 2] = {0};/* slots of class c: [first[c], first[c + 1]); failed: [first[kScClasses], n) */
	uint64_t seq_bytes = 0;            /* of the sequence arena */
	uint64_t rows = 0;                 /* ints of score_kernel's DP rows */
	size_t max_rl_rows = 0;            /* longest window (NUL included) among the pairs that use them */
	int32_t n_scored() const { return (int32_t) first[kScClasses]; }
};

/* CVX_OK, or CVX_ERR_ARG with *bad = the pair (or, for the offsets, -1 - read) that is wrong */
inline int score_windows_plan(uint64_t L, int32_t n_reads, const uint64_t *offsets, int32_t n, const cvx_score_window *pairs,
		bool no_diag, ScoreWinPlan &pl, int64_t *bad) {
	for (int32_t r = 0; r < n_reads; ++r)
		if (offsets[r + 1] <= offsets[r] || offsets[r + 1] - offsets[r] > 0x7fffffffull) { *bad = -1 - (int64_t) r; return CVX_ERR_ARG; }
	pl.order.resize((size_t) n); pl.cls.resize((size_t) n); pl.desc.resize((size_t) n);
	size_t count[kScClasses + 1] = {0};
	for (int32_t i = 0; i < n; ++i) {
		const cvx_score_window &w = pairs[i];
		if (w.buffer_len < 3 || w.read < 0 || w.read >= n_reads) { *bad = i; return CVX_ERR_ARG; }
		const ScoreWinShape s = score_window_shape(w.position, w.buffer_len, L);
		const size_t ql = (size_t) (offsets[w.read + 1] - offsets[w.read]);      /* NUL included */
		pl.cls[(size_t) i] = s.failed ? (int) kScClasses : score_class((size_t) s.ref_chars + 1, ql, no_diag);
		++count[pl.cls[(size_t) i]];
	}
	pl.first[0] = 0;
	for (int c = 0; c <= kScClasses; ++c) pl.first[c + 1] = pl.first[c] + count[c];
	size_t fill[kScClasses + 1];
	memcpy(fill, pl.first, sizeof(fill));
	for (int32_t i = 0; i < n; ++i) pl.order[fill[pl.cls[(size_t) i]]++] = i;
	uint64_t bytes = 0;
	pl.rows = 0; pl.max_rl_rows = 0;
	const uint64_t base = n_reads > 0 ? offsets[0] : 0;
	for (int32_t s = 0; s < n; ++s) {
		const cvx_score_window &w = pairs[pl.order[(size_t) s]];
		const ScoreWinShape sh = score_window_shape(w.position, w.buffer_len, L);
		ScoreWinDesc &d = pl.desc[(size_t) s];
		d.position = w.position;
		d.n_plain = sh.n_plain; d.ref_chars = sh.ref_chars;
		d.read_off = offsets[w.read] - base;
		d.read_len = (int32_t) (offsets[w.read + 1] - offsets[w.read] - 1);
		d.reverse = w.reverse != 0;
		d.ref_off = bytes; bytes += (uint64_t) d.ref_chars + 1;
		d.qry_off = bytes; bytes += (uint64_t) d.read_len + 1;
		d.scratch_off = 0;
		const size_t rl = (size_t) d.ref_chars + 1, ql = (size_t) d.read_len + 1;
		if ((size_t) s >= pl.first[kScRows] && (size_t) s < pl.first[kScClasses] && rl < 100000 && ql < 100000) {    /* score_kernel's two DP rows */
			d.scratch_off = pl.rows;
			pl.rows += 2 * (uint64_t) rl;
			pl.max_rl_rows = std::max(pl.max_rl_rows, rl);
		}
	}
	pl.seq_bytes = bytes;
	return CVX_OK;
}

inline char score_window_dec4(unsigned v) {      /* dec4, src/SequenceProvider.cpp:90-104 (a valid genome holds no value above 4) */
	return v == 0u ? 'A' : v == 1u ? 'T' : v == 2u ? 'G' : v == 3u ? 'C' : v == 4u ? 'N' : '?';
}
inline uint8_t score_window_cpl(uint8_t c) {     /* cpl, src/MappedRead.cpp:35-46 */
	return c == 'A' ? 'T' : c == 'T' ? 'A' : c == 'C' ? 'G' : c == 'G' ? 'C' : c;
}

/* DecodeRefSequence(sequence, 0, position, buffer_len), statement by statement (src/SequenceProvider.cpp:567-625); buf gets
 * buffer_len + 1 bytes, the last one the NUL both call sites have behind the buffer.  Knows nothing of score_window_shape. */
inline bool score_window_decode_host(const uint8_t *bin_ref, uint64_t L, uint64_t position, int32_t buffer_len, std::vector<uint8_t> &buf) {
	buf.assign((size_t) buffer_len + 1, 0);
	uint64_t len = (uint64_t) buffer_len - 2;
	if (position >= L) return false;
	uint64_t end = 0;
	if (len > L - position) {      /* (position + len) > GetConcatRefLen() */
		end = len - (L - position);
		len -= end;
	}
	const uint64_t start = (position + 1) / 2;
	size_t at = 0;
	if (position & 1ull) buf[at++] = (uint8_t) score_window_dec4(bin_ref[start - 1] & 0xFu);
	for (uint64_t i = 0; i < (len + 1) / 2; ++i) {
		buf[at++] = (uint8_t) score_window_dec4(bin_ref[start + i] >> 4);
		buf[at++] = (uint8_t) score_window_dec4(bin_ref[start + i] & 0xFu);
	}
	if (len & 1ull) buf[at - 1] = 'x';
	for (uint64_t i = 0; i < end; ++i) buf[at++] = 'x';
	return true;
}

/* The strings of a planned call, each built the way its reference function builds it and then copied to the slot's place in
 * seq (pl.seq_bytes bytes).  false: a string is not as long as the plan says (the closed form and the restatement disagree). */
inline bool score_windows_stage_host(const uint8_t *bin_ref, uint64_t L, const cvx_score_window *pairs, const ScoreWinPlan &pl,
		const uint8_t *reads, uint8_t *seq) {
	std::vector<uint8_t> buf;
	for (size_t s = 0; s < pl.desc.size(); ++s) {
		const ScoreWinDesc &d = pl.desc[s];
		const cvx_score_window &w = pairs[pl.order[s]];
		const bool ok = score_window_decode_host(bin_ref, L, w.position, w.buffer_len, buf);
		const size_t got = ok ? strlen((const char *) buf.data()) : 0;
		if (got != (size_t) d.ref_chars || ok != (pl.cls[(size_t) pl.order[s]] != kScClasses)) return false;
		memcpy(seq + d.ref_off, buf.data(), got);
		seq[d.ref_off + got] = 0;
		uint8_t *q = seq + d.qry_off;
		const uint8_t *rd = reads + d.read_off;
		if (w.reverse) for (int32_t k = 0; k < d.read_len; ++k) q[k] = score_window_cpl(rd[d.read_len - 1 - k]);      /* computeReverseSeq */
		else memcpy(q, rd, (size_t) d.read_len);
		q[d.read_len] = 0;
	}
	return true;
}

}  // namespace cvx

#endif
