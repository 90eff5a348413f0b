/*
 * cvx_job_text_logic.h -- the host logic of a job that brings its CIGAR / MD strings back with its results (a
 * CVX_CREATE_JOB_TEXT handle): how large the string arena is before anybody knows the total, which tiles a write into such an
 * arena may touch, the CVX_TUNE_JOB_TEXT_CAP knob, and the external soft clips put onto a record and a CIGAR that were formatted
 * without them (cvx_text_reclip).  No HIP and no library: tests/cpp/text_reclip_test.cpp and tests/cpp/job_text_capacity_test.cpp
 * compile it alone.
 */
#ifndef CVX_JOB_TEXT_LOGIC_H
#define CVX_JOB_TEXT_LOGIC_H

#include <stdint.h>
#include <stdlib.h>

#include "cvx_align.h"

#if defined(__HIPCC__)
#define CVX_JT_HD __host__ __device__
#else
#define CVX_JT_HD
#endif

namespace cvx {

/* Bytes of text (CIGAR + NUL + MD + NUL) per read row the arena is first sized for.  Measured on the host form
 * (cvx_format_alignment over the port oracle's ops, external clips zero; tools/job_text_bytes_per_row.py) as the largest
 * (cigar_len + md_len + 2) / H of one tile: 0.643 over 48 synth.workload_pacbio tiles (9-11 kb reads, 15 % errors; 0.610 over
 * the whole set), 1.181 over 400 synth.workload_ont tiles (0.2-20 kb, 25 %; 0.933 over the whole set).  1.181 plus a quarter is
 * 1.477: a job past its arena is still right, but pays a second write and a stream wait (stage_ops). */
static const double kJobTextBytesPerRow = 1.48;
/* ... and per tile: the two NULs, both clips and the trailing MD counter at any read length, with room to spare */
static const uint64_t kJobTextBytesPerTile = 64;

/* the capacity the first write of a job runs with; tune: CVX_TUNE_JOB_TEXT_CAP in bytes (0: the rule) */
inline uint64_t job_text_first_capacity(uint64_t rows, uint64_t n_tiles, uint64_t tune) {
	if (tune) return tune;
	return (uint64_t) (kJobTextBytesPerRow * (double) rows) + 1 + kJobTextBytesPerTile * n_tiles;
}

/* CVX_TUNE_JOB_TEXT_CAP as the environment holds it: a decimal byte count; unset, empty, 0, negative or anything that is
 * not a number all the way through mean the rule */
inline uint64_t job_text_cap_knob(const char *s) {
	if (!s || !*s) return 0;
	for (const char *p = s; *p; ++p) if (*p < '0' || *p > '9') return 0;
	return (uint64_t) strtoull(s, nullptr, 10);
}

/* a tile's text [off, off + len) is written iff all of it lies below cap: the tile is the unit, not the byte */
CVX_JT_HD inline bool job_text_tile_fits(unsigned long long off, unsigned long long len, unsigned long long cap) {
	return off <= cap && len <= cap - off;
}

namespace reclip_detail {

inline int digits(unsigned v) { int n = 1; while (v >= 10u) { v /= 10u; ++n; } return n; }

/* the bounded sink of cvx_format_alignment: counts past the capacity, keeps the last byte for the NUL */
struct Sink {
	char *p;
	int cap;
	int n;
	void ch(char c) {
		if (n < cap - 1) p[n] = c;
		++n;
	}
	void num(int v) {         /* v > 0 */
		char tmp[12];
		int k = 0;
		unsigned u = (unsigned) v;
		do { tmp[k++] = (char) ('0' + u % 10u); u /= 10u; } while (u);
		while (k) ch(tmp[--k]);
	}
	void finish() {
		if (cap > 0) p[n < cap - 1 ? n : cap - 1] = '\0';
	}
};

}  // namespace reclip_detail

/* External clips enter five things of a tile's text (cvx_format.cpp): the leading and the trailing S piece, qstart, qend, ret and
 * cigar_op_count.  rec / cigar: the tile formatted with both external clips zero (cigar: all rec->cigar_len characters).
 * -> *out and cigar_out[cigar_cap] as cvx_format_alignment_ex returns them with the clips ext_qstart / ext_qend: a piece is there
 * iff its sum is above 0, the tile's own piece (there iff rec->qstart / rec->qend is) is skipped, out->cigar_len is the full
 * length whatever fits.  A record without an alignment (ret < 0) passes through with an empty string; an op count of
 * CVX_NOT_WRITTEN (the scalar twin) stays.  0 or CVX_ERR_ARG. */
inline int text_reclip(const cvx_alignment_text *rec, const char *cigar, int32_t ext_qstart, int32_t ext_qend,
		char *cigar_out, int32_t cigar_cap, cvx_alignment_text *out) {
	using namespace reclip_detail;
	if (!rec || !out || cigar_cap < 0 || (cigar_cap > 0 && !cigar_out)) return CVX_ERR_ARG;
	const cvx_alignment_text r = *rec;      /* (out may be rec) */
	Sink cg{cigar_out, cigar_cap, 0};
	if (r.ret < 0) {
		cg.finish();
		*out = r;
		return CVX_OK;
	}
	const int lead = r.qstart > 0 ? digits((unsigned) r.qstart) + 1 : 0;
	const int trail = r.qend > 0 ? digits((unsigned) r.qend) + 1 : 0;
	if (!cigar || r.cigar_len < lead + trail) return CVX_ERR_ARG;
	const int qstart = r.qstart + ext_qstart, qend = r.qend + ext_qend;
	if (qstart > 0) { cg.num(qstart); cg.ch('S'); }
	for (int i = lead; i < r.cigar_len - trail; ++i) cg.ch(cigar[i]);
	if (qend > 0) { cg.num(qend); cg.ch('S'); }
	cg.finish();
	*out = r;
	out->qstart = qstart;
	out->qend = qend;
	/* final_len: the leading clip counts where its piece is written, the trailing one always (cvx_format.cpp) */
	out->ret = r.ret - (r.qstart > 0 ? r.qstart : 0) - r.qend + (qstart > 0 ? qstart : 0) + qend;
	if (r.cigar_op_count != CVX_NOT_WRITTEN)
		out->cigar_op_count = r.cigar_op_count - (r.qstart > 0) - (r.qend > 0) + (qstart > 0) + (qend > 0);
	out->cigar_len = cg.n;
	return CVX_OK;
}

}  // namespace cvx

#endif
