/*
 * cvx_segments.h -- the host half of alignment queries taken as segments of a read block (cvx_submit_segments,
 * cvx_stage_segments*): a tile names its query as (read of the call's read block, start, length, flags) and
 * stage_segments_kernel (cvx_qry_stage.hip) writes the string straight into the job's sequence arena.  Restates
 * AlignmentBuffer::extractReadSeq (reference src/AlignmentBuffer.cpp:1515-1549): a forward read gets a copy of the segment, a
 * reverse read the reverse complement (computeReverseSeq, :1130-1141, over cplBase, :1117-1128), and with revComp the complement
 * is taken a second time -- cpl and the reversal are involutions, so that is the forward copy again:
 *   flags & CVX_SEG_REVCOMP clear:  query[k] = read[start + k]
 *   set:                            query[k] = cpl(read[start + len - 1 - k])
 *   extractReadSeq(len, start, isReverse, read, revComp)  ->  flags = (isReverse != revComp)
 * Here: validation, the read lengths, how a destination string is cut into chunks of 16-byte-aligned pieces (closed form; the
 * kernel evaluates the same function), and the strings built on the host.
 * Header-only and free of HIP -- it compiles with a plain C++ compiler -- so that the CPU suite can exercise it
 * (tests/cpp/segments_logic_test.cpp).
 */
#ifndef CVX_SEGMENTS_H
#define CVX_SEGMENTS_H

#include <cstdint>
#include <cstring>
#include <vector>

#include "cvx_align.h"

/* segment_chunk_shape is the one statement of the work split: stage_segments_kernel calls it on the device.  A plain C++
 * compiler sees no qualifier. */
#ifndef CVX_HOST_DEVICE
#if defined(__HIPCC__)
#define CVX_HOST_DEVICE __host__ __device__
#else
#define CVX_HOST_DEVICE
#endif
#endif

namespace cvx {

/* A destination string is written in 16-byte pieces that are ALIGNED in the arena (one dwordx4 store each); a chunk is
 * kSegChunkPieces of them -- 4 KB, four trips of a wave -- and one wave's work.  A 120 kb read is 30 chunks on 30 waves, a
 * 300-base read one. */
enum { kSegPiece = 16, kSegChunkPieces = 256, kSegLanePieces = kSegChunkPieces / 64 };

inline uint8_t segment_cpl(uint8_t c) {      /* cplBase, src/AlignmentBuffer.cpp:1117-1128: every other byte stays */
	return c == 'A' ? 'T' : c == 'T' ? 'A' : c == 'C' ? 'G' : c == 'G' ? 'C' : c;
}

/* one string of a call, as stage_segments_kernel reads it */
struct SegDesc {
	uint64_t src_off;      /* the segment's first byte (read[start]) in the uploaded read block */
	uint64_t dst_off;      /* the string's first byte in the destination arena; the kernel writes [dst_off, dst_off + len) and nothing else */
	int32_t len;
	int32_t flags;         /* CVX_SEG_REVCOMP */
};
static_assert(sizeof(SegDesc) == 24, "SegDesc layout");

/* one wave's work: the pieces [piece0, piece0 + kSegChunkPieces) of string seg (and its ragged head / tail, where they fall
 * into this chunk) */
struct SegChunk {
	int32_t seg;
	int32_t piece0;
};
static_assert(sizeof(SegChunk) == 8, "SegChunk layout");

/* bytes in front of the first aligned piece of a string of len bytes whose first byte lies at an address = phase (mod 16) */
CVX_HOST_DEVICE inline int32_t segment_head(uint32_t phase, int32_t len) {
	const int32_t h = (int32_t) ((16u - (phase & 15u)) & 15u);
	return h > len ? len : h;
}
/* aligned pieces the string touches behind its head, the last one possibly ragged */
CVX_HOST_DEVICE inline int32_t segment_pieces(uint32_t phase, int32_t len) {
	return (len - segment_head(phase, len) + kSegPiece - 1) / kSegPiece;
}
/* chunks of the string: none for an empty one, one for a string that is all head */
CVX_HOST_DEVICE inline int32_t segment_chunks(uint32_t phase, int32_t len) {
	if (len <= 0) return 0;
	const int32_t c = (segment_pieces(phase, len) + kSegChunkPieces - 1) / kSegChunkPieces;
	return c > 0 ? c : 1;
}

/* What the chunk that begins at piece0 writes, as byte ranges of the string: whole pieces [full_lo, full_hi) (a multiple of 16
 * bytes, every piece aligned in the arena and with all sixteen source bytes inside the segment), the ragged head [0, head_hi)
 * in the first chunk, the ragged tail [tail_lo, tail_hi) in the chunk that holds the piece it lies in.  Over the chunks of a
 * string the three kinds of range cover [0, len) exactly once. */
struct SegChunkShape {
	int32_t head_hi;               /* [0, head_hi): byte by byte (0: none) */
	int32_t full_lo, full_hi;
	int32_t tail_lo, tail_hi;      /* byte by byte (equal: none) */
};
CVX_HOST_DEVICE inline SegChunkShape segment_chunk_shape(uint32_t phase, int32_t len, int32_t piece0) {
	SegChunkShape s;
	const int32_t head = segment_head(phase, len);
	const int32_t n_full = (len - head) / kSegPiece;      /* whole pieces; piece p covers [head + 16 p, head + 16 p + 16) */
	int32_t last = piece0 + kSegChunkPieces;
	if (last > n_full) last = n_full;
	if (last < piece0) last = piece0;
	s.head_hi = piece0 == 0 ? head : 0;
	s.full_lo = head + kSegPiece * piece0;
	s.full_hi = head + kSegPiece * last;
	const int32_t t0 = head + kSegPiece * n_full;
	const bool mine = t0 < len && n_full >= piece0 && n_full < piece0 + kSegChunkPieces;
	s.tail_lo = mine ? t0 : len;
	s.tail_hi = len;
	return s;
}

/* a call laid out: one descriptor per string and the flat chunk table the kernel's waves index */
struct SegPlan {
	std::vector<SegDesc> desc;
	std::vector<SegChunk> chunks;
	std::vector<uint32_t> first;       /* chunks of string i: [first[i], first[i + 1]) */
	uint64_t read_bytes = 0;           /* of the read block, offsets[n_reads] - offsets[0] */
	uint64_t seg_bytes = 0;            /* sum of the lengths */
};

/* the read block has the form cvx_search_batch_arena and cvx_score_windows use: read r is arena[offsets[r] .. offsets[r + 1] - 1),
 * its NUL at offsets[r + 1] - 1 */
inline int64_t segment_read_len(const uint64_t *offsets, int32_t r) { return (int64_t) (offsets[r + 1] - offsets[r]) - 1; }

/* CVX_OK, or CVX_ERR_ARG with *bad = the string (or, for the offsets, -1 - read) that is wrong.
 * len_of(i): the length of string i (tiles[i].qry_len); dst_of(i): its first byte in the destination arena, whose base is
 * aligned to 16 bytes or more (a device allocation) -- the offset modulo 16 is the address modulo 16. */
template <typename LenOf, typename DstOf>
inline int segments_plan(int32_t n_reads, const uint64_t *offsets, int32_t n, const cvx_read_segment *seg, LenOf len_of, DstOf dst_of,
		SegPlan &pl, int64_t *bad) {
	for (int32_t r = 0; r < n_reads; ++r)
		if (offsets[r + 1] <= offsets[r] || offsets[r + 1] - offsets[r] > 0x7fff0000ull) { *bad = -1 - (int64_t) r; return CVX_ERR_ARG; }      /* (a chunk's byte indices stay inside int32) */
	pl.read_bytes = n_reads > 0 ? offsets[n_reads] - offsets[0] : 0;
	pl.desc.resize((size_t) n);
	pl.first.assign((size_t) n + 1, 0);
	pl.chunks.clear();
	pl.seg_bytes = 0;
	for (int32_t i = 0; i < n; ++i) {
		const cvx_read_segment &s = seg[i];
		const int64_t len = (int64_t) len_of(i);
		if (s.read < 0 || s.read >= n_reads || s.start < 0 || len < 0 || (s.flags & ~(int32_t) CVX_SEG_REVCOMP) != 0 ||
				(int64_t) s.start + len > segment_read_len(offsets, s.read)) { *bad = i; return CVX_ERR_ARG; }
		SegDesc &d = pl.desc[(size_t) i];
		d.src_off = offsets[s.read] - offsets[0] + (uint64_t) s.start;
		d.dst_off = (uint64_t) dst_of(i);
		d.len = (int32_t) len;
		d.flags = s.flags;
		const int32_t nc = segment_chunks((uint32_t) (d.dst_off & 15u), d.len);
		for (int32_t c = 0; c < nc; ++c) pl.chunks.push_back(SegChunk{i, c * kSegChunkPieces});
		pl.first[(size_t) i + 1] = (uint32_t) pl.chunks.size();
		pl.seg_bytes += (uint64_t) len;
	}
	return CVX_OK;
}

/* The strings of a planned call built the way extractReadSeq builds them -- a copy, or computeReverseSeq's byte-at-a-time
 * reverse complement -- at their places in out.  reads: the read block (arena + offsets[0]).  Knows nothing of chunks. */
inline void stage_segments_host(const uint8_t *reads, const std::vector<SegDesc> &desc, uint8_t *out) {
	for (const SegDesc &d : desc) {
		const uint8_t *src = reads + d.src_off;
		uint8_t *q = out + d.dst_off;
		if (d.flags & CVX_SEG_REVCOMP) for (int32_t k = 0; k < d.len; ++k) q[k] = segment_cpl(src[d.len - 1 - k]);
		else if (d.len > 0) memcpy(q, src, (size_t) d.len);
	}
}

}  // namespace cvx

#endif
