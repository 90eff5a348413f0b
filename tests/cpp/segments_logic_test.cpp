/*
 * segments_logic_test.cpp -- the host half of queries taken as segments of a read block (ngmlr_amd/csrc/cvx_segments.h and the
 * segments mode of cvx_host_logic.h's upload layout and schedule), no device and no library:
 *   validation: read index, start, length against the read, flag bits, offsets;
 *   the chunk split against a brute-force enumeration: every destination byte covered exactly once, whole pieces aligned and
 *   inside the string, ragged ends shorter than a piece;
 *   the upload schedule: which blocks travel, the read block zero-copy against staged in pieces, the pads cleared on the device.
 */
#include <cstdio>
#include <string>
#include <vector>

#include "../../ngmlr_amd/csrc/cvx_host_logic.h"
#include "../../ngmlr_amd/csrc/cvx_segments.h"

using namespace cvx;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { if (++fails < 20) printf("%s:%d: %s\n", __FILE__, __LINE__, #c); } } while (0)

static void test_validation() {
	const std::string a = std::string("ACGTACGTAC") + '\0' + "GG" + '\0' + '\0';      /* reads of 10, 2 and 0 bytes */
	const uint64_t off[] = {0, 11, 14, 15};
	auto plan = [&](cvx_read_segment s, int32_t len, int64_t *bad) {
		SegPlan pl;
		*bad = 99;
		return segments_plan(3, off, 1, &s, [&](int32_t) { return len; }, [&](int32_t) { return (uint64_t) 0; }, pl, bad);
	};
	int64_t bad;
	CHECK(segment_read_len(off, 0) == 10 && segment_read_len(off, 1) == 2 && segment_read_len(off, 2) == 0);
	CHECK(plan({0, 0, 0, 0}, 10, &bad) == CVX_OK);
	CHECK(plan({0, 3, CVX_SEG_REVCOMP, 0}, 7, &bad) == CVX_OK);
	CHECK(plan({2, 0, 0, 0}, 0, &bad) == CVX_OK);                                     /* an empty string of an empty read */
	CHECK(plan({0, 10, 0, 0}, 0, &bad) == CVX_OK);                                    /* ... at the very end of a read */
	CHECK(plan({3, 0, 0, 0}, 1, &bad) == CVX_ERR_ARG && bad == 0);                    /* read outside [0, n_reads) */
	CHECK(plan({-1, 0, 0, 0}, 1, &bad) == CVX_ERR_ARG && bad == 0);
	CHECK(plan({0, -1, 0, 0}, 1, &bad) == CVX_ERR_ARG && bad == 0);                   /* start < 0 */
	CHECK(plan({0, 4, 0, 0}, 7, &bad) == CVX_ERR_ARG && bad == 0);                    /* start + len beyond the read (its NUL is not part of it) */
	CHECK(plan({1, 0, 0, 0}, 3, &bad) == CVX_ERR_ARG && bad == 0);
	CHECK(plan({0, 0x7fffffff, 0, 0}, 0x7fffffff, &bad) == CVX_ERR_ARG);              /* no overflow in the sum */
	CHECK(plan({0, 0, 2, 0}, 1, &bad) == CVX_ERR_ARG && bad == 0);                    /* an unknown flag bit */
	CHECK(plan({0, 0, -1, 0}, 1, &bad) == CVX_ERR_ARG && bad == 0);
	CHECK(plan({0, 0, 0, 0}, -1, &bad) == CVX_ERR_ARG && bad == 0);                   /* a negative length */
	{
		const uint64_t down[] = {0, 11, 11, 15};      /* read 1 without even a NUL */
		SegPlan pl;
		cvx_read_segment s = {0, 0, 0, 0};
		CHECK(segments_plan(3, down, 1, &s, [&](int32_t) { return 1; }, [&](int32_t) { return (uint64_t) 0; }, pl, &bad) == CVX_ERR_ARG && bad == -2);
		const uint64_t back[] = {20, 11, 14, 15};
		CHECK(segments_plan(3, back, 1, &s, [&](int32_t) { return 1; }, [&](int32_t) { return (uint64_t) 0; }, pl, &bad) == CVX_ERR_ARG && bad == -1);
	}
	/* a block that does not begin at offset 0: source offsets are relative to the block */
	{
		const uint64_t off2[] = {100, 111, 114};
		cvx_read_segment s[2] = {{1, 1, 1, 0}, {0, 2, 0, 0}};
		SegPlan pl;
		CHECK(segments_plan(2, off2, 2, s, [&](int32_t i) { return i ? 8 : 1; }, [&](int32_t i) { return (uint64_t) (i ? 40 : 7); }, pl, &bad) == CVX_OK);
		CHECK(pl.read_bytes == 14 && pl.seg_bytes == 9 && pl.desc[0].src_off == 12 && pl.desc[1].src_off == 2 && pl.desc[0].dst_off == 7 && pl.desc[1].dst_off == 40);
		CHECK(pl.desc[0].flags == 1 && pl.desc[0].len == 1 && pl.chunks.size() == 2 && pl.first[1] == 1 && pl.first[2] == 2);
	}
}

/* the chunks of a string of len bytes at `phase`, enumerated: every byte of [0, len) written exactly once */
static void check_split(uint32_t phase, int32_t len) {
	std::vector<int> hits((size_t) len, 0);
	const int32_t nc = segment_chunks(phase, len);
	CHECK((len == 0) == (nc == 0));
	CHECK(nc <= 1 || nc == (segment_pieces(phase, len) + kSegChunkPieces - 1) / kSegChunkPieces);
	/* no more waves than the bytes need: a string that fits one chunk's pieces (and a head) is one chunk */
	CHECK(nc <= (len + kSegChunkPieces * kSegPiece - 1) / (kSegChunkPieces * kSegPiece) + 1);
	if (len > 0 && len <= 300) CHECK(nc == 1);
	for (int32_t c = 0; c < nc; ++c) {
		const SegChunkShape s = segment_chunk_shape(phase, len, c * kSegChunkPieces);
		CHECK(s.head_hi >= 0 && s.head_hi < kSegPiece && s.head_hi <= len && (c == 0 || s.head_hi == 0));
		CHECK(s.full_lo <= s.full_hi && s.full_hi <= len && (s.full_hi - s.full_lo) % kSegPiece == 0 && s.full_hi - s.full_lo <= kSegChunkPieces * kSegPiece);
		CHECK(s.full_lo == s.full_hi || ((phase + (uint32_t) s.full_lo) & 15u) == 0);      /* whole pieces are aligned in the arena */
		CHECK(s.tail_lo <= s.tail_hi && s.tail_hi - s.tail_lo < kSegPiece && s.tail_hi == len);
		CHECK(s.tail_lo == s.tail_hi || ((phase + (uint32_t) s.tail_lo) & 15u) == 0);
		for (int32_t k = 0; k < s.head_hi; ++k) hits[(size_t) k]++;
		for (int32_t k = s.full_lo; k < s.full_hi; ++k) hits[(size_t) k]++;
		for (int32_t k = s.tail_lo; k < s.tail_hi; ++k) hits[(size_t) k]++;
	}
	int wrong = 0;
	for (int32_t k = 0; k < len; ++k) if (hits[(size_t) k] != 1) wrong++;
	CHECK(wrong == 0);
}

static void test_split() {
	const int C = kSegChunkPieces * kSegPiece;
	static_assert(kSegLanePieces * 64 == kSegChunkPieces, "a chunk is a whole number of trips of a wave");
	for (uint32_t phase = 0; phase < 16; ++phase) {
		for (int32_t len = 0; len <= 70; ++len) check_split(phase, len);
		for (int m = 1; m <= 4; ++m)
			for (int32_t d = -18; d <= 18; ++d) check_split(phase, m * C + d);
		check_split(phase, 120000);
	}
	CHECK(segment_chunks(0, 120000) == 30 && segment_chunks(0, 300) == 1 && segment_chunks(5, 3) == 1 && segment_chunks(0, C) == 1 && segment_chunks(0, C + 1) == 2);
	CHECK(segment_chunks(1, C) == 1);      /* a head of 15, 255 whole pieces, a tail of 1: the 256th piece is the ragged one */
	CHECK(segment_chunks(1, C + 15) == 1 && segment_chunks(1, C + 16) == 2);
}

/* the strings on the host, against the rule written out */
static void test_host_strings() {
	std::string a;
	for (int v = 0; v < 256; ++v) a.push_back((char) v);
	a.push_back('\0');
	const uint64_t off[] = {0, 257};
	cvx_read_segment s[2] = {{0, 0, 0, 0}, {0, 0, CVX_SEG_REVCOMP, 0}};
	SegPlan pl;
	int64_t bad;
	CHECK(segments_plan(1, off, 2, s, [&](int32_t) { return 256; }, [&](int32_t i) { return (uint64_t) (256 * i); }, pl, &bad) == CVX_OK);
	std::vector<uint8_t> out(512, 0xEE);
	stage_segments_host(reinterpret_cast<const uint8_t *>(a.data()), pl.desc, out.data());
	int wrong = 0;
	for (int v = 0; v < 256; ++v) {
		const uint8_t c = (uint8_t) (v == 'A' ? 'T' : v == 'T' ? 'A' : v == 'C' ? 'G' : v == 'G' ? 'C' : v);
		if (out[(size_t) v] != v || out[(size_t) (256 + 255 - v)] != c) wrong++;
		if (segment_cpl(segment_cpl((uint8_t) v)) != v) wrong++;      /* an involution on all 256 values: revComp twice is the forward copy */
	}
	CHECK(wrong == 0);
}

/* upload layout + schedule in segments mode */
static void test_schedule() {
	const int n = 5;
	const int H[n] = {300, 1, 1500, 0, 777}, W[n] = {340, 9, 1600, 4, 800};
	std::vector<uint8_t> ref_block(4000, 'C');
	std::vector<cvx_tile> tiles((size_t) n);
	uint64_t r = 0;
	for (int i = 0; i < n; ++i) {
		cvx_tile &t = tiles[(size_t) i];
		memset(&t, 0, sizeof(t));
		t.qry = nullptr; t.qry_len = H[i];
		t.ref = reinterpret_cast<const char *>(ref_block.data() + r); t.ref_len = W[i]; r += (uint64_t) W[i];
		t.corridor_kind = CVX_CORRIDOR_CONST; t.corridor_width = 50; t.corridor_offset = -5;
	}
	std::vector<TileIn> tin;
	int bad = -1;
	{
		UploadLayout L;
		CHECK(upload_layout(n, tiles.data(), tin, L, &bad) == kLayoutMalformed && bad == 0);                 /* a NULL query is malformed ... */
		CHECK(upload_layout(n, tiles.data(), tin, L, &bad, true) == kLayoutMalformed);                       /* ... with windows too */
	}
	for (int windows = 0; windows < 2; ++windows)
		for (int ref_pinned = 0; ref_pinned < 2; ++ref_pinned)
			for (int reads_pinned = 0; reads_pinned < 2; ++reads_pinned)
				for (uint64_t read_bytes : {(uint64_t) 0, (uint64_t) 4001, 2 * kReadPieceBytes + 3}) {
					UploadLayout L;
					CHECK(upload_layout(n, tiles.data(), tin, L, &bad, windows != 0, true) == kLayoutOk);    /* ... except in segments mode */
					CHECK(L.segments && !L.qry_contig && L.qry_bytes == 2578 && L.ref_contig == !windows);
					/* the arena is laid out as ever: the kernel's destinations are the tiles' query offsets */
					uint64_t q = L.qry_base;
					for (int i = 0; i < n; ++i) { CHECK(tin[(size_t) i].qry_off == q); q += (uint64_t) H[i]; }
					CHECK(L.wprefix[(size_t) n] == (windows ? 0 : L.ref_bytes) + 64ull * n);                 /* no query byte is packing work */
					UploadSchedule s;
					build_upload_schedule(L, tin, n, true /* ignored: no query block exists */, ref_pinned != 0, 4, s, kPackThreadBytes, read_bytes, reads_pinned != 0);
					const bool zc_ref = !windows && ref_pinned;
					CHECK(!s.zc_qry && s.zc_ref == zc_ref);
					CHECK(s.pack_seq == !(zc_ref || windows));                                               /* off when neither block travels from the staging */
					CHECK(s.pack_work == (zc_ref || windows ? 0 : L.ref_bytes));
					/* the read block: one record from the caller's arena, or pieces of the staging; whole dwords, in order, covering it */
					CHECK(s.zc_reads == (read_bytes > 0 && reads_pinned));
					CHECK(s.zero_copy_bytes == (zc_ref ? L.ref_bytes : 0) + (s.zc_reads ? read_bytes : 0));
					uint64_t at = 0;
					for (const UploadCopy &u : s.read_copies) {
						CHECK(u.dst == kToReads && u.src == (s.zc_reads ? kFromReadBlock : kFromReadStaging));
						CHECK(u.dst_off == at && u.src_off == at && u.len > 0 && u.len % 4 == 0 && at % 256 == 0 && (s.zc_reads || u.len <= kReadPieceBytes));
						at += u.len;
					}
					CHECK(at == (read_bytes + 3) / 4 * 4 && at < read_bytes + 4);                            /* (inside what in_pinned_block was asked about / the staging's slack) */
					CHECK(s.read_threads == (!s.zc_reads && read_bytes >= kPackThreadBytes ? 4 : 1));      /* 2 x 4 MB + 3 bytes: worth the pack threads */
					CHECK(s.read_copies.size() == (read_bytes == 0 ? 0u : s.zc_reads ? 1u : (size_t) ((at + kReadPieceBytes - 1) / kReadPieceBytes)));
					/* the sequence arena: nothing is written into the query block, its two pads are cleared on the device behind the
					 * whole upload, everything else is written as without segments */
					std::vector<int> wrote(L.seq_total + 256, 0);
					for (size_t k = 0; k < s.copies.size(); ++k) {
						const UploadCopy &u = s.copies[k];
						CHECK(u.dst == kToSeq && u.src != kFromQryBlock && u.src != kFromReadBlock && u.src != kFromReadStaging);
						if (u.src == kClearOnDevice) CHECK(k >= s.n_staged);
						for (uint64_t x = 0; x < u.len; ++x) wrote[u.dst_off + x] += u.src == kClearOnDevice ? 100 : 1;
					}
					uint64_t wrong = 0;
					for (uint64_t x = 0; x < L.seq_total; ++x) {
						const bool qry = x >= L.qry_base && x < L.qry_base + L.qry_bytes;
						const bool pad_a = x < L.qry_base || (x >= L.qry_base + L.qry_bytes && x < L.ref_base);
						const bool refs = x >= L.ref_base && x < L.ref_base + L.ref_bytes;
						if (qry && wrote[x] != 0) wrong++;                     /* the kernel's alone */
						if (pad_a && wrote[x] != 100) wrong++;                 /* cleared on the device, once, and by nothing else */
						if (refs && (windows ? wrote[x] != 0 : wrote[x] < 1 || wrote[x] >= 100)) wrong++;      /* (a zero record may lie under a block's first / last unit) */
						if (!qry && !pad_a && !refs && wrote[x] == 0) wrong++; /* the last pad: staged, zeros, or cleared (windows) */
					}
					CHECK(wrong == 0);
					/* packing in this mode touches no query pointer (they are NULL) and writes no byte of block A */
					if (s.pack_seq) {
						std::vector<uint8_t> hseq(L.seq_total + 256, 0xCD), hdelta(L.delta_total + 256, 0xCD);
						upload_zero_pads(L, hseq.data());
						std::vector<RowOverflow> overflow;
						for (const UploadPiece &p : s.pieces) upload_pack_piece(s, p, tiles.data(), tin, L, hseq.data(), hdelta.data(), overflow);
						uint64_t touched = 0;
						for (uint64_t x = 0; x < L.ref_base; ++x) if (hseq[x] != 0xCD) touched++;
						CHECK(touched == 0);
						CHECK(memcmp(hseq.data() + L.ref_base, ref_block.data(), L.ref_bytes) == 0);
					}
				}
	/* an empty job: nothing travels, nothing is cleared */
	{
		UploadLayout L;
		CHECK(upload_layout(0, nullptr, tin, L, &bad, false, true) == kLayoutOk);
		UploadSchedule s;
		build_upload_schedule(L, tin, 0, false, false, 4, s, kPackThreadBytes, 100, true);
		CHECK(s.read_copies.empty() && !s.zc_reads && s.copies.size() == s.n_staged);
	}
}

int main() {
	test_validation();
	test_split();
	test_host_strings();
	test_schedule();
	if (fails) { printf("segments_logic_test: %d checks failed\n", fails); return 1; }
	printf("segments_logic_test: ok\n");
	return 0;
}
