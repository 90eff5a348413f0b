// CPU test of the device-independent host logic (ngmlr_amd/csrc/cvx_host_logic.h): upload layout and
// packing (ragged, empty and strided tiles, multi-threaded == single-threaded), kernel-class choice,
// arena offsets and the LPT work lists, and the compute stage's launch schedule (list contents, launch order, stream slots,
// residency cap of chained classes, lanes of the backtrack walks), and the upload stage's copy schedule (executed with memcpy in
// place of the device: final arena contents, 256-byte grid, pads, order, the parent's sequences of transfers).  Built with plain g++ by tests/test_host_logic_cpu.py.
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>

#include "cvx_host_logic.h"

using namespace cvx;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

struct CorridorLine16 { int32_t offset, length; uint64_t offsetInMatrix; };   // the reference's 16-byte row

// ---------------------------------------------------------------- the upload schedule, executed with memcpy in place of the device

// a batch as a caller with two arenas hands it over: reads and references back to back in tile order, some non-zero bytes
// behind either block (what a copy rounded up to dwords picks up), one (offset, length) array pair per tile
enum { kFits = 0, kClosed = 1, kWidthChange = 2, kBigStep = 3 };      // a tile's corridor: rows in the one-byte form, a closed form, two kinds of misfit
struct UpBatch {
	std::vector<uint8_t> qry_block, ref_block;
	std::vector<std::vector<int32_t>> off, len;
	std::vector<cvx_tile> tiles;
	uint64_t qry_bytes = 0, ref_bytes = 0;
};
static void make_batch(UpBatch &b, const std::vector<int> &W, const std::vector<int> &H, const std::vector<int> &kind, bool windows) {
	const int n = (int) W.size();
	for (int i = 0; i < n; ++i) { b.qry_bytes += (uint64_t) H[i]; b.ref_bytes += (uint64_t) W[i]; }
	b.qry_block.assign(b.qry_bytes + 8, 0xEE); b.ref_block.assign(b.ref_bytes + 8, 0xEE);
	for (uint64_t k = 0; k < b.qry_bytes; ++k) b.qry_block[k] = (uint8_t) (1 + k % 61);
	for (uint64_t k = 0; k < b.ref_bytes; ++k) b.ref_block[k] = (uint8_t) (70 + k % 53);
	b.off.resize(n); b.len.resize(n); b.tiles.resize(n);
	uint64_t q = 0, r = 0;
	for (int i = 0; i < n; ++i) {
		cvx_tile &t = b.tiles[i];
		memset(&t, 0, sizeof(t));
		t.qry = reinterpret_cast<const char *>(b.qry_block.data() + q); t.qry_len = H[i]; q += (uint64_t) H[i];
		t.ref = windows ? nullptr : reinterpret_cast<const char *>(b.ref_block.data() + r); t.ref_len = W[i]; r += (uint64_t) W[i];
		if (kind[i] == kClosed) { t.corridor_kind = CVX_CORRIDOR_CONST; t.corridor_width = 40 + i % 9; t.corridor_offset = -7; continue; }
		b.off[i].resize((size_t) H[i] + 1); b.len[i].resize((size_t) H[i] + 1);      // (+ 1: a pointer for H = 0 too)
		for (int y = 0; y < H[i]; ++y) {
			b.off[i][y] = y - 20 + (y * 7 + i) % 3 + (kind[i] == kBigStep && y > H[i] / 2 ? 500 : 0);
			b.len[i][y] = 50 + (kind[i] == kWidthChange && y == H[i] - 1 ? 1 : 0);
		}
		t.row_offset = b.off[i].data(); t.row_length = b.len[i].data(); t.row_stride_bytes = 4;
	}
}

struct UpCase { bool windows = false, qry_pinned = false, ref_pinned = false; int threads = 1; uint64_t thread_bytes = kPackThreadBytes; };

// executes the schedule of a case and checks it against one single-threaded packing of the whole batch; returns the schedule
static UploadSchedule run_upload(const UpBatch &b, const UpCase &c, const char *name) {
	const int before = fails;
	const int n = (int) b.tiles.size();
	const cvx_tile *tiles = n ? b.tiles.data() : nullptr;
	UploadLayout L;
	std::vector<TileIn> tin;
	int bad = -1;
	CHECK(upload_layout(n, tiles, tin, L, &bad, c.windows) == kLayoutOk);
	const std::vector<RowSrc> rsrc0 = L.rsrc;
	UploadSchedule s;
	build_upload_schedule(L, tin, n, c.qry_pinned, c.ref_pinned, c.threads, s, c.thread_bytes);

	// the flags and sizes: the expressions stage_upload has always used
	const bool zc_qry = n > 0 && L.qry_contig && L.qry_bytes > 0 && c.qry_pinned;
	const bool zc_ref = n > 0 && !c.windows && L.ref_contig && L.ref_bytes > 0 && c.ref_pinned;
	CHECK(s.zc_qry == zc_qry && s.zc_ref == zc_ref);
	CHECK(s.zero_copy_bytes == (zc_qry ? L.qry_bytes : 0) + (zc_ref ? L.ref_bytes : 0));
	CHECK(s.pack_seq == !(zc_qry && (zc_ref || c.windows)));
	CHECK(s.pack_work == L.delta_total * 9ull + (zc_qry ? 0 : L.qry_bytes) + (zc_ref || c.windows ? 0 : L.ref_bytes));
	CHECK(s.threads == (s.pack_work < c.thread_bytes ? 1 : std::max(1, c.threads)));
	CHECK(s.pieces.size() == (size_t) (s.threads > 1 ? kUploadPieces : 1));
	CHECK((s.zero_bytes != 0) == (zc_qry || zc_ref));
	// pieces: consecutive tile ranges over [0, n), consecutive record ranges between the leading records and the tail
	{
		int t = 0;
		size_t r = s.n_leading;
		for (const UploadPiece &p : s.pieces) { CHECK(p.t0 == t && p.t1 >= p.t0 && p.rec0 == r && p.rec1 >= p.rec0); t = p.t1; r = p.rec1; }
		CHECK(t == n && r == s.n_staged && s.n_staged <= s.copies.size());
	}

	// the device arenas and the job's staging: poison everywhere but where upload_zero_pads writes
	const uint64_t seq_cap = L.seq_total + 256, delta_cap = L.delta_total + 256;       // what stage_upload ensures
	std::vector<uint8_t> dseq(seq_cap, 0xCD), ddelta(delta_cap, 0xCD), hseq(seq_cap, 0xCD), hdelta(delta_cap, 0xCD), zeros(s.zero_bytes, 0);
	if (s.pack_seq) upload_zero_pads(L, hseq.data());
	const uint8_t *from[] = { hseq.data(), hdelta.data(), zeros.data(), b.qry_block.data(), b.ref_block.data() };
	const uint64_t from_cap[] = { seq_cap, delta_cap, s.zero_bytes, L.qry_bytes + 4, L.ref_bytes + 4, 0 };      // (a block: what in_pinned_block was asked about)
	std::vector<uint8_t> by_host(L.seq_total + 256, 0);      // arena bytes written by staged / zero / clear records
	auto apply = [&](size_t r0, size_t r1) {
		for (size_t r = r0; r < r1; ++r) {
			const UploadCopy &u = s.copies[r];
			std::vector<uint8_t> &dst = u.dst == kToSeq ? dseq : ddelta;
			CHECK(u.dst == kToSeq || u.dst == kToDelta);
			CHECK(u.len > 0 && u.dst_off + u.len <= dst.size());
			if (u.dst_off + u.len > dst.size()) continue;
			if (u.src == kClearOnDevice) { memset(dst.data() + u.dst_off, 0, u.len); }
			else {
				CHECK(u.src >= kFromSeqStaging && u.src <= kFromRefBlock && u.src_off + u.len <= from_cap[u.src]);
				if (u.src_off + u.len > from_cap[u.src]) continue;
				memcpy(dst.data() + u.dst_off, from[u.src] + u.src_off, u.len);
			}
			const bool block = u.src == kFromQryBlock || u.src == kFromRefBlock;
			if (block) {
				const uint64_t bytes = u.src == kFromQryBlock ? L.qry_bytes : L.ref_bytes;
				CHECK(u.dst == kToSeq && u.src_off == 0 && u.dst_off == (u.src == kFromQryBlock ? L.qry_base : L.ref_base));
				CHECK(u.dst_off % 256 == 0 && u.len % 4 == 0 && u.len >= bytes && u.len < bytes + 4);
			} else if (u.src == kClearOnDevice) {
				CHECK(c.windows && u.dst == kToSeq && r >= s.n_staged);
			} else {
				CHECK(u.dst_off % 256 == 0 && u.len % 256 == 0);
				CHECK((u.src == kFromDeltaStaging) == (u.dst == kToDelta));
				if (u.src != kFromZeros) CHECK(u.src_off == u.dst_off && r >= s.n_leading && r < s.n_staged);
				else CHECK(r < s.n_leading);
			}
			if (!block && u.dst == kToSeq) for (uint64_t k = 0; k < u.len; ++k) by_host[u.dst_off + k] = 1;
		}
	};
	apply(0, s.n_leading);
	std::vector<RowOverflow> overflow;
	for (const UploadPiece &p : s.pieces) {
		upload_pack_piece(s, p, tiles, tin, L, hseq.data(), hdelta.data(), overflow);      // this piece only: a record that runs ahead copies poison
		apply(p.rec0, p.rec1);
	}
	apply(s.n_staged, s.copies.size());

	// the reference: pads + one single-threaded packing of everything
	std::vector<uint8_t> rseq(seq_cap, 0xCD), rdelta(delta_cap, 0xCD);
	std::vector<RowSrc> rs = rsrc0;
	RowOverflow ro;
	upload_zero_pads(L, rseq.data());
	if (c.windows && n) memset(rseq.data() + L.ref_base + L.ref_bytes, 0, L.seq_total - L.ref_base - L.ref_bytes);      // (cleared on the device)
	upload_pack(0, n, tiles, tin, rseq.data(), rdelta.data(), rs, ro, true, !c.windows);
	uint64_t seq_diff = 0;
	for (uint64_t x = 0; x < L.seq_total; ++x) {
		if (dseq[x] == rseq[x]) continue;
		if (c.windows && x >= L.ref_base && x < L.ref_base + L.ref_bytes) continue;            // the device decodes these
		if (zc_qry && x >= L.qry_base + L.qry_bytes && x < L.qry_base + (L.qry_bytes + 3) / 4 * 4) continue;      // the dword spill
		if (zc_ref && x >= L.ref_base + L.ref_bytes && x < L.ref_base + (L.ref_bytes + 3) / 4 * 4) continue;
		seq_diff++;
	}
	CHECK(seq_diff == 0);
	CHECK(L.delta_total == 0 || memcmp(ddelta.data(), rdelta.data(), L.delta_total) == 0);
	// every pad byte comes from a staged, zero or clear record
	uint64_t pad_missed = 0;
	for (uint64_t x = 0; x < L.seq_total; ++x) {
		// (an empty batch of windows has nobody to clear its last pad, and nothing that reads it)
		const bool in_pad = x < L.qry_base || (x >= L.qry_base + L.qry_bytes && x < L.ref_base) || (x >= L.ref_base + L.ref_bytes && !(c.windows && n == 0));
		if (in_pad && !by_host[x]) pad_missed++;
	}
	CHECK(pad_missed == 0);
	// staged records into one arena are pairwise disjoint; a zero record under a block's rounded-up copy precedes it
	for (size_t i = 0; i < s.copies.size(); ++i)
		for (size_t j = i + 1; j < s.copies.size(); ++j) {
			const UploadCopy &u = s.copies[i], &v = s.copies[j];
			if (u.dst != v.dst || u.dst_off + u.len <= v.dst_off || v.dst_off + v.len <= u.dst_off) continue;
			const bool ub = u.src == kFromQryBlock || u.src == kFromRefBlock, vb = v.src == kFromQryBlock || v.src == kFromRefBlock;
			CHECK(u.src == kFromZeros && vb && !ub);      // the only overlap there may be, in this order
		}
	// the misfits, renumbered: every tile's rows come back as the caller gave them
	std::vector<RowDesc> hx(misfit_rows(overflow) + 1);
	CHECK(misfit_rows(overflow) == ro.rows.size());
	place_misfits(overflow, tin, L.rsrc, hx.data());
	uint64_t rows_wrong = 0;
	for (int i = 0; i < n; ++i) {
		if (b.tiles[i].corridor_kind != CVX_CORRIDOR_ROWS) { CHECK(L.rsrc[i].fmt == kRowsConst); continue; }
		CHECK(L.rsrc[i].fmt == rs[i].fmt);
		const int H = b.tiles[i].qry_len;
		std::vector<RowDesc> rows((size_t) H + 1);
		expand_rows_host(L.rsrc[i], H, ddelta.data(), hx.data(), rows.data());
		for (int y = 0; y < H; ++y) if (rows[y].off != b.off[i][y] || rows[y].len != b.len[i][y]) rows_wrong++;
	}
	CHECK(rows_wrong == 0);
	if (fails != before) printf("  (upload case: %s)\n", name);
	return s;
}

// (arena, offset, length) of a schedule's records in issue order, against a recorded sequence
struct Xfer { int dst; uint64_t off, len; };
static bool same_sequence(const UploadSchedule &s, const std::vector<Xfer> &want) {
	if (s.copies.size() != want.size()) return false;
	for (size_t i = 0; i < want.size(); ++i)
		if (s.copies[i].dst != want[i].dst || s.copies[i].dst_off != want[i].off || s.copies[i].len != want[i].len) return false;
	return true;
}

// the batches of the parent comparison (sizes only: the sequences of transfers depend on nothing else)
static void parent_case_sizes(int which, std::vector<int> &W, std::vector<int> &H, std::vector<int> &kind) {
	const int n = which == 0 ? 48 : 120;
	for (int i = 0; i < n; ++i) {
		if (which == 0) { W.push_back(300 + (i * 977) % 3700); H.push_back(300 + (i * 613) % 3700); kind.push_back(i % 3 == 1 ? kClosed : i % 11 == 5 ? kBigStep : kFits); }
		else { W.push_back(7000 + (i * 977) % 2000); H.push_back(7000 + (i * 613) % 2000); kind.push_back(i % 13 == 6 ? kWidthChange : kFits); }
	}
}

static void test_upload_schedule() {
	// small batches: n = 0 and 1, empty reads / references, every input form with row arrays, closed forms and both
	for (int n : {0, 1, 2, 37}) for (int rows = 0; rows < 3; ++rows) for (int form = 0; form < 6; ++form) {
		std::vector<int> W, H, kind;
		for (int i = 0; i < n; ++i) {
			W.push_back(i % 7 == 3 ? 0 : 1 + (i * 389) % 900); H.push_back(i % 5 == 2 ? 0 : 1 + (i * 211) % 700);
			kind.push_back(rows == 0 ? (i % 6 == 4 ? kWidthChange : kFits) : rows == 1 ? kClosed : (i % 3 == 0 ? kClosed : i % 4 == 1 ? kBigStep : kFits));
		}
		UpCase c;
		c.windows = form >= 4; c.qry_pinned = form == 0 || form == 2 || form == 5; c.ref_pinned = form == 1 || form == 2;
		UpBatch b;
		make_batch(b, W, H, kind, c.windows);
		for (int threads : {1, 16}) {
			c.threads = threads;
			// one piece below the threshold, eight at it (given threads)
			UploadLayout L; std::vector<TileIn> tin; int bad = -1;
			upload_layout(n, n ? b.tiles.data() : nullptr, tin, L, &bad, c.windows);
			UploadSchedule probe;
			build_upload_schedule(L, tin, n, c.qry_pinned, c.ref_pinned, threads, probe);
			CHECK(probe.pieces.size() == 1);                                     // far below 8 MiB
			c.thread_bytes = probe.pack_work + 1;
			CHECK(run_upload(b, c, "small, one byte below the threshold").pieces.size() == 1);
			c.thread_bytes = probe.pack_work;
			CHECK(run_upload(b, c, "small, at the threshold").pieces.size() == (size_t) (threads > 1 ? kUploadPieces : 1));
		}
	}
	// thousands of tiles of a few bytes around one large tile: piece boundaries that round down into the same 256-byte unit
	// (nothing to copy for a piece) and pieces without tiles
	for (int form = 0; form < 6; ++form) {
		std::vector<int> W, H, kind;
		for (int i = 0; i < 3000; ++i) { W.push_back(i % 4); H.push_back((i * 3) % 5); kind.push_back(i % 7 == 1 ? kClosed : i % 50 == 9 ? kWidthChange : kFits); }
		W[1200] = 30000; H[1200] = 30000; kind[1200] = kFits;
		UpCase c;
		c.windows = form >= 4; c.qry_pinned = form == 0 || form == 2 || form == 5; c.ref_pinned = form == 1 || form == 2;
		c.threads = 16; c.thread_bytes = 1;
		UpBatch b;
		make_batch(b, W, H, kind, c.windows);
		const UploadSchedule s = run_upload(b, c, "tiny tiles");
		int empty_pieces = 0, silent_pieces = 0;
		for (const UploadPiece &p : s.pieces) { if (p.t1 == p.t0) empty_pieces++; if (p.rec1 == p.rec0) silent_pieces++; }
		CHECK(s.pieces.size() == (size_t) kUploadPieces && empty_pieces > 0 && silent_pieces > 0);
	}
	// tiles with row arrays only in the first piece, only in the last: the step stream's cut-off when no later tile has steps
	for (int where = 0; where < 2; ++where) {
		std::vector<int> W(64, 500), H(64, 500), kind(64, kClosed);
		for (int k = 0; k < 2; ++k) { const int i = where ? 62 + k : k; W[i] = H[i] = 200; kind[i] = kFits; }
		UpCase c;
		c.threads = 16; c.thread_bytes = 1;
		UpBatch b;
		make_batch(b, W, H, kind, false);
		const UploadSchedule s = run_upload(b, c, where ? "row arrays in the last piece" : "row arrays in the first piece");
		CHECK(s.pieces.size() == (size_t) kUploadPieces);
		if (s.pieces.size() == (size_t) kUploadPieces) CHECK(where ? s.pieces.back().t0 <= 62 && s.pieces[6].t0 <= s.pieces[6].t1 && s.pieces.back().t0 > 2 : s.pieces[0].t1 >= 2);
		// 400 bytes of steps.  In the first piece: their whole 256-byte units travel with it, the rest with the last piece; in the
		// last piece: nothing travels before it (the cut-off of every earlier piece is the first step of tile 62)
		int delta_copies = 0;
		for (size_t k = 0; k < s.pieces.size(); ++k)
			for (size_t r = s.pieces[k].rec0; r < s.pieces[k].rec1; ++r) {
				if (s.copies[r].dst != kToDelta) continue;
				delta_copies++;
				CHECK(k == s.pieces.size() - 1 || (!where && k == 0 && s.copies[r].len == 256));
			}
		CHECK(delta_copies == (where ? 1 : 2));
	}
	// misfits spread over many packing ranges of every piece
	{
		std::vector<int> W, H, kind;
		for (int i = 0; i < 640; ++i) { W.push_back(50 + (i * 31) % 200); H.push_back(40 + (i * 17) % 150); kind.push_back(i % 5 == 2 ? kBigStep : i % 9 == 4 ? kWidthChange : i % 8 == 7 ? kClosed : kFits); }
		for (int form : {3, 0, 5}) {
			UpCase c;
			c.windows = form >= 4; c.qry_pinned = form == 0 || form == 5;
			c.threads = 16; c.thread_bytes = 1;
			UpBatch b;
			make_batch(b, W, H, kind, c.windows);
			CHECK(run_upload(b, c, "misfits").pieces.size() == (size_t) kUploadPieces);
		}
	}
	// the parent's sequences of transfers for three batches (its inline expressions, evaluated on the same layouts:
	// profiles/r10_upload_schedule.txt): one piece; eight pieces with row arrays; eight pieces with the reads pinned
	{
		static const std::vector<Xfer> want[3] = {
			{ {0, 0, 134400}, {0, 134400, 111104}, {1, 0, 82176} },
			{ {0, 0, 149760}, {0, 1003520, 131072}, {1, 0, 127488}, {0, 149760, 113152}, {0, 1134592, 111872}, {1, 127488, 113152},
			  {0, 262912, 119040}, {0, 1246464, 115200}, {1, 240640, 119296}, {0, 381952, 126976}, {0, 1361664, 132608}, {1, 359936, 126720},
			  {0, 508928, 120320}, {0, 1494272, 119552}, {1, 486656, 120320}, {0, 629248, 120064}, {0, 1613824, 117504}, {1, 606976, 120320},
			  {0, 749312, 112896}, {0, 1731328, 115456}, {1, 727296, 112640}, {0, 862208, 141312}, {0, 1846784, 141056}, {1, 839936, 119296} },
			{ {0, 0, 22272}, {0, 980992, 22528}, {0, 22272, 958820}, {0, 1003520, 131072}, {1, 0, 127488}, {0, 1134592, 111872},
			  {1, 127488, 113152}, {0, 1246464, 115200}, {1, 240640, 119296}, {0, 1361664, 132608}, {1, 359936, 126720}, {0, 1494272, 119552},
			  {1, 486656, 120320}, {0, 1613824, 117504}, {1, 606976, 120320}, {0, 1731328, 115456}, {1, 727296, 112640}, {0, 1846784, 141056},
			  {1, 839936, 119296} },
		};
		for (int which = 0; which < 3; ++which) {
			std::vector<int> W, H, kind;
			parent_case_sizes(which, W, H, kind);
			UpCase c;
			c.threads = 16; c.qry_pinned = which == 2;
			UpBatch b;
			make_batch(b, W, H, kind, false);
			const UploadSchedule s = run_upload(b, c, "parent comparison");
			CHECK(s.pieces.size() == (size_t) (which == 0 ? 1 : kUploadPieces));
			CHECK(same_sequence(s, want[which]));
		}
	}
}

int main() {
	std::mt19937 rng(7);
	// ---------------------------------------------------------------- layout + packing
	const int n = 200;
	std::vector<std::string> refs(n), qrys(n);
	std::vector<std::vector<int32_t>> off(n), len(n);
	std::vector<std::vector<CorridorLine16>> lines(n);
	std::vector<cvx_tile> tiles(n);
	uint64_t n_closed_rows = 0;
	for (int i = 0; i < n; ++i) {
		const int W = (i % 17 == 0) ? 0 : (int) (rng() % 5000);
		const int H = (i % 13 == 0) ? 0 : (int) (rng() % 4000);
		refs[i].resize(W); qrys[i].resize(H);
		for (auto &c : refs[i]) c = "ACGTN"[rng() % 5];
		for (auto &c : qrys[i]) c = "ACGT"[rng() % 4];
		off[i].resize(H); len[i].resize(H); lines[i].resize(H);
		for (int y = 0; y < H; ++y) {
			// (one tile has offsets next to INT32_MIN / INT32_MAX: the 32-bit difference of the vector path would wrap)
			// two thirds of the tiles look like the reference's corridors (one width, offsets creeping along);
			// the others change width from row to row or jump by more than a byte
			off[i][y] = (int32_t) (y - 150 + (int) (rng() % 7)) + ((i % 11 == 5 && y > H / 2) ? 500 : 0) - ((i % 7 == 3) ? 2 * y : 0);
			len[i][y] = (i % 3 == 0) ? (int32_t) (300 + rng() % 70) : 340;
			if (i == 44) off[i][y] = (y & 1) ? INT32_MAX - y : INT32_MIN + y;
			lines[i][y] = {off[i][y], len[i][y], 0xdeadbeefull};
		}
		cvx_tile &t = tiles[i];
		memset(&t, 0, sizeof(t));
		t.ref = refs[i].data(); t.qry = qrys[i].data();
		t.ref_len = W; t.qry_len = H;
		if (i % 9 == 4 || i % 10 == 7) {
			// closed-form corridor: no row arrays; the rows the device would generate replace off / len for the checks below
			n_closed_rows += (uint64_t) H;
			t.corridor_width = 309 + i % 60;
			if (i % 9 == 4) {
				t.corridor_kind = CVX_CORRIDOR_AFFINE;
				t.corridor_k = (float) std::max(H, 1) * 1.0f / (float) std::max(W, 1);
				t.corridor_d = (i & 2) ? (float) t.corridor_width / 2.0f : 0.0f;
				t.corridor_right = (i & 2) ? 0.0f : 156.16f + (float) (i % 5);
			} else {
				t.corridor_kind = CVX_CORRIDOR_CONST;
				t.corridor_offset = (int) (W * -0.2);
			}
			for (int y = 0; y < H; ++y) {
				off[i][y] = t.corridor_kind == CVX_CORRIDOR_CONST ? t.corridor_offset
						: (int32_t) (((float) y - t.corridor_d) / t.corridor_k - t.corridor_right);
				len[i][y] = t.corridor_width;
			}
		} else if (i & 1) {       // CorridorLine[] passed directly, stride 16
			t.row_offset = H ? &lines[i][0].offset : nullptr;
			t.row_length = H ? &lines[i][0].length : nullptr;
			t.row_stride_bytes = 16;
		} else {
			t.row_offset = off[i].data(); t.row_length = len[i].data();
			t.row_stride_bytes = 4;
		}
	}
	UploadLayout L;
	std::vector<TileIn> tin;
	int bad = -1;
	CHECK(upload_layout(n, tiles.data(), tin, L, &bad) == kLayoutOk);
	CHECK(L.pad >= (uint64_t) kRingMax + 256);
	// arena = [pad][every read][pad][every reference][pad]: two blocks in tile order
	uint64_t qo = L.qry_base, so = L.ref_base, ro = 0;
	CHECK(L.qry_base == L.pad && L.pad % 256 == 0 && L.ref_base % 256 == 0 && L.ref_base >= L.qry_base + L.qry_bytes + L.pad);
	for (int i = 0; i < n; ++i) {
		CHECK(tin[i].ref_off == so); so += tiles[i].ref_len;
		CHECK(tin[i].qry_off == qo); qo += tiles[i].qry_len;
		// only corridors that came as row arrays own a slice of the rows arena (closed forms are evaluated in registers)
		if (tiles[i].corridor_kind == CVX_CORRIDOR_ROWS) { CHECK(tin[i].row_off == ro); ro += tiles[i].qry_len; }
		else CHECK(tin[i].row_off == 0);
		CHECK(tin[i].H == tiles[i].qry_len && tin[i].W == tiles[i].ref_len);
	}
	CHECK(qo == L.qry_base + L.qry_bytes && so == L.ref_base + L.ref_bytes && so + L.pad + 64 == L.seq_total && ro == L.arena_rows);
	CHECK(L.arena_rows == L.n_rows - n_closed_rows);
	CHECK(!L.qry_contig && !L.ref_contig);                                           // every tile has its own std::string
	CHECK(L.wprefix.size() == (size_t) n + 1 && L.wprefix[0] == 0);

	CHECK(L.rsrc.size() == (size_t) n && L.delta_total >= L.n_rows - n_closed_rows);
	std::vector<uint8_t> a(L.seq_total, 0xAA), b(L.seq_total, 0x55);
	std::vector<uint8_t> da(L.delta_total + 4, 0x11), db(L.delta_total + 4, 0x22);
	std::vector<RowSrc> sa = L.rsrc, sb = L.rsrc;
	upload_zero_pads(L, a.data());
	upload_zero_pads(L, b.data());
	RowOverflow oa;
	upload_pack(0, n, tiles.data(), tin, a.data(), da.data(), sa, oa);              // one thread
	std::vector<RowOverflow> ob(8);
	std::atomic<int> oslot{0};
	parallel_ranges(n, L.wprefix, 7, [&](int bg, int en) { upload_pack(bg, en, tiles.data(), tin, b.data(), db.data(), sb, ob[oslot++]); });
	CHECK(a == b);                                                                   // every byte defined, same result
	for (uint64_t k = 0; k < L.pad; ++k) if (a[k] != 0 || a[L.seq_total - 1 - k] != 0) { CHECK(!"pads zeroed"); break; }
	// the misfits' rows get their place in the verbatim buffer (what stage_upload does after the parallel phase)
	auto place = [&](std::vector<RowOverflow> &lists, std::vector<RowSrc> &rs, std::vector<RowDesc> &rowsx) {
		rowsx.resize(misfit_rows(lists));
		place_misfits(lists, tin, rs, rowsx.data());
	};
	std::vector<RowDesc> xa, xb;
	std::vector<RowOverflow> la(1, oa);
	place(la, sa, xa);
	place(ob, sb, xb);
	int n_explicit = 0, n_delta = 0, n_closed = 0;
	for (int i = 0; i < n; ++i) {
		CHECK(memcmp(a.data() + tin[i].ref_off, refs[i].data(), refs[i].size()) == 0);
		CHECK(memcmp(a.data() + tin[i].qry_off, qrys[i].data(), qrys[i].size()) == 0);
		CHECK(sa[i].fmt == sb[i].fmt);
		if (tiles[i].corridor_kind != CVX_CORRIDOR_ROWS) { CHECK(sa[i].fmt == (tiles[i].corridor_kind == CVX_CORRIDOR_AFFINE ? kRowsAffine : kRowsConst)); n_closed++; }
		else (sa[i].fmt == kRowsExplicit ? n_explicit : n_delta) += 1;
		const int H = tiles[i].qry_len;
		std::vector<RowDesc> ra((size_t) H + 1), rb((size_t) H + 1);
		expand_rows_host(sa[i], H, da.data(), xa.data(), ra.data());                 // = expand_rows_kernel
		expand_rows_host(sb[i], H, db.data(), xb.data(), rb.data());
		for (int y = 0; y < H; ++y) {
			if (ra[y].off != off[i][y] || ra[y].len != len[i][y] || rb[y].off != off[i][y] || rb[y].len != len[i][y]) { CHECK(!"rows survive the one-byte form"); break; }
		}
	}
	CHECK(n_delta > 0 && n_explicit > 0 && n_closed > 10);                           // every form exercised
	// ranges handed to the threads tile [0, n) exactly once
	{
		std::vector<int> seen(n, 0);
		std::vector<std::pair<int, int>> got(64, {-1, -1});
		std::atomic<int> slot{0};
		parallel_ranges(n, L.wprefix, 16, [&](int bg, int en) { got[slot++] = {bg, en}; });
		for (auto &g : got) if (g.first >= 0) for (int i = g.first; i < g.second; ++i) seen[i]++;
		for (int i = 0; i < n; ++i) if (seen[i] != 1) { CHECK(!"range cover"); break; }
	}
	// malformed input is refused with the index of the offender
	{
		std::vector<cvx_tile> t2(tiles.begin(), tiles.begin() + 5);
		t2[3].row_stride_bytes = 6;
		CHECK(upload_layout(5, t2.data(), tin, L, &bad) == kLayoutMalformed && bad == 3);
		t2[3].row_stride_bytes = 4; t2[2].qry_len = 10; t2[2].row_offset = nullptr;
		CHECK(upload_layout(5, t2.data(), tin, L, &bad) == kLayoutMalformed && bad == 2);
		CHECK(upload_layout(0, nullptr, tin, L, &bad) == kLayoutOk && L.n_rows == 0 && L.seq_total == L.ref_base + L.pad + 64);
		// a malformed closed form, and sequences that do lie back to back (one arena, tile order)
		std::vector<cvx_tile> t3(tiles.begin(), tiles.begin() + 3);
		t3[1].corridor_kind = CVX_CORRIDOR_AFFINE; t3[1].corridor_k = 0.0f; t3[1].corridor_width = 300;
		CHECK(upload_layout(3, t3.data(), tin, L, &bad) == kLayoutMalformed && bad == 1);
		// ... and forms whose (float -> int) row offset would leave the int32 range or is not finite: refused, never
		// evaluated (undefined on the host, saturating on the device)
		t3[1].corridor_k = 1.0f; t3[1].corridor_d = 0.0f; t3[1].corridor_right = 1.0f;
		CHECK(upload_layout(3, t3.data(), tin, L, &bad) == kLayoutOk);
		t3[1].corridor_right = 3.0e9f;
		CHECK(upload_layout(3, t3.data(), tin, L, &bad) == kLayoutMalformed && bad == 1);
		t3[1].corridor_right = 0.0f; t3[1].corridor_d = std::numeric_limits<float>::infinity();
		CHECK(upload_layout(3, t3.data(), tin, L, &bad) == kLayoutMalformed && bad == 1);
		t3[1].corridor_d = 0.0f; t3[1].corridor_k = 1.0e-9f;       // (H - d) / k beyond 2^31 for any real tile height
		CHECK(upload_layout(3, t3.data(), tin, L, &bad) == (t3[1].qry_len >= 3 ? kLayoutMalformed : kLayoutOk));
		std::string arena_q, arena_r;
		for (int i = 0; i < 3; ++i) { arena_q += qrys[i]; arena_r += refs[i]; }
		size_t aq = 0, ar = 0;
		for (int i = 0; i < 3; ++i) { t3[i] = tiles[i]; t3[i].qry = arena_q.data() + aq; t3[i].ref = arena_r.data() + ar; aq += qrys[i].size(); ar += refs[i].size(); }
		CHECK(upload_layout(3, t3.data(), tin, L, &bad) == kLayoutOk && L.qry_contig && L.ref_contig);
		// nothing is copied for a block that travels from the caller's page-locked arena
		std::vector<uint8_t> z(L.seq_total, 0xEE), dz(L.delta_total + 4, 0);
		RowOverflow oz;
		upload_pack(0, 3, t3.data(), tin, z.data(), dz.data(), L.rsrc, oz, false, false);
		bool untouched = true;
		for (uint8_t c : z) if (c != 0xEE) untouched = false;
		CHECK(untouched);
	}
	// the pool: many callers at once, every task exactly once
	{
		std::vector<std::atomic<int>> hits(64 * 50);
		for (auto &h : hits) h = 0;
		std::vector<std::thread> callers;
		for (int c = 0; c < 8; ++c) callers.emplace_back([&, c] { for (int r = 0; r < 8; ++r) PackPool::get().run(50, [&](int i) { hits[(size_t) ((c * 8 + r) * 50 + i)]++; }); });
		for (auto &t : callers) t.join();
		bool once = true;
		for (auto &h : hits) if (h != 1) once = false;
		CHECK(once);
	}

	// ---------------------------------------------------------------- host planning
	const int m = 3000;
	std::vector<TilePlan> plan(m);
	std::vector<TileIn> pin(m);
	for (int i = 0; i < m; ++i) {
		TilePlan &p = plan[i];
		p.r0 = (int) (rng() % 50); p.rend = p.r0 + 100 + (int) (rng() % 20000);
		p.need = 1 + (int) (rng() % 5000);
		p.flags = 0;
		if (i % 97 == 0) p.flags |= kPlanEmpty;
		if (i % 89 == 0) p.flags |= kPlanTooLarge;
		if (i % 53 == 0) p.flags |= kPlanIrregular;
		if (i % 31 == 0) p.flags |= kPlanWrap16;
		p.active = (i % 7 == 0) ? 12345 : rng() % 100000000ull;     // ties on purpose
		p.cells = p.active + rng() % 1000;
		pin[i].H = 10 + (int) (rng() % 20000); pin[i].W = 10 + (int) (rng() % 20000);
	}
	HostPlan hp;
	host_plan(m, plan.data(), pin.data(), nullptr, PlanTuning(), hp);
	uint64_t dir = 0, ops = 0;
	std::vector<int> where(m, -1);
	for (size_t c = 0; c < hp.cls.size(); ++c) for (int32_t t : hp.cls[c]) { CHECK(where[t] == -1); where[t] = (int) c; }
	for (int32_t t : hp.generic) { CHECK(where[t] == -1); where[t] = 1000; }
	for (int i = 0; i < m; ++i) {
		const TilePlan &p = plan[i];
		const TileRun &r = hp.trun[i];
		if (p.flags & kPlanTooLarge) { CHECK(r.skip && hp.tout[i].status == CVX_TILE_TOO_LARGE && where[i] == -1); continue; }
		if (p.flags & kPlanEmpty) { CHECK(r.skip && hp.tout[i].status == CVX_TILE_EMPTY && where[i] == -1); continue; }
		CHECK(!r.skip && hp.tout[i].status == 0 && hp.tout[i].score == -1.0f);
		CHECK(r.dir_off == dir && r.ops_off == ops);                 // arenas are dense, in tile order
		CHECK(r.nsteps == p.rend - p.r0 && r.r0 == p.r0 && r.ops_cap == pin[i].H + pin[i].W + 8);
		dir += (uint64_t) ((r.nsteps + 31) / 32) * (uint64_t) r.ring * 2ull;
		ops += (uint64_t) r.ops_cap;
		/* (gangs of waves -- rings of 384 / 576 slots -- take float-run tiles only: an int16-run tile's widest ring is one wave's 256) */
		int widest = 0;
		for (int c = 0; c < kNumClasses; ++c) if (kClasses[c].gang == 1 || !(p.flags & kPlanWrap16)) widest = std::max(widest, kClasses[c].ring());
		if ((p.flags & kPlanIrregular) || p.need > widest) {    /* (no rows given: no chaining) */
			CHECK(where[i] == 1000 && r.mnw == 0 && r.ring % 64 == 0);
			CHECK(r.ring >= ((p.flags & kPlanIrregular) ? pin[i].H : p.need));
		} else {
			CHECK(where[i] >= 0 && where[i] < 1000);
			const KernelClass &kc = kClasses[where[i] / 2];
			CHECK(kc.ring() == r.ring && kc.ring() >= p.need && r.mnw == kc.m && r.chain_blk0 == -1);
			if (where[i] / 2 > 0) CHECK(kClasses[where[i] / 2 - 1].ring() < p.need);   // smallest class that fits
			CHECK((where[i] & 1) == ((p.flags & kPlanWrap16) ? 1 : 0));
		}
	}
	CHECK(dir == hp.dir_dwords && ops == hp.ops_ints);
	for (auto &v : hp.cls)           // LPT: most cells first, index breaks ties
		for (size_t q = 1; q < v.size(); ++q) {
			const uint64_t x = plan[v[q - 1]].active, y = plan[v[q]].active;
			if (!(x > y || (x == y && v[q - 1] < v[q]))) { CHECK(!"LPT order"); break; }
		}
	// the packed-key sort equals the comparator sort, also when it has to fall back
	{
		std::vector<int32_t> v1, v2;
		for (int i = 0; i < m; ++i) { v1.push_back(i); v2.push_back(i); }
		plan[5].active = 1ull << 50;                                      // does not fit a packed key
		lpt_sort(v1, plan.data());
		std::sort(v2.begin(), v2.end(), [&](int32_t x, int32_t y) {
			const uint64_t ax = plan[x].active, ay = plan[y].active; return ax != ay ? ax > ay : x < y; });
		CHECK(v1 == v2 && v1[0] == 5);
	}
	// tuning knobs: a floor on the ring class, forced int16-run kernels
	{ PlanTuning tn; tn.min_slots = 4; tn.force_wrap = 1; host_plan(m, plan.data(), pin.data(), nullptr, tn, hp); }
	for (size_t c = 0; c < hp.cls.size(); ++c) {
		if (!hp.cls[c].empty()) CHECK((c & 1) == 1 && kClasses[c / 2].m >= 4);
	}
	// ---------------------------------------------------------------- chained tiles (row blocks)
	{
		const int H = 3001, W = 3300, w = 2100;            // slope-1 band, ~1050 live rows: no ring holds it
		std::vector<RowDesc> rows((size_t) H + 10);
		for (int y = 0; y < H; ++y) { rows[(size_t) y + 5].off = y - w / 2; rows[(size_t) y + 5].len = w; }
		TilePlan p; memset(&p, 0, sizeof(p));
		p.r0 = 0; p.rend = (H - 1) + std::min(W, (H - 1) - w / 2 + w); p.need = 1054; p.cells = (uint64_t) H * w; p.active = p.cells;
		TileIn in; memset(&in, 0, sizeof(in));
		in.H = H; in.W = W; in.row_off = 5;
		HostPlan hc;
		host_plan(1, &p, &in, rows.data(), PlanTuning(), hc);
		CHECK(hc.n_chained == 1 && hc.generic.empty() && hc.n_fast == 0);
		const TileRun &r = hc.trun[0];
		const int cc = chain_class_for(p.need, true);
		const int N = 64 * kChainClasses[cc];
		CHECK(r.ring == N && r.chain_blk0 == 0 && r.chain_nblk == (H + N - 1) / N && r.mnw == kChainClasses[cc]);
		const std::vector<ChainTask> &tk = hc.chain_tasks[(size_t) cc * 2];
		CHECK((int) tk.size() == r.chain_nblk && (int) hc.chain_blk.size() == r.chain_nblk);
		uint64_t dir = 0, bnd = 0;
		for (int g = 0; g < (int) tk.size(); ++g) {
			const ChainTask &t = tk[(size_t) g];
			CHECK(t.tile == 0 && t.y0 == g * N && t.rows == std::min(N, H - g * N) && t.blk == g && t.prev == g - 1);
			CHECK(((t.r0 - p.r0) & 31) == 0 && t.has_next == (g + 1 < (int) tk.size() ? 1 : 0));
			// every cell of the block lies inside [r0, r0 + nsteps)
			for (int y = t.y0; y < t.y0 + t.rows; ++y) {
				const int lo = std::max(0, y - w / 2), hi = std::min(W, y - w / 2 + w);
				if (hi > lo) CHECK(lo + y >= t.r0 && hi + y <= t.r0 + t.nsteps && lo + y - t.r0 < 32 + 2 * N);
			}
			CHECK(t.dir_off == dir && hc.chain_blk[(size_t) g].dir_off * 2 == dir && hc.chain_blk[(size_t) g].tblk0 == (t.r0 - p.r0) / 32);
			dir += (uint64_t) hc.chain_blk[(size_t) g].nblk32 * N * 2;
			if (g > 0) {
				const int yb = t.y0 - 1;
				CHECK(t.bnd_lo == std::max(0, yb - w / 2) && t.bnd_len == std::min(W, yb - w / 2 + w) - t.bnd_lo && t.bnd_in_off == tk[(size_t) g - 1].bnd_out_off);
			}
			CHECK(t.bnd_out_off == bnd);
			if (t.has_next) { const int yl = t.y0 + t.rows - 1; bnd += (uint64_t) (std::min(W, yl - w / 2 + w) - std::max(0, yl - w / 2)); }
		}
		CHECK(dir == hc.dir_dwords && bnd == hc.bnd_recs);
		// two wide tiles: tasks interleave by block index, every block after the one above it
		const int nblk1 = r.chain_nblk;
		TilePlan p2[2] = {p, p}; TileIn in2[2] = {in, in};
		host_plan(2, p2, in2, rows.data(), PlanTuning(), hc);
		const std::vector<ChainTask> &t2 = hc.chain_tasks[(size_t) cc * 2];
		CHECK((int) t2.size() == 2 * nblk1);
		std::vector<int> seen(hc.chain_blk.size(), 0);
		for (const ChainTask &t : t2) { CHECK(t.prev < 0 || seen[(size_t) t.prev]); seen[(size_t) t.blk] = 1; }
		CHECK(t2[0].tile == 0 && t2[1].tile == 1 && t2[2].tile == 0 && t2[2].y0 == N);
	}
	// ---------------------------------------------------------------- a long narrow tile: chained only in a batch too small to fill the device
	{
		const int H = 21000, W = 21500, w = 340;
		std::vector<RowDesc> rows((size_t) H);
		for (int y = 0; y < H; ++y) { rows[(size_t) y].off = y - w / 2; rows[(size_t) y].len = w; }
		TilePlan p; memset(&p, 0, sizeof(p));
		p.r0 = 0; p.rend = (H - 1) + std::min(W, (H - 1) - w / 2 + w); p.need = 175; p.cells = (uint64_t) H * w; p.active = p.cells;
		TileIn in; memset(&in, 0, sizeof(in));
		in.H = H; in.W = W;
		HostPlan hl;
		host_plan(1, &p, &in, rows.data(), PlanTuning(), hl);                       // 42 000 steps >= kLongTileSteps, one tile: chained
		CHECK(p.rend - p.r0 >= kLongTileSteps && hl.n_chained == 1 && hl.n_fast == 0 && hl.trun[0].mnw == 1);
		{ PlanTuning tn; tn.long_steps = 50000; host_plan(1, &p, &in, rows.data(), tn, hl); }
		CHECK(hl.n_chained == 0 && hl.n_fast == 1 && hl.trun[0].mnw == 3);          // below the (raised) threshold: an M = 3 ring
		{ PlanTuning tn; tn.small_batch = 1; host_plan(1, &p, &in, rows.data(), tn, hl); }
		CHECK(hl.n_chained == 0 && hl.n_fast == 1);                                 // not a small batch any more: whole tiles
		{ PlanTuning tn; tn.chain_m = 2; host_plan(1, &p, &in, rows.data(), tn, hl); }
		CHECK(hl.n_chained == 1 && hl.trun[0].mnw == 2 && hl.trun[0].ring == 128);   // forced block height
		CHECK(chain_class_for(175, true) == 0 && chain_class_for(4000, false) == 0); // 64-row blocks for every batch
	}
	// ---------------------------------------------------------------- chained tiles: block starts and boundary spans at their edges
	// (the row geometries of tests/chain_cases.py's phase and clip families, written out)
	{
		const int L = 200;
		// plans one tile of rows (off[y], L) in a window of W columns and checks what holds for every chained tile; -> its tasks
		auto plan_rows = [&](const std::vector<int> &off, int W, int N, std::vector<ChainTask> &tk, HostPlan &hc, int &r0) {
			const int H = (int) off.size();
			std::vector<RowDesc> rows((size_t) H);
			std::vector<long long> lo((size_t) H), hi((size_t) H);
			long long r0min = 0x7fffffff, rend = -0x7fffffff;
			for (int y = 0; y < H; ++y) {
				rows[(size_t) y].off = off[(size_t) y]; rows[(size_t) y].len = L;
				lo[(size_t) y] = std::max(off[(size_t) y], 0);
				hi[(size_t) y] = std::max<long long>(std::min<long long>((long long) off[(size_t) y] + L, W), lo[(size_t) y]);
				r0min = std::min(r0min, lo[(size_t) y] + y); rend = std::max(rend, hi[(size_t) y] + y);      // (plan_row_common: every row, empty ones too)
			}
			TilePlan p; memset(&p, 0, sizeof(p));
			p.r0 = (int) r0min; p.rend = (int) rend; p.need = 100;
			TileIn in; memset(&in, 0, sizeof(in));
			in.H = H; in.W = W;
			TileRun r; memset(&r, 0, sizeof(r));
			hc = HostPlan();
			tk.clear();
			plan_chain_tile(0, N / 64, p, in, rows.data(), hc, r, tk);
			r0 = p.r0;
			CHECK((int) tk.size() == (H + N - 1) / N && r.chain_nblk == (int) tk.size() && r.ring == N);
			uint64_t bnd = 0;
			for (int g = 0; g < (int) tk.size(); ++g) {
				const ChainTask &t = tk[(size_t) g];
				const int y0 = g * N, y1 = std::min(H, y0 + N);
				long long first = 0x7fffffff, end = -0x7fffffff;
				for (int y = y0; y < y1; ++y) if (hi[(size_t) y] > lo[(size_t) y]) { first = std::min(first, lo[(size_t) y] + y); end = std::max(end, hi[(size_t) y] + y); }
				CHECK(t.y0 == y0 && t.rows == y1 - y0 && ((t.r0 - p.r0) & 31) == 0 && t.r0 >= p.r0);
				if (end > first) {
					// the block begins on a multiple of 32 steps, its first cell 1 ... 32 steps behind (0 ... 31 in block 0), its last cell inside
					CHECK(first - t.r0 >= (g > 0 ? 1 : 0) && first - t.r0 <= (g > 0 ? 32 : 31) && end == (long long) t.r0 + t.nsteps);
				} else {
					CHECK(t.nsteps == 0);
				}
				if (g > 0) CHECK(t.bnd_lo == lo[(size_t) y0 - 1] && t.bnd_len == hi[(size_t) y0 - 1] - lo[(size_t) y0 - 1] && t.bnd_in_off == tk[(size_t) g - 1].bnd_out_off);
				CHECK(t.bnd_out_off == bnd);
				if (t.has_next) bnd += (uint64_t) (hi[(size_t) y1 - 1] - lo[(size_t) y1 - 1]);
				if (t.nsteps == 0) CHECK(bnd == t.bnd_out_off);      // a block without cells adds no record
			}
			CHECK(bnd == hc.bnd_recs);
		};
		for (int N : {64, 128, 256}) {
			// phase: =56 D d =max(100, N + 20), the path at column 100, 0 or 1 of its row: row N's first cell 2 N + d steps behind r0
			const int tail = std::max(100, N + 20);
			bool seen[32] = {false};
			for (int d = 0; d <= 32; ++d)
				for (int col : {100, 0, 1}) {
					std::vector<int> off((size_t) (56 + tail));
					for (int y = 0; y < (int) off.size(); ++y) off[(size_t) y] = 201 + y + (y >= 56 ? d : 0) - col;
					std::vector<ChainTask> tk; HostPlan hc; int r0;
					plan_rows(off, 402 + 56 + d + tail, N, tk, hc, r0);
					const int first = off[(size_t) N] + N - r0;
					CHECK(first == 2 * N + d && tk.size() >= 2);
					const ChainTask &t = tk[1];
					CHECK((t.r0 - r0) % 32 == 0 && first - (t.r0 - r0) >= 1 && first - (t.r0 - r0) <= 32);
					if (first % 32 == 0) CHECK(t.r0 - r0 == first - 32);      // the first cell on a multiple of 32: the block begins a whole word before it
					CHECK(t.bnd_lo == off[(size_t) N - 1] && t.bnd_len == L);
					seen[first % 32] = true;
				}
			for (bool s : seen) CHECK(s);
			// clip: =(N - 4) D3 =70 I4 =(N + 56), the path at column 100, the window cut from the left or the right
			const int H = 2 * N + 126, Wfull = 2 * N + 527;
			std::vector<int> base((size_t) H);
			for (int y = 0; y < H; ++y) base[(size_t) y] = 101 + (y < N - 4 ? y : y < N + 66 ? y + 3 : y < N + 70 ? N + 68 : y - 1);
			const int last0 = (H - 1) / N * N;
			const int left[] = {base[(size_t) N - 1] + 40, base[(size_t) N - 1], base[(size_t) N], base[(size_t) N - 1] + L, base[(size_t) N - 1] + L - 1};
			const int right[] = {base[(size_t) N - 1] + L - 1, base[(size_t) last0]};
			for (int c = 0; c < 7; ++c) {
				std::vector<int> off = base;
				int W = Wfull;
				if (c < 5) { for (int &o : off) o -= left[c]; W -= left[c]; } else W = right[c - 5];
				std::vector<ChainTask> tk; HostPlan hc; int r0;
				plan_rows(off, W, N, tk, hc, r0);
				const ChainTask &t = tk[1];
				if (c == 0) CHECK(t.bnd_lo == 0 && t.bnd_len == L - 40);
				if (c == 1) CHECK(t.bnd_lo == 0 && t.bnd_len == L);
				if (c == 2) CHECK(t.bnd_lo == 0 && t.bnd_len == L - 1);
				if (c == 3) CHECK(tk[0].nsteps == 0 && t.bnd_len == 0 && tk[1].bnd_out_off == 0 && t.nsteps > 0);
				if (c == 4) CHECK(tk[0].r0 + tk[0].nsteps == N && t.bnd_lo == 0 && t.bnd_len == 1 && tk[1].bnd_out_off == 1);      // one cell, at step N - 1
				if (c == 5) CHECK(t.bnd_lo == off[(size_t) N - 1] && t.bnd_len == L - 1);
				if (c == 6) CHECK(tk.back().nsteps == 0 && tk.back().bnd_len > 0 && tk[tk.size() - 2].nsteps > 0);
			}
		}
	}
	// ---------------------------------------------------------------- the compute stage's launch schedule
	{
		struct Batch {
			std::vector<TilePlan> plan; std::vector<TileIn> tin; uint64_t n_rows = 0;
			void add(std::mt19937 &rng, int need, int H, int steps, uint32_t flags = 0) {
				TilePlan p; memset(&p, 0, sizeof(p));
				p.r0 = 0; p.rend = steps; p.need = need; p.flags = flags;
				p.active = 1000 + rng() % 5000; p.cells = p.active + rng() % 100;     // (few values: LPT ties)
				TileIn in; memset(&in, 0, sizeof(in));
				in.H = H; in.W = H + 50;
				plan.push_back(p); tin.push_back(in); n_rows += (uint64_t) H;
			}
			int n() const { return (int) plan.size(); }
		};
		struct Built { HostPlan hp; std::vector<int32_t> lists; ComputeSchedule s; };
		auto build = [](const Batch &B, const RowDesc *rows, const PlanTuning &pt, const ScheduleTuning &st, Built &o) {
			host_plan(B.n(), B.plan.data(), B.tin.data(), rows, pt, o.hp);
			o.lists.assign((size_t) 2 * B.n() + 16, -1);
			build_schedule(o.hp, B.plan.data(), B.tin.data(), B.n(), B.n_rows, 256, st, o.lists.data(), o.s);
		};
		// what the walk of `count` tiles gets under bt_group = 0, written out: 64 lanes up to 6 144 tiles, 32 up to 12 288, 16 up to 49 152, 8 beyond
		auto lanes_by_count = [](int count) { return count <= 6144 ? 64 : count <= 12288 ? 32 : count <= 49152 ? 16 : 8; };
		// the invariants of every schedule
		auto check = [&](const Batch &B, const Built &o, const ScheduleTuning &st) {
			const HostPlan &hp = o.hp;
			const ComputeSchedule &s = o.s;
			const int n = B.n();
			std::vector<int> filled(n, 0), walked(n, 0);
			static const int free_post[] = {kOnSide0, kOnPost, kOnMain, kOnSide1}, own_post[] = {kOnSide0, kOnMain, kOnSide1};
			size_t fill_at = 0, bt_at = s.bt_begin;
			int n_ring = 0, stage = 0, last_slot = -1;
			for (const FillLaunch &L : s.launches) if (L.kind == CVX_LAUNCH_WHOLE || L.kind == CVX_LAUNCH_GANG) n_ring++;
			bool first_ring = true;
			for (size_t i = 0; i < s.launches.size(); ++i) {
				const FillLaunch &L = s.launches[i];
				// order: chained classes (ascending), whole-tile classes from the widest ring down, the catch-all kernel
				const int stg = L.kind == CVX_LAUNCH_CHAINED ? 0 : L.kind == CVX_LAUNCH_CATCH_ALL ? 2 : 1;
				CHECK(stg >= stage);
				if (stg == stage && stg == 0) CHECK(L.slot > last_slot);
				if (stg == stage && stg == 1) CHECK(L.slot < last_slot);
				if (stg == stage && stg == 2) CHECK(!"one catch-all launch");
				stage = stg; last_slot = L.slot;
				CHECK(L.stream == (st.overlap_post ? own_post[i % 3] : free_post[i % 4]));
				CHECK(L.tiles != nullptr && !L.tiles->empty());
				uint64_t cells = 0;
				for (int32_t t : *L.tiles) cells += B.plan[t].cells;
				CHECK(L.info.kind == L.kind && L.info.n_tiles == (int) L.tiles->size() && L.info.cells == cells && L.info.slots_per_lane == L.m && L.info.wrap16 == L.wrap);
				if (stg == 0) {
					CHECK(L.tiles == &hp.chain_tiles[L.slot] && L.count == (int) hp.chain_tasks[L.slot].size() && L.info.waves == L.count);
					CHECK(L.m == kChainClasses[L.slot / 2] && L.wrap == (L.slot & 1) && L.prio == (st.chain_prio >= 0 ? st.chain_prio : 1));
					for (int32_t t : *L.tiles) filled[t]++;
				} else {
					// the fill lists lie back to back in front of the backtrack segments: classes from the narrowest ring up, then the catch-all list
					CHECK(L.count == (int) L.tiles->size());
					for (int q = 0; q < L.count; ++q) { const int32_t t = o.lists[L.list_off + q]; CHECK(t == (*L.tiles)[q]); filled[t]++; }
					fill_at += (size_t) L.count;
					if (stg == 1) {
						const KernelClass &kc = kClasses[L.slot / 2];
						CHECK(L.tiles == &hp.cls[L.slot] && L.m == kc.m && L.gang == kc.gang && L.wrap == (L.slot & 1) && L.info.waves == kc.gang);
						CHECK(L.kind == (kc.gang > 1 ? CVX_LAUNCH_GANG : CVX_LAUNCH_WHOLE));
						// wide_prio: the widest ring class only, and only beside another ring class; gangs have their own knob
						CHECK(L.prio == (kc.gang > 1 ? st.gang_prio : (first_ring && n_ring > 1) ? st.wide_prio : 0));
						first_ring = false;
						// the direct-exact prefix: flagged, in LPT order, and everything behind it shorter
						int reach = 0;
						for (int32_t t : *L.tiles) if (st.exact_steps > 0 && hp.trun[t].nsteps >= st.exact_steps) reach++;
						CHECK(L.n_direct == ((reach >= 1 && reach <= kExactDirectMaxTiles) ? reach : 0));
						for (int q = 0; q < L.count; ++q) {
							const int32_t t = (*L.tiles)[q];
							CHECK((hp.tout[t].pad == kPadRedo) == (q < L.n_direct));
							if (L.n_direct) CHECK((hp.trun[t].nsteps >= st.exact_steps) == (q < L.n_direct));
							if (q > 0 && q != L.n_direct) {
								const uint64_t x = B.plan[(*L.tiles)[q - 1]].active, y = B.plan[t].active;
								if (!(x > y || (x == y && (*L.tiles)[q - 1] < t))) { CHECK(!"LPT order on either side of the prefix"); break; }
							}
						}
					} else {
						CHECK(L.tiles == &hp.generic && L.m == 0 && L.info.waves == 16 && L.wrap == 1 && L.prio == 0 && L.n_direct == 0);
					}
				}
				// one backtrack segment per launch, in launch order, back to back; H >> 5 never increases, ties keep the class's order
				CHECK(L.bt_off == bt_at && L.bt_count == (int) L.tiles->size());
				std::vector<int> pos(n, -1);
				for (size_t q = 0; q < L.tiles->size(); ++q) pos[(*L.tiles)[q]] = (int) q;
				for (int q = 0; q < L.bt_count; ++q) {
					const int32_t t = o.lists[L.bt_off + q];
					if (t < 0 || t >= n || pos[t] < 0) { CHECK(!"segment holds the launch's tiles"); break; }
					walked[t]++;
					if (q > 0) {
						const int32_t u = o.lists[L.bt_off + q - 1];
						const int ku = B.tin[u].H >> 5, kt = B.tin[t].H >> 5;
						if (!(ku > kt || (ku == kt && pos[u] < pos[t]))) { CHECK(!"backtrack order"); break; }
					}
				}
				bt_at += (size_t) L.bt_count;
				if (s.per_class) CHECK(L.walk.bulk_lanes == (st.bt_group > 0 ? st.bt_group : st.bt_group < 0 ? 8 : lanes_by_count(L.bt_count)));
			}
			CHECK(fill_at == s.bt_begin && bt_at == s.n_listed && s.n_walk == (int) (s.n_listed - s.bt_begin) && s.n_listed <= (size_t) 2 * n);
			for (int i = 0; i < n; ++i) {
				const int want = hp.trun[i].skip ? 0 : 1;
				if (filled[i] != want || walked[i] != want) { CHECK(!"every computed tile once in the fill lists and once in the backtrack segments"); break; }
				if (hp.tout[i].pad == kPadRedo && hp.trun[i].nsteps < st.exact_steps) CHECK(!"only direct-exact tiles are flagged");
			}
			CHECK(s.per_class == (s.launches.size() > 1 && s.n_walk >= 4096 && !st.overlap_post && st.bt_per_class));
			if (!s.per_class) CHECK(s.walk.bulk_lanes == (st.bt_group > 0 ? st.bt_group : st.bt_group < 0 ? (s.n_walk < 4096 ? 64 : 8) : lanes_by_count(s.n_walk)));
			// the chain upload: tasks of every class, the block table, the tile lists (8-byte aligned), nothing else
			if (hp.n_chained) {
				size_t at = 0;
				for (size_t c = 0; c < hp.chain_tasks.size(); ++c) { CHECK(s.chain_task_off[c] == at); at += hp.chain_tasks[c].size() * sizeof(ChainTask); }
				CHECK(s.chain_blk_off == at); at += hp.chain_blk.size() * sizeof(ChainBlk);
				for (size_t c = 0; c < hp.chain_tiles.size(); ++c) { CHECK(s.chain_tile_off[c] == at && at % 8 == 0); at += (hp.chain_tiles[c].size() * 4 + 7) / 8 * 8; }
				CHECK(s.chain_bytes == at);
			} else CHECK(s.chain_bytes == 0);
		};
		// rows of a slope-1 band no ring holds (~1050 live rows): shared by every chained tile of the batches below
		const int cH = 3001, cw = 2100;
		std::vector<RowDesc> crow((size_t) cH);
		for (int y = 0; y < cH; ++y) { crow[(size_t) y].off = y - cw / 2; crow[(size_t) y].len = cw; }
		// a mixed batch of `count` tiles: four ring classes, int16-run tiles, irregular tiles, skipped tiles, `chained` wide tiles
		auto mixed = [&](int count, int chained, Batch &B) {
			static const int needs[] = {40, 100, 150, 150, 150, 250};
			for (int i = 0; i < count; ++i) {
				uint32_t fl = 0;
				if (i % 97 == 5) fl |= kPlanEmpty;
				if (i % 89 == 7) fl |= kPlanTooLarge;
				if (i % 53 == 9) fl |= kPlanIrregular;
				if (i % 31 == 3) fl |= kPlanWrap16;
				// (a few reads much longer than the rest; not in a small batch, which would chain them)
				const int H = (count >= kSmallBatchTiles && i % 211 == 0) ? 60000 + (int) (rng() % 30000) : 200 + (int) (rng() % 12000);
				if (i < chained) B.add(rng, 1054, cH, 2 * cH);
				else B.add(rng, needs[i % 6], H, 2 * H + 100, fl);
			}
		};
		for (const int count : {600, 4200, 6300, 12400, 49300}) {
			for (int variant = 0; variant < 4; ++variant) {
				Batch B;
				mixed(count, 5, B);
				ScheduleTuning st;
				if (variant == 1) st.overlap_post = true;
				if (variant == 2) { st.bt_group = -1; st.wide_prio = 2; st.chain_prio = 0; }
				if (variant == 3) { st.bt_per_class = false; st.bt_group = 8; st.exact_steps = 0; }
				Built o;
				build(B, crow.data(), PlanTuning(), st, o);
				check(B, o, st);
				// chained, M = 4, 3, 2, 1 in both run forms where populated, the catch-all last
				CHECK(o.hp.n_chained == 5 && !o.hp.generic.empty() && o.s.launches.size() >= 6);
				CHECK(o.s.launches.front().kind == CVX_LAUNCH_CHAINED && o.s.launches.back().kind == CVX_LAUNCH_CATCH_ALL);
				CHECK(o.s.per_class == (count >= 4200 && variant != 1 && variant != 3));
				// live = 5 tiles x (1054 / (64 + kChainChunk) + 2) = 75 blocks: 768 resident tasks, 3 per CU; beside ring classes 48 KB per CU
				CHECK(o.s.launches.front().pad_lds == 12288);
			}
		}
		// the direct-exact prefix: 1 to kExactDirectMaxTiles tiles of a class reach exact_steps
		for (const int reach : {0, 1, kExactDirectMaxTiles, kExactDirectMaxTiles + 1}) {
			Batch B;
			for (int i = 0; i < kExactDirectMaxTiles + 600; ++i) {
				const bool lng = (i * 7 % (kExactDirectMaxTiles + 600)) < reach;      // scattered through the class
				B.add(rng, 150, 3000, lng ? kExactDirectSteps + (int) (rng() % 3) : kExactDirectSteps - 1 - (int) (rng() % 100));
			}
			for (const int steps : {kExactDirectSteps, 0}) {
				ScheduleTuning st;
				st.exact_steps = steps;
				Built o;
				build(B, nullptr, PlanTuning(), st, o);
				check(B, o, st);
				CHECK(o.s.launches.size() == 1 && o.s.launches[0].count == B.n());
				CHECK(o.s.launches[0].n_direct == ((steps > 0 && reach >= 1 && reach <= kExactDirectMaxTiles) ? reach : 0));
				int flagged = 0;
				for (const TileOut &t : o.hp.tout) flagged += t.pad == kPadRedo;
				CHECK(flagged == o.s.launches[0].n_direct);
			}
		}
		// launch order, stream slots and priorities of batches of 1, 3 and 4 ring classes (M = 3; 3, 2, 1; 4, 3, 2, 1)
		for (const int classes : {1, 3, 4}) {
			for (const bool overlap : {false, true}) {
				static const int needs[] = {150, 100, 40, 250};
				Batch B;
				for (int i = 0; i < 400; ++i) B.add(rng, needs[i % classes], 1000 + (int) (rng() % 100), 2500);
				ScheduleTuning st;
				st.overlap_post = overlap;
				st.wide_prio = 2;
				Built o;
				build(B, nullptr, PlanTuning(), st, o);
				check(B, o, st);
				const std::vector<FillLaunch> &ls = o.s.launches;
				CHECK((int) ls.size() == classes);
				static const int m3[] = {3, 2, 1}, m4[] = {4, 3, 2, 1};
				static const int slots[] = {kOnSide0, kOnPost, kOnMain, kOnSide1}, slots_overlap[] = {kOnSide0, kOnMain, kOnSide1, kOnSide0};
				for (int i = 0; i < (int) ls.size() && i < classes; ++i) {
					CHECK(ls[i].m == (classes == 1 ? 3 : classes == 3 ? m3[i] : m4[i]) && ls[i].kind == CVX_LAUNCH_WHOLE);
					CHECK(ls[i].stream == (overlap ? slots_overlap[i] : slots[i]));
					CHECK(ls[i].prio == ((i == 0 && classes > 1) ? 2 : 0));
				}
				CHECK(!o.s.per_class);
			}
		}
		// a gang class is the widest ring: it takes gang_prio, and wide_prio goes to nobody
		{
			Batch B;
			for (int i = 0; i < 300; ++i) B.add(rng, (i % 3 == 0) ? 300 : (i % 3 == 1) ? 150 : 40, 1000, 2500);
			ScheduleTuning st;
			st.gang_prio = 1;
			Built o;
			build(B, nullptr, PlanTuning(), st, o);
			check(B, o, st);
			CHECK(o.s.launches.size() == 3 && o.s.launches[0].kind == CVX_LAUNCH_GANG && o.s.launches[0].gang == 2 && o.s.launches[0].prio == 1);
			CHECK(o.s.launches[1].prio == 0 && o.s.launches[2].prio == 0);
		}
		// per_class exactly when: more than one launch, n_walk >= 4096, no overlap_post, the knob not 0
		for (const int count : {4095, 4096, 4097}) {
			for (const int classes : {1, 2}) {
				Batch B;
				for (int i = 0; i < count; ++i) B.add(rng, (classes == 2 && (i & 1)) ? 100 : 150, 1000, 2500);
				for (int variant = 0; variant < 3; ++variant) {
					ScheduleTuning st;
					st.overlap_post = variant == 1;
					st.bt_per_class = variant != 2;
					Built o;
					build(B, nullptr, PlanTuning(), st, o);
					check(B, o, st);
					CHECK(o.s.n_walk == count && o.s.per_class == (classes == 2 && count >= 4096 && variant == 0));
				}
			}
		}
		// chain_pad_lds on 256 CUs.  Expected values worked out from the rule as stage_compute had it inline:
		//   resident = min(8192, max(768, live * 3 / 2 + 256)), per_cu = ceil(resident / CUs), pad = (160 KB / per_cu - 4 KB, at most 60 KB) in
		//   256-byte units, 0 from 32 tasks per CU on; beside ring classes at most (chain_lds_kb KB / per_cu - 4 KB)
		CHECK(chain_pad_lds(10, 256, 0, true) == 50432 && chain_pad_lds(10, 256, 48, false) == 50432 && chain_pad_lds(10, 256, 48, true) == 12288);        // 3 per CU
		CHECK(chain_pad_lds(400, 256, 0, true) == 36864 && chain_pad_lds(400, 256, 48, false) == 36864 && chain_pad_lds(400, 256, 48, true) == 8192);       // 4 per CU
		CHECK(chain_pad_lds(1000, 256, 0, true) == 19200 && chain_pad_lds(1000, 256, 48, false) == 19200 && chain_pad_lds(1000, 256, 48, true) == 2816);    // 7 per CU
		CHECK(chain_pad_lds(4000, 256, 0, true) == 2304 && chain_pad_lds(4000, 256, 48, false) == 2304 && chain_pad_lds(4000, 256, 48, true) == 0);         // 25 per CU: 48 KB / 25 < 4 KB
		CHECK(chain_pad_lds(6000, 256, 0, true) == 0 && chain_pad_lds(6000, 256, 48, true) == 0);                                                           // 32 per CU: no padding
		CHECK(chain_pad_lds(10, 1024, 0, true) == 61440 && chain_pad_lds(10, 1024, 48, true) == 45056);                                                     // 1 per CU: the 60 KB limit
		// ... and as the schedule applies it: chained tiles alone (no ring class beside them), and with the cap switched off
		{
			Batch B;
			mixed(5, 5, B);
			Built o;
			build(B, crow.data(), PlanTuning(), ScheduleTuning(), o);
			check(B, o, ScheduleTuning());
			CHECK(o.s.launches.size() == 1 && o.s.launches[0].pad_lds == 50432 && o.s.launches[0].prio == 1);
			Batch B2;
			mixed(300, 5, B2);
			ScheduleTuning st;
			st.chain_lds_kb = 0;
			build(B2, crow.data(), PlanTuning(), st, o);
			check(B2, o, st);
			CHECK(o.s.launches[0].kind == CVX_LAUNCH_CHAINED && o.s.launches[0].pad_lds == 50432);
		}
		// the walk plan at each threshold and one either side
		{
			const int big = 49154;
			std::vector<TileIn> tin((size_t) big);
			std::vector<int32_t> list((size_t) big);
			for (int i = 0; i < big; ++i) { memset(&tin[(size_t) i], 0, sizeof(TileIn)); tin[(size_t) i].H = 1000; list[(size_t) i] = big - 1 - i; }
			const uint64_t mean = 1000;
			// the head: three reads of more than 3 x the mean, then one of exactly 3 x
			tin[(size_t) list[0]].H = 9000; tin[(size_t) list[1]].H = 3002; tin[(size_t) list[2]].H = 3001; tin[(size_t) list[3]].H = 3000;
			struct Want { int count, lanes, n_long; };
			static const Want by_count[] = { {1, 64, 0}, {6143, 64, 0}, {6144, 64, 0}, {6145, 32, 0}, {12287, 32, 0}, {12288, 32, 0}, {12289, 16, 3},
					{49151, 16, 3}, {49152, 16, 3}, {49153, 8, 3}, {49154, 8, 3} };
			for (const Want &w : by_count) {
				const WalkPlan a = walk_plan(w.count, w.count, 0, mean, list.data(), tin.data());
				CHECK(a.bulk_lanes == w.lanes && a.n_long == w.n_long && a.long_lanes == 32);
				// forced groups: that many lanes for every tile, no 32-lane head
				const WalkPlan f8 = walk_plan(w.count, w.count, 8, mean, list.data(), tin.data()), f64 = walk_plan(w.count, w.count, 64, mean, list.data(), tin.data());
				CHECK(f8.bulk_lanes == 8 && f8.n_long == 0 && f64.bulk_lanes == 64 && f64.n_long == 0);
				// -1: by the tiles of the whole batch, 64 lanes below 4 096 and 8 (+ the head) from there on, whatever this walk's own count
				const WalkPlan small = walk_plan(w.count, 4095, -1, mean, list.data(), tin.data()), large = walk_plan(w.count, 4096, -1, mean, list.data(), tin.data());
				CHECK(small.bulk_lanes == 64 && small.n_long == 0 && large.bulk_lanes == 8 && large.n_long == std::min(3, w.count));
			}
			CHECK(walk_plan(20000, 4097, -1, mean, list.data(), tin.data()).bulk_lanes == 8);
			// the lanes follow the walk's own count, not the batch's (a class walked behind its own fill)
			CHECK(walk_plan(5000, 60000, 0, mean, list.data(), tin.data()).bulk_lanes == 64 && walk_plan(5000, 60000, 0, mean, list.data(), tin.data()).n_long == 0);
			// a head that is the whole list; a mean that makes nobody long
			CHECK(walk_plan(2, 50000, -1, mean, list.data(), tin.data()).n_long == 2);
			CHECK(walk_plan(20000, 20000, 0, 3000, list.data(), tin.data()).n_long == 0 && walk_plan(20000, 20000, 0, 2999, list.data(), tin.data()).n_long == 1);
		}
	}
	test_upload_schedule();
	printf(fails ? "host_logic_test: %d FAILED\n" : "host_logic_test: ok\n", fails);
	return fails ? 1 : 0;
}
