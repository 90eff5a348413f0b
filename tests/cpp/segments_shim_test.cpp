/*
 * segments_shim_test.cpp -- Convex::ConvexAlignHip with queries noted as segments of reads (DeviceReads) against the same tiles
 * with host-built query strings: a launch whose tiles are all noted (cvx_submit_segments, every distinct read sent once), a
 * launch that mixes noted and plain queries (materialised on the host, and counted), and DeviceReads::Materialise.  On every
 * logical device of the process (CVX_ALIAS_DEVICES=2: two aligners).  tests/test_gpu_shim_segments.py runs it.
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "convex_align_hip.h"
#include "service_device.h"

typedef Convex::ConvexAlignHip::Tile Tile;

static uint32_t rs = 977;
static uint32_t rnd() { rs = rs * 1664525u + 1013904223u; return rs >> 8; }

static char cpl(char c) { return c == 'A' ? 'T' : c == 'T' ? 'A' : c == 'C' ? 'G' : c == 'G' ? 'C' : c; }
static std::string revcomp(std::string const & s) { std::string r; for (size_t k = s.size(); k-- > 0;) r.push_back(cpl(s[k])); return r; }

struct Case {
	std::string ref, qry;
	std::vector<CorridorLine> lines;
	int read, start, flags;
	std::vector<char> buf;      /* what extractReadSeq's caller holds under the binding: DeviceReads::BufferBytes(length) */
	Align * align;
};

static Align * new_align(int readLength) {
	Align * a = new Align();
	a->maxBufferLength = readLength * 4;
	a->maxMdBufferLength = readLength * 4;
	a->pBuffer1 = new char[a->maxBufferLength + 16];
	a->pBuffer2 = new char[a->maxMdBufferLength + 16];
	a->pBuffer1[0] = '\0'; a->pBuffer2[0] = '\0';
	a->nmPerPostionLength = (readLength + 1) * 2;
	a->nmPerPosition = new PositionNM[a->nmPerPostionLength];
	a->svType = 0;
	return a;
}

static bool same(Align const & a, Align const & b, int ra, int rb) {
	return ra == rb && memcmp(&a.Score, &b.Score, 4) == 0 && memcmp(&a.Identity, &b.Identity, 4) == 0 && a.QStart == b.QStart && a.QEnd == b.QEnd &&
			a.PositionOffset == b.PositionOffset && a.NM == b.NM && a.alignmentLength == b.alignmentLength && a.cigarOpCount == b.cigarOpCount &&
			(ra < 0 || (strcmp(a.pBuffer1, b.pBuffer1) == 0 && strcmp(a.pBuffer2, b.pBuffer2) == 0));
}

/* the staged form of AlignTiles; tiles are prepared by the caller (a note belongs to the context that prepares the tile) */
static void run(Convex::ConvexAlignHip & al, std::vector<Tile> & tiles) {
	cvx_job job = al.Submit(tiles.data(), (int) tiles.size());
	cvx_result const * res = 0;
	uint32_t const * ops = 0;
	al.Wait(job, &res, &ops);
	for (size_t i = 0; i < tiles.size(); ++i) al.Finish(tiles[i], res[i], ops);
	al.Release(job);
}

int main() {
	int nl = 0, np = 0, bad = 0;
	Convex::DeviceLayout(nl, np);
	if (nl < 1) { printf("no device\n"); return 1; }
	if (!Convex::DeviceReads::Enabled()) { printf("CVX_DEVICE_READS=0\n"); return 1; }

	/* 24 tiles over 6 reads: the query is a mutated copy of the reference, embedded in its read as it is or reverse-complemented */
	int const n = 24, perRead = 4;
	std::vector<Case> cases((size_t) n);
	std::vector<std::string> reads;
	std::string cur;
	for (int i = 0; i < n; ++i) {
		Case & c = cases[(size_t) i];
		int const W = 300 + (int) (rnd() % 1200);
		for (int k = 0; k < W; ++k) c.ref.push_back("ACGT"[rnd() % 4]);
		for (int k = 0; k < W; ++k) {
			unsigned const e = rnd() % 100;
			if (e < 4) continue;                                                          /* deletion */
			c.qry.push_back(e < 10 ? "ACGTN"[rnd() % 5] : c.ref[(size_t) k]);           /* substitution */
			if (e >= 96) c.qry.push_back("acgt"[rnd() % 4]);                              /* insertion */
		}
		int const H = (int) c.qry.size();
		c.lines.resize((size_t) H);
		for (int y = 0; y < H; ++y) { c.lines[(size_t) y].offset = (int) ((long long) y * W / H) - 45; c.lines[(size_t) y].length = 90; c.lines[(size_t) y].offsetInMatrix = 0; }
		c.flags = (int) (rnd() & 1);
		for (unsigned k = rnd() % 30; k > 0; --k) cur.push_back("ACGTN"[rnd() % 5]);
		c.read = (int) reads.size();
		c.start = (int) cur.size();
		cur += c.flags ? revcomp(c.qry) : c.qry;
		if ((i + 1) % perRead == 0) { reads.push_back(cur); cur.clear(); }
		c.buf.assign((size_t) Convex::DeviceReads::BufferBytes(H), 0);
		c.align = 0;
	}

	auto tile_of = [&](Case & c, char const * qry) {
		Tile t;
		memset(&t, 0, sizeof(t));
		t.corridor = c.lines.data(); t.corridorHeight = (int) c.lines.size();
		t.refSeq = c.ref.c_str(); t.qrySeq = qry; t.result = c.align;
		t.externalQStart = 0; t.externalQEnd = 0; t.ret = -2;
		return t;
	};
	auto note = [&](Case & c) {
		std::string const & r = reads[(size_t) c.read];
		Convex::DeviceReads::Placeholder(c.buf.data(), r.c_str(), (int) r.size(), c.start, (int) c.qry.size(), c.flags);
	};

	for (int d = 0; d < nl; ++d) {
		Convex::ConvexAlignHip al(0, 2.0f, -5.0f, -5.0f, -5.0f, -1.0f, 0.15f, Convex::PhysicalDeviceOf(d));      /* (CVX_ALIAS_DEVICES: two aligners on one device) */
		/* the expectation: host-built strings */
		std::vector<Tile> plain;
		std::vector<Align *> want;
		for (Case & c : cases) { c.align = new_align((int) c.qry.size()); want.push_back(c.align); plain.push_back(tile_of(c, c.qry.c_str())); Convex::ConvexAlignHip::Prepare(plain.back()); }
		run(al, plain);
		int valid = 0;
		for (Tile const & t : plain) { valid += t.ret >= 0; if (t.segment) { printf("a plain tile was taken for a noted one\n"); ++bad; } }
		if (valid < n / 2) { printf("device %d: only %d of %d plain tiles aligned\n", d, valid, n); ++bad; }

		long l0 = 0, t0 = 0, m0 = 0, l1 = 0, t1 = 0, m1 = 0;
		Convex::ConvexAlignHip::ReadStats(l0, t0, m0);
		/* a noted launch: every buffer is noted first and prepared afterwards -- 24 placeholders alive in this one context */
		{
			std::vector<Tile> tiles;
			for (Case & c : cases) note(c);
			for (Case & c : cases) {
				c.align = new_align((int) c.qry.size());
				tiles.push_back(tile_of(c, c.buf.data()));
				Convex::ConvexAlignHip::Prepare(tiles.back());
				if (!tiles.back().segment || tiles.back().qryLen != (int) c.qry.size()) { printf("Prepare did not recognise a noted query\n"); ++bad; }
			}
			run(al, tiles);
			for (int i = 0; i < n; ++i)
				if (!same(*want[(size_t) i], *cases[(size_t) i].align, plain[(size_t) i].ret, tiles[(size_t) i].ret)) { printf("device %d noted launch: tile %d differs\n", d, i); ++bad; }
			for (Case & c : cases) {
				char const * sq = 0;
				int rl = 0, st = 0, ln = 0, fl = 0;
				if (!Convex::DeviceReads::Lookup(c.buf.data(), sq, rl, st, ln, fl)) { printf("a noted launch wrote into the caller's buffer\n"); ++bad; break; }
			}
		}
		Convex::ConvexAlignHip::ReadStats(l1, t1, m1);
		if (l1 - l0 != 1 || t1 - t0 != n || m1 != m0) { printf("device %d: stats after the noted launch: %ld launches, %ld tiles, %ld mixed\n", d, l1 - l0, t1 - t0, m1 - m0); ++bad; }
		/* a mixed launch: every third query is a plain string */
		{
			std::vector<Tile> tiles;
			int i = 0;
			for (Case & c : cases) note(c);
			for (Case & c : cases) {
				c.align = new_align((int) c.qry.size());
				bool const plainOne = i++ % 3 == 0;
				tiles.push_back(tile_of(c, plainOne ? c.qry.c_str() : c.buf.data()));
				Convex::ConvexAlignHip::Prepare(tiles.back());
			}
			run(al, tiles);
			for (int k = 0; k < n; ++k) {
				if (!same(*want[(size_t) k], *cases[(size_t) k].align, plain[(size_t) k].ret, tiles[(size_t) k].ret)) { printf("device %d mixed launch: tile %d differs\n", d, k); ++bad; }
				if (k % 3 != 0 && cases[(size_t) k].qry != cases[(size_t) k].buf.data()) { printf("device %d mixed launch: tile %d was not materialised\n", d, k); ++bad; }
			}
		}
		long l2 = 0, t2 = 0, m2 = 0;
		Convex::ConvexAlignHip::ReadStats(l2, t2, m2);
		if (l2 != l1 || t2 != t1 || m2 - m1 != 1) { printf("device %d: stats after the mixed launch: %ld launches, %ld tiles, %ld mixed\n", d, l2 - l1, t2 - t1, m2 - m1); ++bad; }
		printf("device %d of %d: %d tiles over %zu reads, %d valid\n", d, nl, n, reads.size(), valid);
	}
	/* the one reader of the characters on the host: a noted buffer swapped for the string itself */
	for (Case & c : cases) {
		note(c);
		if (!Convex::DeviceReads::Materialise(c.buf.data()) || c.qry != c.buf.data()) { printf("Materialise: wrong string\n"); ++bad; }
		if (Convex::DeviceReads::Materialise(c.buf.data())) { printf("Materialise: a buffer that holds characters\n"); ++bad; }
	}
	if (bad) { printf("segments_shim_test: %d differences\n", bad); return 1; }
	printf("segments_shim_test: ok\n");
	return 0;
}
