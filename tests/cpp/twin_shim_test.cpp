/*
 * twin_shim_test.cpp -- the C++ drop-ins in scalar-twin mode (tests/test_gpu_twin_shim.py).
 *
 * One tile with 'x' in its reference window through Convex::ConvexAlignHip and Convex::SharedAligner, each driven like
 * AlignmentBuffer::computeAlignment drives the reference aligner, with Align::svType = 1234 and Align::cigarOpCount = 77
 * going in (ngmlr stores the read's id in svType before SingleAlign, src/AlignmentBuffer.cpp:362):
 *   twin mode     both come back unchanged (Convex::ConvexAlign writes neither, src/ConvexAlign.cpp:418-467)
 *   default mode  svType is 0 and cigarOpCount the number of CIGAR operations (ConvexAlignFast)
 * and the two modes score the tile differently (the mismatches against 'x' cost mismatch * 100 in twin mode).
 * usage: twin_shim_test twin|default      (the mode of the SharedAligner: its backend is one per device and process)
 * Exit code 0 = everything as stated.
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "convex_align_hip.h"
#include "batching_aligner.h"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

struct Run { int ret, svType, cigarOpCount; float score; std::string cigar; };

static Run align(IAlignment * al, std::string const & ref, std::string const & qry) {
	int const H = (int) qry.size(), w = 120;
	std::vector<CorridorLine> lines((size_t) H);
	for (int y = 0; y < H; ++y) { lines[(size_t) y].offset = y - w / 2; lines[(size_t) y].length = w; lines[(size_t) y].offsetInMatrix = 0; }
	Align a;      /* buffers as the one caller allocates them (src/AlignmentBuffer.cpp:271-278) */
	a.maxBufferLength = H * 4; a.maxMdBufferLength = H * 4;
	a.pBuffer1 = new char[a.maxBufferLength + 16]; a.pBuffer2 = new char[a.maxMdBufferLength + 16];
	a.pBuffer1[0] = a.pBuffer2[0] = '\0';
	a.nmPerPostionLength = (H + 1) * 2;
	a.nmPerPosition = new PositionNM[a.nmPerPostionLength];
	a.svType = 1234;
	a.cigarOpCount = 77;
	Run r;
	r.ret = al->SingleAlign(0, lines.data(), H, ref.c_str(), qry.c_str(), a, 0, 0, 0);
	r.svType = a.svType; r.cigarOpCount = a.cigarOpCount; r.score = a.Score; r.cigar = a.pBuffer1;
	delete[] a.pBuffer1; delete[] a.pBuffer2; delete[] a.nmPerPosition;
	return r;
}

static int cigar_ops(std::string const & c) { int n = 0; for (char ch : c) if (ch < '0' || ch > '9') ++n; return n; }

int main(int argc, char ** argv) {
	bool const sharedTwin = argc > 1 && strcmp(argv[1], "twin") == 0;
	/* 400 bases, an 'x' every 40 in the window; the read is the window's bases with a few substitutions, so that every 'x' faces a base */
	std::string ref, qry;
	unsigned s = 12345u;
	for (int i = 0; i < 400; ++i) { s = s * 1664525u + 1013904223u; ref.push_back("ACGT"[(s >> 24) & 3]); }
	qry = ref;
	for (int i = 20; i < 400; i += 40) ref[(size_t) i] = 'x';
	for (int i = 33; i < 400; i += 97) qry[(size_t) i] = qry[(size_t) i] == 'A' ? 'C' : 'A';

	IAlignment * fast = new Convex::ConvexAlignHip(0, 2.0f, -5.0f, -5.0f, -5.0f, -1.0f, 0.15f);
	IAlignment * twin = new Convex::ConvexAlignHip(0, 2.0f, -5.0f, -5.0f, -5.0f, -1.0f, 0.15f, 0, 0, true);
	Run const f = align(fast, ref, qry), t = align(twin, ref, qry);
	printf("default: ret %d score %.1f svType %d cigarOpCount %d cigar %s\n", f.ret, f.score, f.svType, f.cigarOpCount, f.cigar.c_str());
	printf("twin:    ret %d score %.1f svType %d cigarOpCount %d cigar %s\n", t.ret, t.score, t.svType, t.cigarOpCount, t.cigar.c_str());
	CHECK(f.ret >= 0 && f.svType == 0 && f.cigarOpCount == cigar_ops(f.cigar) && f.cigarOpCount > 0 && f.cigarOpCount != 77);
	CHECK(t.ret >= 0 && t.svType == 1234 && t.cigarOpCount == 77);
	CHECK(t.score != f.score && t.cigar != f.cigar);       /* ten mismatches against 'x': bridged at -5 each by the fast form, never by the twin */
	/* a tile without a valid alignment: the twin still leaves both alone, the fast form has cleared svType */
	std::string const junk(200, 'A'), other(200, 'C');
	Run const fj = align(fast, junk, other), tj = align(twin, junk, other);
	CHECK(fj.ret < 0 && fj.svType == 0);
	CHECK(tj.ret < 0 && tj.svType == 1234 && tj.cigarOpCount == 77);
	delete fast; delete twin;

	{
		Convex::SharedAligner sh(0, 2.0f, -5.0f, -5.0f, -5.0f, -1.0f, 0.15f, -1, sharedTwin);
		Run const r = align(&sh, ref, qry);
		printf("shared (%s): ret %d score %.1f svType %d cigarOpCount %d\n", sharedTwin ? "twin" : "default", r.ret, r.score, r.svType, r.cigarOpCount);
		Run const & want = sharedTwin ? t : f;
		CHECK(r.ret == want.ret && r.score == want.score && r.cigar == want.cigar && r.svType == want.svType && r.cigarOpCount == want.cigarOpCount);
		Run const j = align(&sh, junk, other);
		CHECK(j.ret < 0 && j.svType == (sharedTwin ? 1234 : 0));
	}
	if (fails) { printf("twin_shim_test: %d checks failed\n", fails); return 1; }
	printf("twin_shim_test: ok\n");
	return 0;
}
