/*
 * ladder_shim_test.cpp -- Convex::ConvexAlignHip::AlignLadders (one device job that climbs computeAlignment's corridor retry
 * ladder, cvx_submit_ladder) against the loop a caller runs today: the corridor of rung m built on the host from
 * cvx_ladder_rung's form, the way the reference's builders write it, SingleAlign, and again at m + 1 while the attempt is invalid
 * and the rung exists.  Same return value, same Align, same rung.  tests/test_gpu_shim_ladder.py runs it.
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "convex_align_hip.h"

typedef Convex::ConvexAlignHip::LadderTile LadderTile;

static uint32_t rs = 4711;
static uint32_t rnd() { rs = rs * 1664525u + 1013904223u; return rs >> 8; }

static Align * new_align(int readLength) {
	Align * a = new Align();
	a->maxBufferLength = readLength * 4 + 64;
	a->maxMdBufferLength = readLength * 4 + 64;
	a->pBuffer1 = new char[a->maxBufferLength + 16];
	a->pBuffer2 = new char[a->maxMdBufferLength + 16];
	a->pBuffer1[0] = '\0'; a->pBuffer2[0] = '\0';
	a->nmPerPostionLength = (readLength + 1) * 2;
	a->nmPerPosition = new PositionNM[a->nmPerPostionLength];
	a->svType = 0;
	return a;
}

static bool same(Align const & a, Align const & b, int ra, int rb) {
	return ra == rb && memcmp(&a.Score, &b.Score, 4) == 0 && (ra < 0 || (memcmp(&a.Identity, &b.Identity, 4) == 0 && a.QStart == b.QStart && a.QEnd == b.QEnd &&
			a.PositionOffset == b.PositionOffset && a.NM == b.NM && a.alignmentLength == b.alignmentLength && a.cigarOpCount == b.cigarOpCount &&
			strcmp(a.pBuffer1, b.pBuffer1) == 0 && strcmp(a.pBuffer2, b.pBuffer2) == 0));
}

struct Case {
	std::string ref, qry;
	cvx_ladder ladder;
};

int main() {
	/* reads of 500 bases: 250 matched, a deletion of d, 250 matched, a few substitutions; the window is what they span */
	std::string genome;
	for (int k = 0; k < 3000; ++k) genome.push_back("ACGT"[rnd() % 4]);
	int const dels[] = { 0, 15, 60, 100, 130, 200, 250, 300, 400, 40, 160, 90 };
	std::vector<Case> cases;
	for (size_t i = 0; i < sizeof(dels) / sizeof(dels[0]); ++i) {
		Case c;
		int const d = dels[i], at = (int) (rnd() % 1500);
		c.ref = genome.substr((size_t) at, (size_t) (500 + d));
		c.qry = c.ref.substr(0, 250) + c.ref.substr((size_t) (250 + d));
		for (int k = 0; k < 8; ++k) c.qry[rnd() % c.qry.size()] = "ACGT"[rnd() % 4];
		memset(&c.ladder, 0, sizeof(c.ladder));
		c.ladder.corridor = i % 4 == 3 ? 64 : 256;
		if (i % 3 == 1) { c.ladder.flags = CVX_LADDER_ANCHORS; c.ladder.left = 40.0f + (float) i; c.ladder.right = 37.5f; }
		if (i % 5 == 4) c.ladder.flags |= CVX_LADDER_REALIGN;
		cases.push_back(c);
	}
	{ Case c; c.ref = genome.substr(100, 400); c.qry = genome.substr(130, 300); memset(&c.ladder, 0, sizeof(c.ladder)); c.ladder.corridor = 100; c.ladder.flags = CVX_LADDER_FULL; cases.push_back(c); }
	{ Case c; c.ref = genome.substr(700, 100); c.qry = genome.substr(700, 100); memset(&c.ladder, 0, sizeof(c.ladder)); c.ladder.corridor = 120; c.ladder.flags = CVX_LADDER_SHORT; cases.push_back(c); }
	int const n = (int) cases.size();
	int bad = 0;

	Convex::ConvexAlignHip al(0, 2.0f, -5.0f, -5.0f, -5.0f, -1.0f, 0.15f, 0);
	/* the loop of today: one SingleAlign per rung */
	std::vector<Align *> want((size_t) n);
	std::vector<int> wantRet((size_t) n, -1), wantRung((size_t) n, 0), wantWidth((size_t) n, 0);
	for (int i = 0; i < n; ++i) {
		Case & c = cases[(size_t) i];
		int const H = (int) c.qry.size();
		want[(size_t) i] = new_align(H);
		cvx_tile t;
		memset(&t, 0, sizeof(t));
		t.ref_len = (int32_t) c.ref.size(); t.qry_len = H;
		for (int m = 1;; ++m) {
			cvx_tile form;
			memset(&form, 0, sizeof(form));
			int const rc = cvx_ladder_rung(&t, &c.ladder, m, &form);
			if (rc < 0) { printf("cvx_ladder_rung: %s\n", cvx_last_error()); return 1; }
			if (rc == 0) break;
			std::vector<CorridorLine> lines((size_t) H);
			for (int y = 0; y < H; ++y) {
				lines[(size_t) y].offset = form.corridor_kind == CVX_CORRIDOR_CONST ? form.corridor_offset : (int) (((float) y - form.corridor_d) / form.corridor_k - form.corridor_right);
				lines[(size_t) y].length = form.corridor_width;
				lines[(size_t) y].offsetInMatrix = 0;
			}
			wantRung[(size_t) i] = m;
			wantWidth[(size_t) i] = form.corridor_width;
			wantRet[(size_t) i] = al.SingleAlign(0, lines.data(), H, c.ref.c_str(), c.qry.c_str(), *want[(size_t) i], 0, 0, 0);
			if (wantRet[(size_t) i] >= 0) break;
		}
	}
	/* the ladders in one job */
	std::vector<LadderTile> tiles((size_t) n);
	for (int i = 0; i < n; ++i) {
		LadderTile & t = tiles[(size_t) i];
		memset(&t, 0, sizeof(t));
		t.refSeq = cases[(size_t) i].ref.c_str(); t.qrySeq = cases[(size_t) i].qry.c_str();
		t.result = new_align((int) cases[(size_t) i].qry.size());
		t.ladder = cases[(size_t) i].ladder;
		t.ret = -2;
	}
	al.AlignLadders(tiles.data(), n);
	int rungs[6] = { 0, 0, 0, 0, 0, 0 }, valid = 0;
	for (int i = 0; i < n; ++i) {
		LadderTile const & t = tiles[(size_t) i];
		if (t.failed || t.rung != wantRung[(size_t) i] || t.attempts != t.rung || t.width != wantWidth[(size_t) i] || !same(*want[(size_t) i], *t.result, wantRet[(size_t) i], t.ret)) {
			printf("tile %d: rung %d (want %d), width %d (want %d), ret %d (want %d)%s\n", i, t.rung, wantRung[(size_t) i], t.width, wantWidth[(size_t) i], t.ret, wantRet[(size_t) i], t.failed ? ", failed" : "");
			++bad;
		}
		if (t.rung >= 1 && t.rung <= 5) rungs[t.rung] += 1;
		valid += t.ret >= 0;
	}
	printf("%d ladders: %d valid; reported at rung 1..5: %d %d %d %d %d\n", n, valid, rungs[1], rungs[2], rungs[3], rungs[4], rungs[5]);
	if (rungs[1] == 0 || rungs[2] + rungs[3] + rungs[4] + rungs[5] < 3 || valid < n / 2 || valid == n) { printf("the cases do not climb as intended\n"); ++bad; }
	if (bad) { printf("ladder_shim_test: %d differences\n", bad); return 1; }
	printf("ladder_shim_test: ok\n");
	return 0;
}
