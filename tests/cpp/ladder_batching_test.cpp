/*
 * ladder_batching_test.cpp -- Convex::SharedAligner::SingleLadder: eight threads, each with its own SharedAligner as ngmlr's
 * workers have theirs, hand whole retry ladders to the one dispatcher of the device, which gathers them into ladder launches
 * (ConvexAlignHip::PrepareLadder in the caller's context / SubmitLadders / FinishLadder in the caller's thread).  Every answer --
 * return value, every Align field, CIGAR, MD, note, rung / attempts / width -- against ConvexAlignHip::AlignLadders on that tile
 * alone on a private aligner with the same flags.  The tiles are ladder_stages_shim_test.cpp's engineered ones at a few hundred
 * rows: deletions that resolve at rungs 1 .. 5, one no rung resolves, one whose ladder the cap ends, anchors, FULL, SHORT and
 * REALIGN tiles.
 *
 *   phase 1   every reference a DeviceWindows placeholder, noted in the thread that calls: launches gathered from eight calling
 *             contexts travel as windows of the genome -- what AlignLadders, which resolves in its one calling thread, cannot form
 *   phase 2   plain strings; two of the threads interleave plain SingleAlign calls, so launches are of both kinds; one poisoned
 *             request (a CIGAR buffer far too small) must fail alone
 *
 * argv[1]: plain | regions | jobtext | twin -- the flags of the shared backend (regions: the binding's finder site announced;
 * jobtext: and the aligners constructed with jobText; twin: scalar-twin mode).  With CVX_DEVICE_LADDER=0 in the environment
 * every SingleLadder must answer false and nothing may be queued.  The dispatcher runs with a batch target of eight and a hold
 * of 20 ms (the pool's rule, at this test's size): a launch waits until eight requests are queued, or that long.
 * tests/test_gpu_shim_ladder_batching.py runs it.
 */
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "batching_aligner.h"
#include "nm_regions_note.h"

typedef Convex::ConvexAlignHip::LadderTile LadderTile;
typedef Convex::NmRegionsNote Note;

static std::atomic<int> fails(0);
#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

static uint32_t rs = 90210;
static uint32_t rnd() { rs = rs * 1664525u + 1013904223u; return rs >> 8; }
static char other(char c) { return c == 'A' ? 'C' : c == 'C' ? 'G' : c == 'G' ? 'T' : 'A'; }

static int const kSmallRows = 16;
static int const kThreads = 8;

struct Case {
	int at;                /* the window's first base in the genome sequence */
	std::string ref, qry;
	cvx_ladder ladder;
	int extStart, extEnd;
};

struct Held {
	Align a;
	int ret, rung, attempts, width;
	bool failed, taken;
	Held(int H, bool marked) : ret(-2), rung(0), attempts(0), width(0), failed(false), taken(true) {
		a.maxBufferLength = H * 4 + 64; a.maxMdBufferLength = H * 4 + 64;
		a.pBuffer1 = new char[a.maxBufferLength + 16]; a.pBuffer2 = new char[a.maxMdBufferLength + 16];
		a.pBuffer1[0] = a.pBuffer2[0] = '\0';
		a.nmPerPostionLength = marked ? kSmallRows : (H + 1) * 2;
		a.nmPerPosition = new PositionNM[a.nmPerPostionLength];
		a.svType = 0; a.cigarOpCount = 0;
		if (marked) Note::Request(a.nmPerPosition);
	}
	~Held() { delete[] a.pBuffer1; delete[] a.pBuffer2; delete[] a.nmPerPosition; }
private:
	Held(Held const &);
	Held & operator=(Held const &);
};

static bool same(Held const & x, Held const & y, bool marked) {
	Align const & p = x.a, & q = y.a;
	if (x.ret != y.ret || x.failed != y.failed || x.rung != y.rung || x.attempts != y.attempts || x.width != y.width) return false;
	if (x.failed) return true;
	if (x.ret < 0) return p.Score == q.Score && (!marked || (Note::IsRequest(p.nmPerPosition, p.nmPerPostionLength) && Note::IsRequest(q.nmPerPosition, q.nmPerPostionLength)));
	bool const ok = memcmp(&p.Score, &q.Score, sizeof(float)) == 0 && memcmp(&p.Identity, &q.Identity, sizeof(float)) == 0 && p.NM == q.NM &&
			p.QStart == q.QStart && p.QEnd == q.QEnd && p.alignmentLength == q.alignmentLength && p.PositionOffset == q.PositionOffset &&
			p.cigarOpCount == q.cigarOpCount && p.svType == q.svType &&
			p.firstPosition.refPosition == q.firstPosition.refPosition && p.firstPosition.readPosition == q.firstPosition.readPosition &&
			p.lastPosition.refPosition == q.lastPosition.refPosition && p.lastPosition.readPosition == q.lastPosition.readPosition &&
			strcmp(p.pBuffer1, q.pBuffer1) == 0 && strcmp(p.pBuffer2, q.pBuffer2) == 0;
	if (!ok) return false;
	if (marked) {
		int n = -1, m = -2;
		if (!Note::IsNote(p.nmPerPosition, p.nmPerPostionLength, n) || !Note::IsNote(q.nmPerPosition, q.nmPerPostionLength, m) || n != m) return false;
		for (int i = 0; i < n; ++i) {
			Note::Region const g = Note::At(p.nmPerPosition, i), h = Note::At(q.nmPerPosition, i);
			if (memcmp(&g, &h, sizeof(g)) != 0) return false;
		}
		return true;
	}
	int const rows = p.alignmentLength < p.nmPerPostionLength ? p.alignmentLength : p.nmPerPostionLength;
	return memcmp(p.nmPerPosition, q.nmPerPosition, (size_t) rows * sizeof(PositionNM)) == 0;
}

/* rung 1 of a case's ladder as the CorridorLine[] a plain SingleAlign takes */
static std::vector<CorridorLine> rung_one(Case const & c) {
	int const H = (int) c.qry.size();
	cvx_tile t, form;
	memset(&t, 0, sizeof(t));
	memset(&form, 0, sizeof(form));
	t.ref_len = (int32_t) c.ref.size(); t.qry_len = H;
	std::vector<CorridorLine> lines((size_t) H);
	if (cvx_ladder_rung(&t, &c.ladder, 1, &form) != 1) { printf("cvx_ladder_rung: %s\n", cvx_last_error()); ++fails; return lines; }
	for (int y = 0; y < H; ++y) {
		lines[(size_t) y].offset = form.corridor_kind == CVX_CORRIDOR_CONST ? form.corridor_offset : (int) (((float) y - form.corridor_d) / form.corridor_k - form.corridor_right);
		lines[(size_t) y].length = form.corridor_width;
		lines[(size_t) y].offsetInMatrix = 0;
	}
	return lines;
}

struct Barrier {
	std::atomic<int> arrived;
	Barrier() : arrived(0) {}
	void wait(int round) { arrived.fetch_add(1); while (arrived.load() < round * kThreads) std::this_thread::yield(); }
};

int main(int argc, char ** argv) {
	std::string const mode = argc > 1 ? argv[1] : "plain";
	bool const regionsOn = mode == "regions" || mode == "jobtext", jobText = mode == "jobtext", twin = mode == "twin";
	if (!regionsOn && !twin && mode != "plain") { fprintf(stderr, "usage: ladder_batching_test plain | regions | jobtext | twin\n"); return 2; }
	bool ladderOff = false;
	if (char const * e = getenv("CVX_DEVICE_LADDER")) ladderOff = atoi(e) == 0;
	setenv("CVX_BATCH_TARGET", "8", 1);
	setenv("CVX_BATCH_HOLD_US", "20000", 1);
	if (regionsOn) Convex::DeviceRegions::Announce();

	std::string genome;
	for (int k = 0; k < 8000; ++k) genome.push_back("ACGT"[rnd() % 4]);
	char const * sp[1] = { genome.c_str() };
	uint64_t lens[1] = { genome.size() };
	std::vector<uint8_t> bin((size_t) cvx_genome_encoded_bytes(1, lens));
	uint64_t nNibbles = 0, starts[2];
	int32_t nStarts = 0;
	if (cvx_genome_encode(1, sp, lens, bin.data(), &nNibbles, starts, &nStarts) != CVX_OK) { printf("encode failed\n"); return 1; }
	Convex::DeviceWindows::SetGenome(bin.data(), nNibbles, (unsigned long long const *) starts, nStarts);
	if (!Convex::DeviceWindows::Enabled()) { printf("CVX_DEVICE_DECODE=0\n"); return 1; }
	if (regionsOn != Convex::DeviceRegions::Enabled()) { printf("CVX_DEVICE_REGIONS=0\n"); return 1; }

	/* reads of 2 * flank bases: flank matched, a deletion of d, flank matched; with `bursts` a 24-base substitution burst every 110
	 * bases (mismatches for the regions to find; a burst also lets a local alignment end inside a corridor that an unbroken flank
	 * runs out of).  Without anchors rung m is corridor * m / 4 columns wide around the line from corner to corner, from which a
	 * deletion of d in the middle leads the path d / 2 away: the unbroken tiles at a fixed window resolve at rungs 1, 2, 3, 4 and 5
	 * (checked below on the private aligner), the tile of corridor 64 at none, and the tile of corridor 1200 has one rung --
	 * 1200 * 2 > 2 * (850 + 1), the cap -- which fails. */
	struct Spec { int flank, d, corridor, flags; float left, right; int extStart, extEnd; bool bursts; int at; };
	Spec const specs[] = {
		{ 300, 0, 256, 0, 0.0f, 0.0f, 0, 0, true, -1 }, { 300, 30, 256, 0, 0.0f, 0.0f, 7, 0, true, -1 }, { 300, 75, 256, 0, 0.0f, 0.0f, 0, 12, true, -1 }, { 300, 90, 256, 0, 0.0f, 0.0f, 3, 4999, true, -1 },
		{ 300, 125, 256, 0, 0.0f, 0.0f, 0, 0, true, -1 }, { 300, 190, 256, 0, 0.0f, 0.0f, 1, 2, true, -1 }, { 300, 240, 256, 0, 0.0f, 0.0f, 0, 0, true, -1 },
		{ 300, 80, 256, 0, 0.0f, 0.0f, 0, 0, false, 1000 }, { 300, 130, 256, 0, 0.0f, 0.0f, 0, 0, false, 1000 }, { 300, 160, 256, 0, 0.0f, 0.0f, 0, 0, false, 1000 },
		{ 300, 300, 64, 0, 0.0f, 0.0f, 0, 0, false, -1 },                  /* never: five rungs of at most 80 columns */
		{ 300, 550, 1200, 0, 0.0f, 0.0f, 0, 0, false, 1000 },              /* the cap: one rung of 300 columns */
		{ 300, 120, 256, CVX_LADDER_ANCHORS, 40.0f, 40.0f, 0, 0, true, -1 }, { 300, 200, 256, CVX_LADDER_ANCHORS, 40.0f, 40.0f, 5, 5, true, -1 },
		{ 300, 150, 100, CVX_LADDER_REALIGN, 0.0f, 0.0f, 0, 0, true, -1 }, { 300, 180, 256, 0, 0.0f, 0.0f, 0, 0, false, 1000 },
		{ 300, 50, 256, CVX_LADDER_FULL, 0.0f, 0.0f, 0, 0, true, -1 }, { 300, 20, 256, 0, 0.0f, 0.0f, 0, 3, false, 1000 },
		{ 300, 50, 256, CVX_LADDER_SHORT, 0.0f, 0.0f, 0, 0, true, -1 }, { 200, 200, 128, CVX_LADDER_SHORT, 0.0f, 0.0f, 4, 0, true, -1 },
	};
	std::vector<Case> cases;
	for (Spec const & s : specs) {
		Case c;
		c.at = s.at >= 0 ? s.at : (int) (rnd() % 5000);
		c.ref = genome.substr((size_t) c.at, (size_t) (2 * s.flank + s.d));
		c.qry = c.ref.substr(0, (size_t) s.flank) + c.ref.substr((size_t) (s.flank + s.d));
		for (int part = 0; part < 2 && s.bursts; ++part) for (int a = 60; a < s.flank - 60 - 24; a += 110) for (int k = 0; k < 24; ++k) {
			char & b = c.qry[(size_t) (part * s.flank + a + k)];
			b = other(b);
		}
		memset(&c.ladder, 0, sizeof(c.ladder));
		c.ladder.corridor = s.corridor; c.ladder.flags = s.flags; c.ladder.left = s.left; c.ladder.right = s.right;
		c.extStart = s.extStart; c.extEnd = s.extEnd;
		cases.push_back(c);
	}
	size_t const n = cases.size();
	size_t const kNever = 10, kCap = 11;
	std::vector<bool> marked(n);
	for (size_t i = 0; i < n; ++i) marked[i] = regionsOn && i % 3 != 2;      /* a request on every tile but each third: the host form beside them in one launch */

	if (ladderOff) {
		/* CVX_DEVICE_LADDER=0: nothing is taken, nothing is queued */
		Convex::SharedAligner mine(0, 2.0f, -5.0f, -5.0f, -5.0f, -1.0f, 0.15f, -1, twin, jobText);
		for (size_t i = 0; i < n; ++i) {
			Held h((int) cases[i].qry.size(), marked[i]);
			int ret = -7, rung = -7, attempts = -7, width = -7;
			bool const took = mine.SingleLadder(cases[i].ref.c_str(), cases[i].qry.c_str(), h.a, cases[i].extStart, cases[i].extEnd, cases[i].ladder, ret, rung, attempts, width);
			CHECK(!took && ret == -7 && rung == -7 && attempts == -7 && width == -7 && h.a.pBuffer1[0] == '\0');
		}
		CHECK(Convex::SharedAligner::Requests() == 0 && Convex::SharedAligner::Launches() == 0);
		if (fails) { printf("ladder_batching_test %s (CVX_DEVICE_LADDER=0): %d failures\n", mode.c_str(), fails.load()); return 1; }
		printf("ladder_batching_test %s (CVX_DEVICE_LADDER=0): ok, %zu calls answered false, nothing queued\n", mode.c_str(), n);
		return 0;
	}

	/* what every answer must be: AlignLadders on that tile alone, and SingleAlign on rung 1 of it, on a private aligner */
	std::vector<Held *> want, wantPlain;
	{
		Convex::ConvexAlignHip al(0, 2.0f, -5.0f, -5.0f, -5.0f, -1.0f, 0.15f, 0, 0, twin, regionsOn, jobText);
		for (size_t i = 0; i < n; ++i) {
			want.push_back(new Held((int) cases[i].qry.size(), marked[i]));
			LadderTile t;
			memset(&t, 0, sizeof(t));
			t.refSeq = cases[i].ref.c_str(); t.qrySeq = cases[i].qry.c_str(); t.result = &want[i]->a;
			t.externalQStart = cases[i].extStart; t.externalQEnd = cases[i].extEnd; t.ladder = cases[i].ladder;
			al.AlignLadders(&t, 1);
			want[i]->ret = t.ret; want[i]->failed = t.failed; want[i]->rung = t.rung; want[i]->attempts = t.attempts; want[i]->width = t.width;
			wantPlain.push_back(new Held((int) cases[i].qry.size(), marked[i]));
			std::vector<CorridorLine> lines = rung_one(cases[i]);
			try { wantPlain[i]->ret = al.SingleAlign(0, lines.data(), (int) lines.size(), cases[i].ref.c_str(), cases[i].qry.c_str(), wantPlain[i]->a, cases[i].extStart, cases[i].extEnd, 0); }
			catch (...) { wantPlain[i]->failed = true; }
		}
	}
	{
		bool at[6] = { false, false, false, false, false, false };
		for (size_t i = 0; i < n; ++i) if (want[i]->ret >= 0 && want[i]->rung >= 1 && want[i]->rung <= 5) at[want[i]->rung] = true;
		printf("alone:");
		for (size_t i = 0; i < n; ++i) printf(" %d/%d%s", want[i]->rung, want[i]->attempts, want[i]->ret < 0 ? "!" : "");
		printf("  (rung / attempts per tile, ! = no alignment)\n");
		CHECK(at[1] && at[2] && at[3] && at[4] && at[5]);      /* tiles that resolve at every rung */
		CHECK(want[kNever]->ret < 0 && want[kNever]->attempts == 5);
		{      /* unresolved because the cap leaves no further rung, not because five attempts ran */
			cvx_tile t, form;
			memset(&t, 0, sizeof(t));
			memset(&form, 0, sizeof(form));
			t.ref_len = (int32_t) cases[kCap].ref.size(); t.qry_len = (int32_t) cases[kCap].qry.size();
			CHECK(want[kCap]->ret < 0 && want[kCap]->attempts >= 1 && want[kCap]->attempts < 5 && cvx_ladder_rung(&t, &cases[kCap].ladder, want[kCap]->attempts + 1, &form) == 0);
		}
		for (size_t i = 0; i < n; ++i) CHECK(!want[i]->failed);
	}

	/* got[w][i]: thread w's answer for case i in phase 1 (windows) and phase 2 (strings); plain[w][i]: its interleaved SingleAlign */
	std::vector<std::vector<Held *> > got1((size_t) kThreads), got2((size_t) kThreads), plain((size_t) kThreads);
	for (int w = 0; w < kThreads; ++w) for (size_t i = 0; i < n; ++i) {
		got1[(size_t) w].push_back(new Held((int) cases[i].qry.size(), marked[i]));
		got2[(size_t) w].push_back(new Held((int) cases[i].qry.size(), marked[i]));
		plain[(size_t) w].push_back(0);
	}
	int const kPoisonThread = 3;
	size_t const kPoisonCase = 4;
	CHECK(want[kPoisonCase]->ret >= 0 && strlen(want[kPoisonCase]->a.pBuffer1) > 8);
	got2[(size_t) kPoisonThread][kPoisonCase]->a.maxBufferLength = 8;      /* a hard error of that tile alone (src/AlignmentBuffer.cpp:454-463) */
	long wl0 = 0, wt0 = 0, wm0 = 0, wl1 = 0, wt1 = 0, wm1 = 0, wl2 = 0, wt2 = 0, wm2 = 0;
	Convex::ConvexAlignHip::WindowStats(wl0, wt0, wm0);
	Barrier barrier;
	std::atomic<long> plainCalls(0);
	std::vector<std::thread> th;
	for (int w = 0; w < kThreads; ++w) {
		th.emplace_back([&, w]() {
			Convex::SharedAligner mine(0, 2.0f, -5.0f, -5.0f, -5.0f, -1.0f, 0.15f, -1, twin, jobText);
			barrier.wait(1);
			for (size_t j = 0; j < n; ++j) {
				size_t const i = (j + (size_t) w * 3) % n;
				Case const & c = cases[i];
				Held & h = *got1[(size_t) w][i];
				int const length = (int) c.ref.size() + 1;
				std::vector<char> buf((size_t) length + 100);
				Convex::DeviceWindows::Placeholder(buf.data(), (unsigned long long) starts[0] + (unsigned long long) c.at, length);
				try { h.taken = mine.SingleLadder(buf.data(), c.qry.c_str(), h.a, c.extStart, c.extEnd, c.ladder, h.ret, h.rung, h.attempts, h.width); }
				catch (...) { h.failed = true; }
				if (buf[0] != 'x') { printf("FAIL: a window placeholder was written\n"); ++fails; }      /* decoded on the device: nothing wrote the caller's buffer */
			}
			barrier.wait(2);
			if (w == 0) Convex::ConvexAlignHip::WindowStats(wl1, wt1, wm1);
			barrier.wait(3);
			for (size_t j = 0; j < n; ++j) {
				size_t const i = (j + (size_t) w * 3) % n;
				Case const & c = cases[i];
				Held & h = *got2[(size_t) w][i];
				try { h.taken = mine.SingleLadder(c.ref.c_str(), c.qry.c_str(), h.a, c.extStart, c.extEnd, c.ladder, h.ret, h.rung, h.attempts, h.width); }
				catch (...) { h.failed = true; }
				if ((w == 1 || w == 6) && j % 5 == 2) {      /* a plain request between two ladders */
					Held * p = new Held((int) c.qry.size(), marked[i]);
					plain[(size_t) w][i] = p;
					std::vector<CorridorLine> lines = rung_one(c);
					try { p->ret = mine.SingleAlign(0, lines.data(), (int) lines.size(), c.ref.c_str(), c.qry.c_str(), p->a, c.extStart, c.extEnd, 0); }
					catch (...) { p->failed = true; }
					plainCalls.fetch_add(1);
				}
			}
		});
	}
	for (auto & t : th) t.join();
	Convex::ConvexAlignHip::WindowStats(wl2, wt2, wm2);

	int ok1 = 0, ok2 = 0, okPlain = 0;
	for (int w = 0; w < kThreads; ++w) for (size_t i = 0; i < n; ++i) {
		Held const & a = *got1[(size_t) w][i], & b = *got2[(size_t) w][i];
		bool const s1 = a.taken && same(*want[i], a, marked[i]);
		if (!s1) printf("  windows: thread %d case %zu differs: rung %d (want %d), width %d (want %d), ret %d (want %d)%s\n", w, i, a.rung, want[i]->rung, a.width, want[i]->width, a.ret, want[i]->ret, a.failed ? ", failed" : "");
		CHECK(s1);
		ok1 += s1;
		bool s2;
		if (w == kPoisonThread && i == kPoisonCase) s2 = b.failed;      /* its own hard error, in its own thread */
		else s2 = b.taken && same(*want[i], b, marked[i]);              /* nobody else is dragged along */
		if (!s2) printf("  strings: thread %d case %zu differs: rung %d (want %d), width %d (want %d), ret %d (want %d)%s\n", w, i, b.rung, want[i]->rung, b.width, want[i]->width, b.ret, want[i]->ret, b.failed ? ", failed" : "");
		CHECK(s2);
		ok2 += s2;
		if (Held const * p = plain[(size_t) w][i]) {
			Held const & q = *wantPlain[i];
			bool sp = p->failed == q.failed && p->ret == q.ret;
			if (sp && !p->failed) sp = same(q, *p, marked[i]);      /* (the ladder fields of both are as constructed) */
			if (!sp) printf("  SingleAlign: thread %d case %zu differs: ret %d (want %d)\n", w, i, p->ret, q.ret);
			CHECK(sp);
			okPlain += sp;
		}
	}
	long const ladderCalls = 2L * kThreads * (long) n, requests = Convex::SharedAligner::Requests(), launches = Convex::SharedAligner::Launches();
	printf("ladder_batching_test %s: %d of %ld window ladders and %d of %ld string ladders as AlignLadders leaves them alone, %d of %ld interleaved SingleAlign calls; "
			"%ld requests in %ld launches; phase 1: %ld windows in %ld window launches\n", mode.c_str(), ok1, ladderCalls / 2, ok2, ladderCalls / 2, okPlain, plainCalls.load(),
			requests, launches, wt1 - wt0, wl1 - wl0);
	CHECK(plainCalls.load() >= 4);
	CHECK(requests == ladderCalls + plainCalls.load());
	CHECK(launches * 4 <= requests);
	/* phase 1: every launch travelled as windows of the genome, gathered from several calling contexts */
	CHECK(wt1 - wt0 == (long) kThreads * (long) n && wm1 == wm0 && (wl1 - wl0) * 4 <= wt1 - wt0);
	CHECK(wl2 == wl1 && wm2 == wm1);      /* phase 2 carried none */

	for (int w = 0; w < kThreads; ++w) for (size_t i = 0; i < n; ++i) { delete got1[(size_t) w][i]; delete got2[(size_t) w][i]; delete plain[(size_t) w][i]; }
	for (size_t i = 0; i < n; ++i) { delete want[i]; delete wantPlain[i]; }
	if (fails) { printf("ladder_batching_test %s: %d failures\n", mode.c_str(), fails.load()); return 1; }
	printf("ladder_batching_test %s: ok, 1 request failed alone as it must\n", mode.c_str());
	return 0;
}
