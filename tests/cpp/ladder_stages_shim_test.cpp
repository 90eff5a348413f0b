/*
 * ladder_stages_shim_test.cpp -- Convex::ConvexAlignHip::AlignLadders on aligners constructed with nmRegions, with jobText and
 * with both (cvx_submit_ladder_ex), against the loop a caller runs today on an equally flagged aligner: SingleAlign rung by
 * rung on the corridor built from cvx_ladder_rung's form, into the same kind of Align -- one whose small nmPerPosition holds a
 * request (answered with a note of the reported rung's regions; with jobText its CIGAR and MD come from the job's text) or one
 * with the reference's own profile buffer (the host form).  Same return value, Align fields, CIGAR, MD, note and rung / attempts /
 * width.  Then Submit's input forms against the plain-string form: every reference a DeviceWindows placeholder (the genome
 * form; the note of a window belongs to the calling context, so a launch from one thread carries one), every query a DeviceReads
 * placeholder (the segments form, tiles sharing reads), and a launch that mixes them (materialised on the host).
 * tests/test_gpu_shim_ladder_stages.py runs it.
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "convex_align_hip.h"
#include "nm_regions_note.h"

typedef Convex::ConvexAlignHip::LadderTile LadderTile;
typedef Convex::NmRegionsNote Note;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

static uint32_t rs = 90210;
static uint32_t rnd() { rs = rs * 1664525u + 1013904223u; return rs >> 8; }
static char other(char c) { return c == 'A' ? 'C' : c == 'C' ? 'G' : c == 'G' ? 'T' : 'A'; }
static char comp(char c) { return c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : c; }

static int const kSmallRows = 16;

struct Case {
	int at;                /* the window's first base in the genome sequence */
	std::string ref, qry;
	cvx_ladder ladder;
	int extStart, extEnd;
};

struct Held {
	Align a;
	int ret, rung, attempts, width;
	bool failed;
	Held(int H, bool marked) : ret(-2), rung(0), attempts(0), width(0), failed(false) {
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

/* the loop of today: one SingleAlign per rung, into one Align */
static void rung_by_rung(Convex::ConvexAlignHip & al, Case const & c, Held & h) {
	int const H = (int) c.qry.size();
	cvx_tile t;
	memset(&t, 0, sizeof(t));
	t.ref_len = (int32_t) c.ref.size(); t.qry_len = H;
	for (int m = 1;; ++m) {
		cvx_tile form;
		memset(&form, 0, sizeof(form));
		int const rc = cvx_ladder_rung(&t, &c.ladder, m, &form);
		if (rc < 0) { printf("cvx_ladder_rung: %s\n", cvx_last_error()); ++fails; return; }
		if (rc == 0) break;
		std::vector<CorridorLine> lines((size_t) H);
		for (int y = 0; y < H; ++y) {
			lines[(size_t) y].offset = form.corridor_kind == CVX_CORRIDOR_CONST ? form.corridor_offset : (int) (((float) y - form.corridor_d) / form.corridor_k - form.corridor_right);
			lines[(size_t) y].length = form.corridor_width;
			lines[(size_t) y].offsetInMatrix = 0;
		}
		h.rung = h.attempts = m;
		h.width = form.corridor_width;
		h.ret = al.SingleAlign(0, lines.data(), H, c.ref.c_str(), c.qry.c_str(), h.a, c.extStart, c.extEnd, 0);
		if (h.ret >= 0) break;
	}
}

static LadderTile ladder_tile(Case const & c, char const * ref, char const * qry, Held & h) {
	LadderTile t;
	memset(&t, 0, sizeof(t));
	t.refSeq = ref; t.qrySeq = qry; t.result = &h.a;
	t.externalQStart = c.extStart; t.externalQEnd = c.extEnd;
	t.ladder = c.ladder;
	t.ret = -2;
	return t;
}

static void take(Held & h, LadderTile const & t) { h.ret = t.ret; h.failed = t.failed; h.rung = t.rung; h.attempts = t.attempts; h.width = t.width; }

static void compare(char const * form, std::vector<Case> const & cases, std::vector<Held *> const & want, std::vector<Held *> const & got, std::vector<bool> const & marked) {
	int ok = 0;
	for (size_t i = 0; i < cases.size(); ++i) {
		bool const s = same(*want[i], *got[i], marked[i]);
		if (!s) printf("  %s: case %zu differs: rung %d (want %d), width %d (want %d), ret %d (want %d)%s\n", form, i, got[i]->rung, want[i]->rung, got[i]->width, want[i]->width,
				got[i]->ret, want[i]->ret, got[i]->failed ? ", failed" : "");
		CHECK(s);
		ok += s;
	}
	printf("  %s: %d of %zu as SingleAlign rung by rung leaves them\n", form, ok, cases.size());
}

static void free_all(std::vector<Held *> & v) { for (Held * h : v) delete h; v.clear(); }

int main() {
	std::string genome;
	for (int k = 0; k < 8000; ++k) genome.push_back("ACGT"[rnd() % 4]);
	char const * sp[1] = { genome.c_str() };
	uint64_t lens[1] = { genome.size() };
	std::vector<uint8_t> bin((size_t) cvx_genome_encoded_bytes(1, lens));
	uint64_t nNibbles = 0, starts[2];
	int32_t nStarts = 0;
	if (cvx_genome_encode(1, sp, lens, bin.data(), &nNibbles, starts, &nStarts) != CVX_OK) { printf("encode failed\n"); return 1; }
	Convex::DeviceWindows::SetGenome(bin.data(), nNibbles, (unsigned long long const *) starts, nStarts);
	if (!Convex::DeviceWindows::Enabled() || !Convex::DeviceReads::Enabled()) { printf("CVX_DEVICE_DECODE=0 / CVX_DEVICE_READS=0\n"); return 1; }

	/* reads of 2 * flank bases: flank matched, a deletion of d, flank matched, a 24-base substitution burst every 110 bases (but for
	 * the tile no rung resolves: corridor 64, a deletion of 300) */
	struct Spec { int flank, d, corridor, flags; float left, right; int extStart, extEnd; };
	Spec const specs[] = {
		{ 600, 0, 256, 0, 0.0f, 0.0f, 0, 0 }, { 600, 80, 256, 0, 0.0f, 0.0f, 7, 0 }, { 600, 130, 256, 0, 0.0f, 0.0f, 0, 12 }, { 600, 170, 256, 0, 0.0f, 0.0f, 3, 4999 },
		{ 600, 120, 256, CVX_LADDER_ANCHORS, 40.0f, 40.0f, 0, 0 }, { 600, 200, 256, CVX_LADDER_ANCHORS, 40.0f, 40.0f, 5, 5 }, { 600, 150, 100, CVX_LADDER_REALIGN, 0.0f, 0.0f, 0, 0 },
		{ 300, 300, 64, 0, 0.0f, 0.0f, 0, 0 }, { 300, 90, 256, 0, 0.0f, 0.0f, 1, 2 }, { 400, 50, 256, CVX_LADDER_FULL, 0.0f, 0.0f, 0, 0 },
	};
	std::vector<Case> cases;
	for (Spec const & s : specs) {
		Case c;
		c.at = (int) (rnd() % 5000);
		c.ref = genome.substr((size_t) c.at, (size_t) (2 * s.flank + s.d));
		c.qry = c.ref.substr(0, (size_t) s.flank) + c.ref.substr((size_t) (s.flank + s.d));
		for (int part = 0; part < 2 && s.corridor != 64; ++part) for (int a = 60; a < s.flank - 60 - 24; a += 110) for (int k = 0; k < 24; ++k) {
			char & b = c.qry[(size_t) (part * s.flank + a + k)];
			b = other(b);
		}
		memset(&c.ladder, 0, sizeof(c.ladder));
		c.ladder.corridor = s.corridor; c.ladder.flags = s.flags; c.ladder.left = s.left; c.ladder.right = s.right;
		c.extStart = s.extStart; c.extEnd = s.extEnd;
		cases.push_back(c);
	}
	size_t const n = cases.size();

	bool const combos[3][2] = { { true, false }, { false, true }, { true, true } };
	for (int k = 0; k < 3; ++k) {
		bool const regionsOn = combos[k][0], jobText = combos[k][1];
		printf("aligner with%s%s\n", regionsOn ? " nmRegions" : "", jobText ? " jobText" : "");
		Convex::ConvexAlignHip al(0, 2.0f, -5.0f, -5.0f, -5.0f, -1.0f, 0.15f, 0, 0, false, regionsOn, jobText);
		/* a request where the aligner answers one, on every tile but each third (the host form beside them in one launch) */
		std::vector<bool> marked(n);
		for (size_t i = 0; i < n; ++i) marked[i] = regionsOn && i % 3 != 2;
		std::vector<Held *> want, got;
		for (size_t i = 0; i < n; ++i) {
			want.push_back(new Held((int) cases[i].qry.size(), marked[i]));
			rung_by_rung(al, cases[i], *want[i]);
		}
		int climbed = 0, noted = 0, invalid = 0;
		for (size_t i = 0; i < n; ++i) {
			climbed += want[i]->rung >= 2 && want[i]->ret >= 0;
			invalid += want[i]->ret < 0;
			int r = 0;
			if (marked[i] && want[i]->ret >= 0 && Note::IsNote(want[i]->a.nmPerPosition, want[i]->a.nmPerPostionLength, r) && r > 0 && want[i]->rung >= 2) ++noted;
		}
		printf("  rung by rung: %d tiles resolved at rung 2 or later, %d never, %d notes with regions on tiles that climbed\n", climbed, invalid, noted);
		CHECK(climbed >= 4 && invalid >= 1);
		if (regionsOn) CHECK(noted >= 3);      /* tiles that climbed carry a note with regions */

		/* plain strings, one launch */
		long dev0 = 0, host0 = 0, dev1 = 0, host1 = 0;
		Convex::ConvexAlignHip::JobTextStats(dev0, host0);
		{
			std::vector<LadderTile> tiles;
			for (size_t i = 0; i < n; ++i) { got.push_back(new Held((int) cases[i].qry.size(), marked[i])); tiles.push_back(ladder_tile(cases[i], cases[i].ref.c_str(), cases[i].qry.c_str(), *got[i])); }
			al.AlignLadders(tiles.data(), (int) n);
			for (size_t i = 0; i < n; ++i) take(*got[i], tiles[i]);
		}
		Convex::ConvexAlignHip::JobTextStats(dev1, host1);
		compare("plain strings", cases, want, got, marked);
		if (regionsOn && jobText) CHECK(dev1 - dev0 >= 5);      /* the marked tiles with an alignment took their text from the device */
		else CHECK(dev1 == dev0);
		free_all(got);

		/* every reference a window placeholder: one launch per tile (a thread holds one window note at a time) */
		long wl0 = 0, wt0 = 0, wm0 = 0, wl1 = 0, wt1 = 0, wm1 = 0;
		Convex::ConvexAlignHip::WindowStats(wl0, wt0, wm0);
		for (size_t i = 0; i < n; ++i) {
			got.push_back(new Held((int) cases[i].qry.size(), marked[i]));
			int const length = (int) cases[i].ref.size() + 1;
			std::vector<char> buf((size_t) length + 100);
			Convex::DeviceWindows::Placeholder(buf.data(), (unsigned long long) starts[0] + (unsigned long long) cases[i].at, length);
			LadderTile t = ladder_tile(cases[i], buf.data(), cases[i].qry.c_str(), *got[i]);
			al.AlignLadders(&t, 1);
			take(*got[i], t);
			CHECK(buf[0] == 'x');      /* the launch decoded on the device: nothing wrote the caller's buffer */
		}
		Convex::ConvexAlignHip::WindowStats(wl1, wt1, wm1);
		compare("window placeholders", cases, want, got, marked);
		CHECK(wl1 - wl0 == (long) n && wt1 - wt0 == (long) n && wm1 == wm0);
		free_all(got);

		/* every query a read placeholder: one launch, two tiles per read, both strands */
		long rl0 = 0, rt0 = 0, rm0 = 0, rl1 = 0, rt1 = 0, rm1 = 0;
		Convex::ConvexAlignHip::ReadStats(rl0, rt0, rm0);
		std::vector<std::string> reads((n + 1) / 2);
		std::vector<int> startIn(n), flagOf(n);
		for (size_t i = 0; i < n; ++i) {
			std::string & r = reads[i / 2];
			for (int j = (int) (rnd() % 20); j > 0; --j) r.push_back("ACGT"[rnd() % 4]);
			startIn[i] = (int) r.size();
			flagOf[i] = (int) ((i >> 1) & 1) ^ (int) (i & 1);
			std::string q = cases[i].qry;
			if (flagOf[i]) { std::string rc; for (size_t j = q.size(); j > 0; --j) rc.push_back(comp(q[j - 1])); q = rc; }
			r += q;
		}
		std::vector<std::vector<char> > qbuf(n);
		{
			std::vector<LadderTile> tiles;
			for (size_t i = 0; i < n; ++i) {
				got.push_back(new Held((int) cases[i].qry.size(), marked[i]));
				int const H = (int) cases[i].qry.size();
				qbuf[i].assign((size_t) Convex::DeviceReads::BufferBytes(H), 0);
				Convex::DeviceReads::Placeholder(qbuf[i].data(), reads[i / 2].c_str(), (int) reads[i / 2].size(), startIn[i], H, flagOf[i] ? CVX_SEG_REVCOMP : 0);
				tiles.push_back(ladder_tile(cases[i], cases[i].ref.c_str(), qbuf[i].data(), *got[i]));
			}
			al.AlignLadders(tiles.data(), (int) n);
			for (size_t i = 0; i < n; ++i) take(*got[i], tiles[i]);
		}
		Convex::ConvexAlignHip::ReadStats(rl1, rt1, rm1);
		compare("read placeholders", cases, want, got, marked);
		CHECK(rl1 - rl0 == 1 && rt1 - rt0 == (long) n && rm1 == rm0);
		free_all(got);

		/* a mixed launch: plain and noted queries side by side, the last tile's reference a window placeholder -- everything is
		 * materialised on the host and travels as characters */
		Convex::ConvexAlignHip::WindowStats(wl0, wt0, wm0);
		Convex::ConvexAlignHip::ReadStats(rl0, rt0, rm0);
		{
			std::vector<LadderTile> tiles;
			int const length = (int) cases[n - 1].ref.size() + 1;
			std::vector<char> wbuf((size_t) length + 100);
			for (size_t i = 0; i < n; ++i) {
				got.push_back(new Held((int) cases[i].qry.size(), marked[i]));
				int const H = (int) cases[i].qry.size();
				bool const notedQry = i % 2 == 0;
				if (notedQry) Convex::DeviceReads::Placeholder(qbuf[i].data(), reads[i / 2].c_str(), (int) reads[i / 2].size(), startIn[i], H, flagOf[i] ? CVX_SEG_REVCOMP : 0);
				tiles.push_back(ladder_tile(cases[i], i == n - 1 ? wbuf.data() : cases[i].ref.c_str(), notedQry ? qbuf[i].data() : cases[i].qry.c_str(), *got[i]));
			}
			Convex::DeviceWindows::Placeholder(wbuf.data(), (unsigned long long) starts[0] + (unsigned long long) cases[n - 1].at, length);
			al.AlignLadders(tiles.data(), (int) n);
			for (size_t i = 0; i < n; ++i) take(*got[i], tiles[i]);
			CHECK(cases[n - 1].ref == wbuf.data());      /* the window was decoded into the caller's buffer */
		}
		Convex::ConvexAlignHip::WindowStats(wl1, wt1, wm1);
		Convex::ConvexAlignHip::ReadStats(rl1, rt1, rm1);
		compare("a mixed launch", cases, want, got, marked);
		CHECK(wm1 - wm0 == 1 && rm1 - rm0 == 1 && wl1 == wl0 && rl1 == rl0);
		free_all(got);
		free_all(want);
	}
	if (fails) { printf("ladder_stages_shim_test: %d failures\n", fails); return 1; }
	printf("ladder_stages_shim_test: ok\n");
	return 0;
}
