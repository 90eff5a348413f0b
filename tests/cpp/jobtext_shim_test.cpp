/*
 * jobtext_shim_test.cpp -- the drop-ins taking CIGAR and MD of a tile from the launch's device-made text (CVX_CREATE_JOB_TEXT,
 * ConvexAlignHip::FinishJobText; tests/test_gpu_shim_jobtext.py) instead of walking its ops on the host.
 *
 * Every case is aligned into an Align whose small nmPerPosition holds a request (answered with a note: the tile FinishJobText
 * takes) and into one with the reference's own profile buffer (the host form, as always), both in ONE launch of
 * Convex::ConvexAlignHip::AlignTiles -- once on an aligner with regions and job text, once on one with regions alone, whose
 * Finish formats every tile on the host.  Every Align field, both strings, the note and the profile of the two runs must be the
 * same, with external clips of 0, 7 and 4 999.  A pBuffer2 too small for the MD is regrown in both, a CIGAR beyond
 * maxBufferLength is the tile's hard error in both.  Then the same through Convex::SharedAligner on `devices` logical devices
 * (argv[1], with CVX_ALIAS_DEVICES set to it) with the binding announced: CVX_JOB_TEXT=1 takes the marked tiles' text from the
 * device, CVX_JOB_TEXT=0 (or unset) none.  Exit code 0 = everything as stated.
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "convex_align_hip.h"
#include "batching_aligner.h"
#include "nm_regions_note.h"

typedef Convex::NmRegionsNote Note;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

static unsigned lcg = 4321u;
static char base() { lcg = lcg * 1664525u + 1013904223u; return "ACGT"[(lcg >> 24) & 3]; }
static char other(char c) { return c == 'A' ? 'C' : c == 'C' ? 'G' : c == 'G' ? 'T' : 'A'; }

struct Case {
	std::string tag, ref, qry;
	int extStart, extEnd;
	int cigarCap, mdCap;      /* 0: H * 4, as the reference's caller sizes them */
};

static Case make(char const * tag, int length, int first, int period, int run, int extStart, int extEnd) {
	Case c;
	c.tag = tag; c.extStart = extStart; c.extEnd = extEnd; c.cigarCap = 0; c.mdCap = 0;
	for (int i = 0; i < length; ++i) c.ref.push_back(base());
	c.qry = c.ref;
	if (period > 0) for (int a = first; a + run + 60 < length; a += period) for (int k = 0; k < run; ++k) c.qry[(size_t) (a + k)] = other(c.qry[(size_t) (a + k)]);
	return c;
}

/* a base inserted into the read every 25 and a reference base skipped every 90: a CIGAR of many pieces, an MD with deletions */
static void indels(Case & c) {
	std::string q;
	for (size_t i = 0; i < c.qry.size(); ++i) {
		if (i % 90 == 45) continue;
		q.push_back(c.qry[i]);
		if (i % 25 == 12) q.push_back(other(c.qry[i]));
	}
	c.qry = q;
}

static int const kSmallRows = 16;

struct Held {
	Align a;
	std::vector<CorridorLine> lines;
	int ret;
	bool failed;
	Held(Case const & c, bool marked) : ret(-2), failed(false) {
		int const H = (int) c.qry.size(), w = 120;
		lines.resize((size_t) H);
		for (int y = 0; y < H; ++y) { lines[(size_t) y].offset = y - w / 2; lines[(size_t) y].length = w; lines[(size_t) y].offsetInMatrix = 0; }
		a.maxBufferLength = c.cigarCap ? c.cigarCap : H * 4; a.maxMdBufferLength = c.mdCap ? c.mdCap : H * 4;
		a.pBuffer1 = new char[a.maxBufferLength + 16]; a.pBuffer2 = new char[a.maxMdBufferLength + 16];
		a.pBuffer1[0] = a.pBuffer2[0] = '\0';
		a.nmPerPostionLength = marked ? kSmallRows : (H + 1) * 2;
		a.nmPerPosition = new PositionNM[a.nmPerPostionLength];
		a.svType = 77; a.cigarOpCount = 55;      /* (overwritten by a default handle) */
		if (marked) Note::Request(a.nmPerPosition);
	}
	~Held() { delete[] a.pBuffer1; delete[] a.pBuffer2; delete[] a.nmPerPosition; }
	Convex::ConvexAlignHip::Tile tile(Case const & c) {
		Convex::ConvexAlignHip::Tile t;
		memset(&t, 0, sizeof(t));
		t.corridor = lines.data(); t.corridorHeight = (int) lines.size();
		t.refSeq = c.ref.c_str(); t.qrySeq = c.qry.c_str(); t.result = &a;
		t.externalQStart = c.extStart; t.externalQEnd = c.extEnd; t.ret = -2; t.failed = false;
		return t;
	}
private:
	Held(Held const &);
	Held & operator=(Held const &);
};

/* every Align field, both strings, and what nmPerPosition holds: the note's regions, or the profile's alignmentLength rows */
static bool same_align(Held const & x, Held const & y, bool marked) {
	Align const & p = x.a, & q = y.a;
	if (x.ret != y.ret || x.failed != y.failed) return false;
	if (x.failed) return true;      /* a tile's hard error: the caller drops the alignment */
	if (x.ret < 0) return p.Score == q.Score && (!marked || (Note::IsRequest(p.nmPerPosition, p.nmPerPostionLength) && Note::IsRequest(q.nmPerPosition, q.nmPerPostionLength)));
	bool ok = memcmp(&p.Score, &q.Score, sizeof(float)) == 0 && memcmp(&p.Identity, &q.Identity, sizeof(float)) == 0 && p.NM == q.NM && p.MQ == q.MQ &&
			p.QStart == q.QStart && p.QEnd == q.QEnd && p.alignmentLength == q.alignmentLength && p.PositionOffset == q.PositionOffset &&
			p.cigarOpCount == q.cigarOpCount && p.svType == q.svType && p.maxBufferLength == q.maxBufferLength && p.maxMdBufferLength == q.maxMdBufferLength &&
			p.firstPosition.refPosition == q.firstPosition.refPosition && p.firstPosition.readPosition == q.firstPosition.readPosition &&
			p.lastPosition.refPosition == q.lastPosition.refPosition && p.lastPosition.readPosition == q.lastPosition.readPosition &&
			p.nmPerPostionLength == q.nmPerPostionLength && strcmp(p.pBuffer1, q.pBuffer1) == 0 && strcmp(p.pBuffer2, q.pBuffer2) == 0;
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

/* held[2 k] unmarked, held[2 k + 1] marked */
static void through_align_tiles(std::vector<Case> const & cases, bool jobText, std::vector<Held *> & held) {
	Convex::ConvexAlignHip al(0, 2.0f, -5.0f, -5.0f, -5.0f, -1.0f, 0.15f, 0, 0, false, true, jobText);
	CHECK(al.NmRegions() && al.JobTextOn() == jobText);
	std::vector<Convex::ConvexAlignHip::Tile> tiles;
	for (Case const & c : cases) for (int marked = 0; marked < 2; ++marked) {
		held.push_back(new Held(c, marked != 0));
		tiles.push_back(held.back()->tile(c));
	}
	long dev0 = 0, host0 = 0, dev1 = 0, host1 = 0;
	Convex::ConvexAlignHip::JobTextStats(dev0, host0);
	al.AlignTiles(tiles.data(), (int) tiles.size());      /* requests and plain buffers in one launch */
	Convex::ConvexAlignHip::JobTextStats(dev1, host1);
	int valid = 0;
	for (size_t i = 0; i < tiles.size(); ++i) { held[i]->ret = tiles[i].ret; held[i]->failed = tiles[i].failed; valid += (tiles[i].ret >= 0 && !tiles[i].failed && (i & 1)) ? 1 : 0; }
	/* the marked tiles with an alignment took their text from the device, everything else was formatted on the host; a tile
	 * whose CIGAR does not fit counts where it was tried */
	printf("AlignTiles (%s): %ld from the device, %ld on the host\n", jobText ? "job text" : "host form", dev1 - dev0, host1 - host0);
	if (jobText) CHECK(dev1 - dev0 >= valid && dev1 - dev0 <= (long) cases.size() && valid >= 5);
	else CHECK(dev1 == dev0);
	CHECK((dev1 - dev0) + (host1 - host0) <= (long) tiles.size());
}

static void through_shared(std::vector<Case> const & cases, int devices, bool ctorFlag, bool expectDevice, std::vector<Held *> const & want) {
	long dev0 = 0, host0 = 0, dev1 = 0, host1 = 0;
	Convex::ConvexAlignHip::JobTextStats(dev0, host0);
	std::vector<Convex::SharedAligner *> sh;
	for (int d = 0; d < devices; ++d) sh.push_back(new Convex::SharedAligner(0, 2.0f, -5.0f, -5.0f, -5.0f, -1.0f, 0.15f, d, false, ctorFlag));
	int same = 0;
	for (int d = 0; d < devices; ++d) for (size_t k = 0; k < cases.size(); ++k) for (int marked = 0; marked < 2; ++marked) {
		Case const & c = cases[k];
		Held h(c, marked != 0);
		try {
			h.ret = sh[(size_t) d]->SingleAlign(0, h.lines.data(), (int) h.lines.size(), c.ref.c_str(), c.qry.c_str(), h.a, c.extStart, c.extEnd, 0);
		} catch (int) {
			h.failed = true; h.ret = -1;      /* the reference's caller catches it and drops the alignment */
		}
		Held const & w = *want[2 * k + (size_t) marked];
		if (w.failed) { CHECK(h.failed); ++same; continue; }
		bool const ok = same_align(h, w, marked != 0);
		CHECK(ok);
		if (!ok) printf("  %s (%s) differs on logical device %d\n", c.tag.c_str(), marked ? "request" : "profile", d);
		same += ok;
	}
	for (Convex::SharedAligner * s : sh) delete s;
	Convex::ConvexAlignHip::JobTextStats(dev1, host1);
	printf("SharedAligner on %d logical device(s): %d Aligns as the host form leaves them; %ld from the device, %ld on the host\n", devices, same, dev1 - dev0, host1 - host0);
	if (expectDevice) CHECK(dev1 - dev0 >= 5 * devices);
	else CHECK(dev1 == dev0);
}

int main(int argc, char ** argv) {
	int const devices = argc > 1 ? atoi(argv[1]) : 1;
	bool const ctorFlag = argc > 2 && atoi(argv[2]) != 0;
	std::vector<Case> cases;
	cases.push_back(make("one-stretch", 1500, 700, 100000, 40, 0, 0));
	cases.push_back(make("bursts", 3000, 90, 110, 24, 7, 0));
	cases.push_back(make("few-bursts", 900, 200, 300, 24, 0, 7));
	cases.push_back(make("clean", 700, 0, 0, 0, 4999, 1));
	cases.push_back(make("short", 40, 0, 0, 0, 1, 4999));
	{
		Case c = make("indels", 1000, 300, 330, 24, 12, 34);
		indels(c);
		cases.push_back(c);
	}
	{
		Case c = make("small-md-buffer", 1000, 300, 330, 24, 0, 3);      /* checkMdBufferLength: regrown with new[] */
		indels(c);
		c.mdCap = 8;
		cases.push_back(c);
	}
	{
		Case c = make("cigar-too-long", 1000, 300, 330, 24, 5, 0);      /* "CIGAR/MD buffer not long enough": this tile's hard error */
		indels(c);
		c.cigarCap = 24;
		cases.push_back(c);
	}
	{
		Case c = make("cigar-fits-exactly", 700, 0, 0, 0, 0, 0);        /* "700M": four characters in a buffer of four and of five */
		c.cigarCap = 4;
		cases.push_back(c);
		c.tag = "cigar-and-nul-fit"; c.cigarCap = 5;
		cases.push_back(c);
	}
	Case junk = make("no-alignment", 10, 0, 0, 0, 3, 3);
	junk.ref = std::string(200, 'A'); junk.qry = std::string(180, 'C');
	cases.push_back(junk);

	std::vector<Held *> host, dev;
	through_align_tiles(cases, false, host);
	through_align_tiles(cases, true, dev);
	int regrown = 0, hard = 0, invalid = 0;
	for (size_t k = 0; k < cases.size(); ++k) for (int marked = 0; marked < 2; ++marked) {
		Held const & h = *host[2 * k + (size_t) marked], & d = *dev[2 * k + (size_t) marked];
		bool const ok = same_align(d, h, marked != 0);
		CHECK(ok);
		printf("%s (%s): ret %d%s, CIGAR %.24s%s MD %.16s%s -- %s\n", cases[k].tag.c_str(), marked ? "request" : "profile", d.ret, d.failed ? " (hard error)" : "",
				d.failed || d.ret < 0 ? "" : d.a.pBuffer1, !d.failed && d.ret >= 0 && strlen(d.a.pBuffer1) > 24 ? "..." : "", d.failed || d.ret < 0 ? "" : d.a.pBuffer2,
				!d.failed && d.ret >= 0 && strlen(d.a.pBuffer2) > 16 ? "..." : "", ok ? "same" : "DIFFERENT");
		if (marked) {
			regrown += (!d.failed && cases[k].mdCap && d.a.maxMdBufferLength > cases[k].mdCap) ? 1 : 0;
			hard += d.failed ? 1 : 0;
			invalid += (!d.failed && d.ret < 0) ? 1 : 0;
		}
	}
	CHECK(regrown >= 1 && hard >= 1 && invalid >= 1);
	/* the external clips reached the CIGAR of the device-made text */
	CHECK(strncmp(dev[2 * 3 + 1]->a.pBuffer1, "4999S", 5) == 0 && dev[2 * 3 + 1]->a.QStart == 4999 && dev[2 * 3 + 1]->a.QEnd == 1);
	CHECK(dev[2 * 1 + 1]->a.svType != 77 && dev[2 * 1 + 1]->a.cigarOpCount != 55);

	Convex::DeviceRegions::Announce();
	CHECK(Convex::DeviceRegions::Enabled());
	char const * const sw = getenv("CVX_JOB_TEXT");
	bool const on = sw && atoi(sw) != 0;
	CHECK(Convex::DeviceRegions::JobText() == on);
	through_shared(cases, devices, ctorFlag, on || ctorFlag, host);
	for (Held * h : host) delete h;
	for (Held * h : dev) delete h;
	if (fails) { printf("jobtext_shim_test: %d checks failed\n", fails); return 1; }
	printf("jobtext_shim_test: ok (%s)\n", on || ctorFlag ? "device text" : "host form");
	return 0;
}
