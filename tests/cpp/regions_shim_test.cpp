/*
 * regions_shim_test.cpp -- the drop-ins answering a request in Align::nmPerPosition with a note of the job's regions
 * (nm_regions_note.h; tests/test_gpu_shim_regions.py).
 *
 * Every case is aligned twice in ONE launch of Convex::ConvexAlignHip::AlignTiles on an aligner with regions: into an Align
 * whose profile buffer is allocated as the reference's caller allocates it (unmarked), and into one whose small buffer holds a
 * request (marked).  The unmarked one comes back with its profile, the marked one with a note whose regions must equal
 * cvx_nm_regions_host over that profile, and every other field of the two Aligns must be the same.  A case with more regions
 * than the small buffer holds has its buffer regrown; a case without a valid alignment keeps its request.  On an aligner
 * WITHOUT regions a request ends as the full profile: alignmentLength rows equal to the unmarked Align's, in a buffer at least that
 * long (the indels case has more columns than entries).  Then the same through Convex::SharedAligner on `devices` logical devices
 * (argv[1], with CVX_ALIAS_DEVICES set to it), with the binding announced -- and, under CVX_DEVICE_REGIONS=0, switched off.
 * Exit code 0 = everything as stated.
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

static unsigned lcg = 12345u;
static char base() { lcg = lcg * 1664525u + 1013904223u; return "ACGT"[(lcg >> 24) & 3]; }
static char other(char c) { return c == 'A' ? 'C' : c == 'C' ? 'G' : c == 'G' ? 'T' : 'A'; }

struct Case { std::string tag, ref, qry; std::vector<CorridorLine> lines; };

static Case make(char const * tag, int length, int first, int period, int run) {
	Case c;
	c.tag = tag;
	for (int i = 0; i < length; ++i) c.ref.push_back(base());
	c.qry = c.ref;
	/* `run` substituted bases every `period`: the alignment stays on the diagonal and every run is one low-identity region */
	if (period > 0) for (int a = first; a + run + 60 < length; a += period) for (int k = 0; k < run; ++k) c.qry[(size_t) (a + k)] = other(c.qry[(size_t) (a + k)]);
	return c;
}

static int const kSmallRows = 16;      /* the marked buffer: a header and eleven regions */

struct Held {
	Align a;
	std::vector<CorridorLine> lines;
	int ret;
	Held(Case const & c, bool marked) : ret(-2) {
		int const H = (int) c.qry.size(), w = 120;
		lines.resize((size_t) H);
		for (int y = 0; y < H; ++y) { lines[(size_t) y].offset = y - w / 2; lines[(size_t) y].length = w; lines[(size_t) y].offsetInMatrix = 0; }
		a.maxBufferLength = H * 4; a.maxMdBufferLength = H * 4;
		a.pBuffer1 = new char[a.maxBufferLength + 16]; a.pBuffer2 = new char[a.maxMdBufferLength + 16];
		a.pBuffer1[0] = a.pBuffer2[0] = '\0';
		a.nmPerPostionLength = marked ? kSmallRows : (H + 1) * 2;      /* (unmarked: src/AlignmentBuffer.cpp:277-278) */
		a.nmPerPosition = new PositionNM[a.nmPerPostionLength];
		if (marked) Note::Request(a.nmPerPosition);
	}
	~Held() { delete[] a.pBuffer1; delete[] a.pBuffer2; delete[] a.nmPerPosition; }
	Convex::ConvexAlignHip::Tile tile(Case const & c) {
		Convex::ConvexAlignHip::Tile t;
		memset(&t, 0, sizeof(t));
		t.corridor = lines.data(); t.corridorHeight = (int) lines.size();
		t.refSeq = c.ref.c_str(); t.qrySeq = c.qry.c_str(); t.result = &a;
		t.externalQStart = 0; t.externalQEnd = 0; t.ret = -2; t.failed = false;
		return t;
	}
private:
	Held(Held const &);
	Held & operator=(Held const &);
};

/* the regions of the profile an unmarked Align came back with, as detectMisalignment's finder would find them */
static std::vector<cvx_nm_region> regions_of_profile(Align const & a) {
	int64_t n = 0;
	int64_t const entries = a.alignmentLength < a.nmPerPostionLength ? a.alignmentLength : a.nmPerPostionLength;
	CHECK(cvx_nm_regions_host((int32_t const *) a.nmPerPosition, entries, a.alignmentLength, 0, 0, &n, 0) == CVX_OK);
	std::vector<cvx_nm_region> r((size_t) n + 1);
	if (n > 0) CHECK(cvx_nm_regions_host((int32_t const *) a.nmPerPosition, entries, a.alignmentLength, r.data(), n, &n, 0) == CVX_OK);
	r.resize((size_t) n);
	return r;
}

static bool same_fields(Align const & x, Align const & y) {
	return x.Score == y.Score && x.Identity == y.Identity && x.NM == y.NM && x.QStart == y.QStart && x.QEnd == y.QEnd &&
			x.alignmentLength == y.alignmentLength && x.PositionOffset == y.PositionOffset && x.cigarOpCount == y.cigarOpCount &&
			x.firstPosition.refPosition == y.firstPosition.refPosition && x.lastPosition.readPosition == y.lastPosition.readPosition &&
			strcmp(x.pBuffer1, y.pBuffer1) == 0 && strcmp(x.pBuffer2, y.pBuffer2) == 0;
}

/* plain and noted: the same case through an unmarked and a marked Align; -> regions in the note (-1: no valid alignment) */
static int check_pair(Case const & c, Held & plain, Held & noted, bool regionsOn) {
	CHECK(plain.ret == noted.ret);
	if (plain.ret < 0) {
		CHECK(Note::IsRequest(noted.a.nmPerPosition, noted.a.nmPerPostionLength) && noted.a.nmPerPostionLength == kSmallRows);      /* left for the retry */
		return -1;
	}
	CHECK(same_fields(plain.a, noted.a));
	CHECK(!Note::Wanted(plain.a.nmPerPosition, plain.a.nmPerPostionLength));      /* an unmarked buffer gets its profile, flag or no flag */
	std::vector<cvx_nm_region> const want = regions_of_profile(plain.a);
	if (!regionsOn) {
		/* no regions on this path: the request ended as the FULL profile -- every row the finder's loop scans, alignmentLength of
		 * them (insertion columns and the first 16 positions have no entry, so that is more than the entries): the rows of the
		 * unmarked Align's profile, zeros behind the entries included (its buffer is 2 * (H + 1) zeroed rows) */
		CHECK(!Note::Wanted(noted.a.nmPerPosition, noted.a.nmPerPostionLength));
		CHECK(plain.a.nmPerPostionLength >= plain.a.alignmentLength);
		CHECK(noted.a.nmPerPostionLength >= noted.a.alignmentLength);
		if (noted.a.nmPerPostionLength >= noted.a.alignmentLength && plain.a.nmPerPostionLength >= plain.a.alignmentLength)
			CHECK(memcmp(plain.a.nmPerPosition, noted.a.nmPerPosition, (size_t) plain.a.alignmentLength * sizeof(PositionNM)) == 0);
		printf("%s: ret %d, the request ended as a profile: alignmentLength %d in %d rows\n", c.tag.c_str(), noted.ret, noted.a.alignmentLength, noted.a.nmPerPostionLength);
		std::vector<cvx_nm_region> const got = regions_of_profile(noted.a);
		CHECK(got.size() == want.size() && (want.empty() || memcmp(got.data(), want.data(), want.size() * sizeof(cvx_nm_region)) == 0));
		return (int) want.size();
	}
	int n = -1;
	CHECK(Note::IsNote(noted.a.nmPerPosition, noted.a.nmPerPostionLength, n));
	CHECK(n == (int) want.size());
	for (int i = 0; i < n && i < (int) want.size(); ++i) {
		Note::Region const g = Note::At(noted.a.nmPerPosition, i);
		CHECK(memcmp(&g, &want[(size_t) i], sizeof(g)) == 0);
	}
	if (Note::RowsFor(n) > kSmallRows) CHECK(noted.a.nmPerPostionLength >= Note::RowsFor(n));      /* regrown */
	else CHECK(noted.a.nmPerPostionLength == kSmallRows);
	printf("%s: ret %d, %d regions, note in %d rows\n", c.tag.c_str(), noted.ret, n, noted.a.nmPerPostionLength);
	return n;
}

static void through_align_tiles(std::vector<Case> const & cases, bool regionsOn, std::vector<int> & counts) {
	Convex::ConvexAlignHip al(0, 2.0f, -5.0f, -5.0f, -5.0f, -1.0f, 0.15f, 0, 0, false, regionsOn);
	CHECK(al.NmRegions() == regionsOn);
	std::vector<Held *> held;
	std::vector<Convex::ConvexAlignHip::Tile> tiles;
	for (Case const & c : cases) for (int marked = 0; marked < 2; ++marked) {
		held.push_back(new Held(c, marked != 0));
		tiles.push_back(held.back()->tile(c));
	}
	al.AlignTiles(tiles.data(), (int) tiles.size());      /* marked and unmarked buffers in one launch */
	int total = 0, regrown = 0, invalid = 0;
	counts.clear();
	for (size_t k = 0; k < cases.size(); ++k) {
		held[2 * k]->ret = tiles[2 * k].ret; held[2 * k + 1]->ret = tiles[2 * k + 1].ret;
		CHECK(!tiles[2 * k].failed && !tiles[2 * k + 1].failed);
		int const n = check_pair(cases[k], *held[2 * k], *held[2 * k + 1], regionsOn);
		counts.push_back(n);
		if (n < 0) { ++invalid; continue; }
		total += n;
		if (regionsOn && Note::RowsFor(n) > kSmallRows) ++regrown;
	}
	printf("AlignTiles (%s): %d regions in %zu cases, %d notes regrown, %d without an alignment\n", regionsOn ? "regions" : "plain", total, cases.size(), regrown, invalid);
	CHECK(total >= 10 && invalid >= 1);
	if (regionsOn) CHECK(regrown >= 1);
	/* a second alignment into the Aligns that hold notes now: the note is answered again, not taken for a profile */
	if (regionsOn) {
		for (size_t k = 0; k < cases.size(); ++k) tiles[2 * k + 1] = held[2 * k + 1]->tile(cases[k]);
		al.AlignTiles(tiles.data(), (int) tiles.size());
		for (size_t k = 0; k < cases.size(); ++k) {
			held[2 * k]->ret = tiles[2 * k].ret; held[2 * k + 1]->ret = tiles[2 * k + 1].ret;
			if (counts[k] >= 0) CHECK(check_pair(cases[k], *held[2 * k], *held[2 * k + 1], true) == counts[k]);
		}
	}
	for (Held * h : held) delete h;
}

static void through_shared(std::vector<Case> const & cases, int devices, bool regionsOn, std::vector<int> const & counts) {
	std::vector<Convex::SharedAligner *> sh;
	for (int d = 0; d < devices; ++d) sh.push_back(new Convex::SharedAligner(0, 2.0f, -5.0f, -5.0f, -5.0f, -1.0f, 0.15f, d, false));
	int total = 0;
	for (int d = 0; d < devices; ++d) for (size_t k = 0; k < cases.size(); ++k) {
		Case const & c = cases[k];
		Held plain(c, false), noted(c, true);
		plain.ret = sh[(size_t) d]->SingleAlign(0, plain.lines.data(), (int) plain.lines.size(), c.ref.c_str(), c.qry.c_str(), plain.a, 0, 0, 0);
		noted.ret = sh[(size_t) d]->SingleAlign(0, noted.lines.data(), (int) noted.lines.size(), c.ref.c_str(), c.qry.c_str(), noted.a, 0, 0, 0);
		int const n = check_pair(c, plain, noted, regionsOn);
		CHECK(n == counts[k]);
		if (n > 0) total += n;
	}
	printf("SharedAligner on %d logical device(s) (%s): %d regions\n", devices, regionsOn ? "regions" : "plain", total);
	CHECK(total >= 10 * devices);
	for (Convex::SharedAligner * s : sh) delete s;
}

int main(int argc, char ** argv) {
	int const devices = argc > 1 ? atoi(argv[1]) : 1;
	std::vector<Case> cases;
	cases.push_back(make("one-stretch", 1500, 700, 100000, 40));
	cases.push_back(make("bursts", 3000, 90, 110, 24));          /* some 26 regions: more than the stage keeps, more than the small buffer holds */
	cases.push_back(make("few-bursts", 900, 200, 300, 24));
	cases.push_back(make("clean", 700, 0, 0, 0));
	cases.push_back(make("short", 40, 0, 0, 0));
	{
		/* indels: a base inserted into the read every 25 and a reference base skipped every 90 -- about 990 entries in an alignment of
		 * about 1 050 columns, so a buffer grown by the entry count alone (16 rows doubled to 1 024) is shorter than what the finder scans */
		Case c = make("indels", 1000, 300, 330, 24);
		std::string q;
		for (size_t i = 0; i < c.qry.size(); ++i) {
			if (i % 90 == 45) continue;
			q.push_back(c.qry[i]);
			if (i % 25 == 12) q.push_back(other(c.qry[i]));
		}
		c.qry = q;
		cases.push_back(c);
	}
	Case junk;
	junk.tag = "no-alignment"; junk.ref = std::string(200, 'A'); junk.qry = std::string(180, 'C');
	cases.push_back(junk);

	std::vector<int> counts, plainCounts;
	through_align_tiles(cases, true, counts);
	through_align_tiles(cases, false, plainCounts);
	CHECK(counts == plainCounts);

	/* SharedAligner: plain handles until a binding announces itself */
	CHECK(!Convex::DeviceRegions::Enabled());
	Convex::DeviceRegions::Announce();
	char const * const off = getenv("CVX_DEVICE_REGIONS");
	bool const on = !(off && atoi(off) == 0);
	CHECK(Convex::DeviceRegions::Enabled() == on);
	through_shared(cases, devices, on, counts);
	if (fails) { printf("regions_shim_test: %d checks failed\n", fails); return 1; }
	printf("regions_shim_test: ok (%s)\n", on ? "regions" : "profile");
	return 0;
}
