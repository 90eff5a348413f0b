/*
 * invchecks_shim_test.cpp -- the drop-ins answering a request in Align::nmPerPosition with the checks form of the note
 * (nm_regions_note.h; Convex::DeviceInvChecks, convex_align_hip.h; tests/test_gpu_invchecks_shim.py).
 *
 * One genome of one contig, and six tiles whose reference is a window of it (a DeviceWindows placeholder) and whose Align holds a
 * request in the buffer the allocation binding allocates -- the smallest shapes that reach every branch:
 *   bursts    3 000 bases, a 24-base substituted run every 110: 26 regions, whose checks note (71 rows) regrows the buffer
 *   edges     600 bases, a noisy stretch at either end and a run in the middle: one region's midpoint on the read lies below 50,
 *             one beyond H - 50 (both CVX_CHECK_NO_READ)
 *   short     nine substitutions three bases apart: one region of length <= 10 (CVX_CHECK_TOO_SHORT)
 *   start     the window at base 0 of a genome WITHOUT a leading spacer, a run at base 100: the check window's position
 *             (midpoint - 250 - length / 2) falls below zero and does not decode (CVX_CHECK_NO_WINDOW).  (A region inside a
 *             contig cannot reach the other failure, position >= GetConcatRefLen(): the position lies below the midpoint.  With
 *             the 1 000-nibble spacer ngmlr puts in front of its first contig neither can happen.)
 *   clean     no region
 *   invalid   no valid alignment: the request must stay
 * Every launch is made in stages, as the dispatcher makes it (Prepare in the caller's context right behind the placeholder -- a
 * thread holds one window note at a time -- then Submit, Wait, WindowRefs, Regions, Finish), and every tile again alone through
 * AlignTiles / AlignLadders and through Convex::SharedAligner.  Every note's regions must equal cvx_job_regions', every check
 * record cvx_inv_checks_host's over the same regions and results, byte for byte.  The same tiles as ONE ladder job; on an aligner
 * with jobText; a launch with one plain reference string (materialised on the host: regions-only notes, counted); an aligner
 * without invChecks (today's notes, byte for byte).  Under CVX_DEVICE_INV_CHECKS=0 every note is the regions-only form.
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
typedef Convex::ConvexAlignHip Aligner;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

static uint32_t rs = 90210;
static uint32_t rnd() { rs = rs * 1664525u + 1013904223u; return rs >> 8; }
static char other(char c) { return c == 'A' ? 'C' : c == 'C' ? 'G' : c == 'G' ? 'T' : 'A'; }

/* the genome as the aligners see it: cvx_genome_encode's bytes without the leading spacer, so that the contig starts at nibble 0 */
static std::string genome;
static std::vector<uint8_t> bin;
static uint64_t nNibbles = 0, starts[2] = { 0, 0 };
static int32_t nStarts = 0;

struct Case { std::string tag; int at; std::string ref, qry; };

static Case window_case(char const * tag, int at, int W, std::vector<int> const & muts) {
	Case c;
	c.tag = tag; c.at = at;
	c.ref = genome.substr((size_t) at, (size_t) W);
	c.qry = c.ref;
	for (int m : muts) c.qry[(size_t) m] = other(c.qry[(size_t) m]);
	return c;
}

static int const kRequestRows = 44;      /* Note::RowsFor(32): what nm_regions_alloc_binding.inc allocates */

struct Held {
	Align a;
	std::vector<CorridorLine> lines;
	std::vector<char> window;      /* the placeholder's buffer (window length + 100 bytes, as the binding allocates it) */
	int ret;
	bool failed;
	explicit Held(Case const & c) : ret(-2), failed(false) {
		int const H = (int) c.qry.size(), w = 120;
		lines.resize((size_t) H);
		for (int y = 0; y < H; ++y) { lines[(size_t) y].offset = y - w / 2; lines[(size_t) y].length = w; lines[(size_t) y].offsetInMatrix = 0; }
		a.maxBufferLength = H * 4 + 64; a.maxMdBufferLength = H * 4 + 64;
		a.pBuffer1 = new char[a.maxBufferLength + 16]; a.pBuffer2 = new char[a.maxMdBufferLength + 16];
		a.pBuffer1[0] = a.pBuffer2[0] = '\0';
		a.svType = 0; a.cigarOpCount = 0;
		a.nmPerPostionLength = kRequestRows;
		a.nmPerPosition = new PositionNM[a.nmPerPostionLength];
		Note::Request(a.nmPerPosition);
		window.assign(c.ref.size() + 1 + 100, 0);
	}
	~Held() { delete[] a.pBuffer1; delete[] a.pBuffer2; delete[] a.nmPerPosition; }
	/* the reference of the tile: the placeholder of its window, or the characters themselves */
	char const * reference(Case const & c, bool asWindow) {
		if (!asWindow) return c.ref.c_str();
		Convex::DeviceWindows::Placeholder(window.data(), (unsigned long long) starts[0] + (unsigned long long) c.at, (int) c.ref.size() + 1);
		return window.data();
	}
private:
	Held(Held const &);
	Held & operator=(Held const &);
};

static std::vector<Held *> hold(std::vector<Case> const & cases) {
	std::vector<Held *> v;
	for (Case const & c : cases) v.push_back(new Held(c));
	return v;
}
static void free_all(std::vector<Held *> & v) { for (Held * h : v) delete h; v.clear(); }

/* what a launch brought for one tile, copied out of the job's memory before Release */
struct Brought { std::vector<cvx_nm_region> regions; int32_t positionOffset; bool checks; };

struct Totals { int scored, tooShort, noRead, noWindow, checksNotes, plainNotes, regrown, requestsKept; Totals() { memset(this, 0, sizeof(*this)); } };

/* the note in h against the regions its job brought and -- withChecks -- cvx_inv_checks_host over them */
static void check_note(Case const & c, Held & h, Brought const & b, bool withChecks, Totals & t) {
	CHECK(!h.failed);
	if (h.ret < 0) {
		CHECK(Note::IsRequest(h.a.nmPerPosition, h.a.nmPerPostionLength) && h.a.nmPerPostionLength == kRequestRows);      /* left for the retry */
		t.requestsKept += 1;
		return;
	}
	int const want = (int) b.regions.size();
	int n = -1;
	if (!withChecks) {
		CHECK(Note::IsNote(h.a.nmPerPosition, h.a.nmPerPostionLength, n) && n == want);
		int m = -1;
		CHECK(!Note::IsChecksNote(h.a.nmPerPosition, h.a.nmPerPostionLength, m));
		if (n != want) return;
		/* today's note, byte for byte */
		std::vector<PositionNM> fresh((size_t) Note::RowsFor(want));
		CHECK(Note::Write(fresh.data(), (int) fresh.size(), reinterpret_cast<Note::Region const *>(b.regions.data()), want));
		CHECK(memcmp(fresh.data(), h.a.nmPerPosition, fresh.size() * sizeof(PositionNM)) == 0);
		CHECK(h.a.nmPerPostionLength == (Note::RowsFor(want) > kRequestRows ? 2 * kRequestRows : kRequestRows));
		t.plainNotes += 1;
		return;
	}
	CHECK(Note::IsChecksNote(h.a.nmPerPosition, h.a.nmPerPostionLength, n) && n == want);
	int m = -1;
	CHECK(!Note::IsNote(h.a.nmPerPosition, h.a.nmPerPostionLength, m));
	if (n != want) return;
	CHECK(h.a.PositionOffset == b.positionOffset);
	/* the host rule over the same regions and results */
	std::vector<cvx_inv_check> host((size_t) want + 1);
	char const * qrys[1] = { c.qry.c_str() };
	int32_t const qryLen[1] = { (int32_t) c.qry.size() };
	uint64_t const refPosition[1] = { starts[0] + (uint64_t) c.at };
	int32_t const offset[1] = { h.a.PositionOffset };
	uint64_t const regionOff[2] = { 0, (uint64_t) want };
	CHECK(cvx_inv_checks_host(bin.data(), nNibbles, starts, nStarts, 1, qrys, qryLen, refPosition, offset, regionOff, b.regions.data(), host.data()) == CVX_OK);
	for (int i = 0; i < want; ++i) {
		Note::Region const r = Note::At(h.a.nmPerPosition, i);
		Note::Check const k = Note::CheckAt(h.a.nmPerPosition, want, i);
		CHECK(memcmp(&r, &b.regions[(size_t) i], sizeof(r)) == 0);
		bool const same = memcmp(&k, &host[(size_t) i], sizeof(k)) == 0;
		if (!same) printf("  %s region %d: note (%g, %g, %d, %d), host (%g, %g, %d, %d)\n", c.tag.c_str(), i, k.scoreFwd, k.scoreRev, k.status, k.windowChars,
				host[(size_t) i].score_fwd, host[(size_t) i].score_rev, host[(size_t) i].status, host[(size_t) i].window_chars);
		CHECK(same);
		t.scored += k.status == CVX_CHECK_SCORED; t.tooShort += k.status == CVX_CHECK_TOO_SHORT;
		t.noRead += k.status == CVX_CHECK_NO_READ; t.noWindow += k.status == CVX_CHECK_NO_WINDOW;
	}
	if (Note::RowsForChecks(want) > kRequestRows) { CHECK(h.a.nmPerPostionLength == 2 * kRequestRows && Note::RowsForChecks(want) <= 2 * kRequestRows); t.regrown += 1; }
	else CHECK(h.a.nmPerPostionLength == kRequestRows);
	t.checksNotes += 1;
}

static void bring(Aligner::JobRegions const & jr, cvx_result const * res, size_t n, std::vector<Brought> & out) {
	out.resize(n);
	for (size_t i = 0; i < n; ++i) {
		out[i].regions.assign(jr.regions + jr.off[i], jr.regions + jr.off[i + 1]);
		out[i].positionOffset = res[i].ref_position;
		out[i].checks = jr.checks != 0;
	}
}

/* one launch of all cases in stages; plainAt: the tile whose reference travels as characters (-1: none) */
static bool staged_tiles(Aligner & al, std::vector<Case> const & cases, std::vector<Held *> & held, int plainAt, std::vector<Brought> & out) {
	size_t const n = cases.size();
	std::vector<Aligner::Tile> tiles(n);
	for (size_t i = 0; i < n; ++i) {
		Aligner::Tile & t = tiles[i];
		memset(&t, 0, sizeof(t));
		t.corridor = held[i]->lines.data(); t.corridorHeight = (int) held[i]->lines.size();
		t.refSeq = held[i]->reference(cases[i], (int) i != plainAt); t.qrySeq = cases[i].qry.c_str(); t.result = &held[i]->a;
		t.ret = -2;
		Aligner::Prepare(t, false);      /* in the "caller's context": the window note is this tile's until the next placeholder */
	}
	cvx_job const job = al.Submit(tiles.data(), (int) n);
	cvx_result const * res = 0;
	uint32_t const * ops = 0;
	Aligner::JobRegions jr;
	Aligner::JobTextView jx;
	bool haveChecks = false;
	try {
		al.Wait(job, &res, &ops);
		std::vector<Aligner::Tile *> ptrs(n);
		for (size_t i = 0; i < n; ++i) ptrs[i] = &tiles[i];
		(void) al.WindowRefs(job, ptrs.data(), (int) n);
		CHECK(al.Regions(job, jr));
		bool const haveTexts = al.JobTexts(job, jx);
		haveChecks = jr.checks != 0;
		bring(jr, res, n, out);
		for (size_t i = 0; i < n; ++i) {
			try { al.Finish(tiles[i], res[i], ops, &jr, (int) i, haveTexts ? &jx : 0); } catch (...) { tiles[i].failed = true; tiles[i].ret = -1; }
			held[i]->ret = tiles[i].ret; held[i]->failed = tiles[i].failed;
		}
	} catch (...) {
		al.Release(job);
		throw;
	}
	al.Release(job);
	return haveChecks;
}

static cvx_ladder ladder_of() { cvx_ladder l; memset(&l, 0, sizeof(l)); l.corridor = 120; return l; }

/* the same tiles as ONE ladder job, in stages */
static bool staged_ladders(Aligner & al, std::vector<Case> const & cases, std::vector<Held *> & held, std::vector<Brought> & out) {
	size_t const n = cases.size();
	std::vector<Aligner::LadderTile> tiles(n);
	for (size_t i = 0; i < n; ++i) {
		Aligner::LadderTile & t = tiles[i];
		memset(&t, 0, sizeof(t));
		t.refSeq = held[i]->reference(cases[i], true); t.qrySeq = cases[i].qry.c_str(); t.result = &held[i]->a;
		t.ladder = ladder_of();
		t.ret = -2;
		Aligner::PrepareLadder(t);
	}
	cvx_job const job = al.SubmitLadders(tiles.data(), (int) n);
	cvx_result const * res = 0;
	uint32_t const * ops = 0;
	cvx_ladder_result const * lr = 0;
	Aligner::JobRegions jr;
	Aligner::JobTextView jx;
	bool haveChecks = false;
	try {
		al.Wait(job, &res, &ops);      /* (blocking in it advances the job waited for, as in AlignLadders) */
		al.Ladders(job, &lr);
		std::vector<Aligner::Tile *> ptrs(n);
		for (size_t i = 0; i < n; ++i) ptrs[i] = &tiles[i].resolved;
		(void) al.WindowRefs(job, ptrs.data(), (int) n);
		CHECK(al.Regions(job, jr));
		bool const haveTexts = al.JobTexts(job, jx);
		haveChecks = jr.checks != 0;
		bring(jr, res, n, out);
		for (size_t i = 0; i < n; ++i) {
			try { al.FinishLadder(tiles[i], res[i], ops, lr[i], &jr, (int) i, haveTexts ? &jx : 0); } catch (...) { tiles[i].failed = true; tiles[i].ret = -1; }
			held[i]->ret = tiles[i].ret; held[i]->failed = tiles[i].failed;
		}
	} catch (...) {
		al.Release(job);
		throw;
	}
	al.Release(job);
	return haveChecks;
}

static bool same_note(Held const & x, Held const & y) {
	if (x.ret != y.ret || x.a.nmPerPostionLength != y.a.nmPerPostionLength) return false;
	int n = 0, rows = 1;
	if (Note::IsChecksNote(x.a.nmPerPosition, x.a.nmPerPostionLength, n)) rows = Note::RowsForChecks(n);
	else if (Note::IsNote(x.a.nmPerPosition, x.a.nmPerPostionLength, n)) rows = Note::RowsFor(n);
	return memcmp(x.a.nmPerPosition, y.a.nmPerPosition, (size_t) rows * sizeof(PositionNM)) == 0 && strcmp(x.a.pBuffer1, y.a.pBuffer1) == 0 && strcmp(x.a.pBuffer2, y.a.pBuffer2) == 0;
}

static void report(char const * what, Totals const & t) {
	printf("%s: %d checks notes (%d regrown), %d regions-only notes, %d requests kept; records: %d scored, %d too short, %d without a read part, %d without a window\n",
			what, t.checksNotes, t.regrown, t.plainNotes, t.requestsKept, t.scored, t.tooShort, t.noRead, t.noWindow);
}

/* every branch was reached */
static void check_coverage(Totals const & t, bool on) {
	CHECK(t.requestsKept == 1);
	if (on) CHECK(t.checksNotes == 5 && t.plainNotes == 0 && t.regrown == 1 && t.scored >= 20 && t.tooShort >= 1 && t.noRead >= 2 && t.noWindow >= 1);
	else CHECK(t.checksNotes == 0 && t.plainNotes == 5);
}

static void on_aligner(char const * what, std::vector<Case> const & cases, bool jobText, bool on) {
	size_t const n = cases.size();
	printf("aligner with nmRegions, invChecks%s\n", jobText ? ", jobText" : "");
	Aligner al(0, 2.0f, -5.0f, -5.0f, -5.0f, -1.0f, 0.15f, 0, 0, false, true, jobText, true);
	CHECK(al.NmRegions() && al.InvChecks() && al.JobTextOn() == jobText);
	std::vector<Brought> brought;
	long dev0 = 0, host0 = 0, dev1 = 0, host1 = 0;
	Aligner::JobTextStats(dev0, host0);

	/* one launch of windows */
	std::vector<Held *> first = hold(cases);
	bool const haveChecks = staged_tiles(al, cases, first, -1, brought);
	CHECK(haveChecks);      /* the handle delivers them whether or not the binding reads them */
	Totals t;
	for (size_t i = 0; i < n; ++i) check_note(cases[i], *first[i], brought[i], on, t);
	report(what, t);
	check_coverage(t, on);
	Aligner::JobTextStats(dev1, host1);
	if (jobText) CHECK(dev1 - dev0 == 5); else CHECK(dev1 == dev0);

	/* a second answer into the Aligns that hold notes now: a stale checks note is a request */
	{
		std::vector<Brought> again;
		(void) staged_tiles(al, cases, first, -1, again);
		Totals t2;
		for (size_t i = 0; i < n; ++i) check_note(cases[i], *first[i], again[i], on, t2);
		CHECK(t2.checksNotes == t.checksNotes && t2.plainNotes == t.plainNotes && t2.scored == t.scored);
	}

	/* every tile alone through AlignTiles: the same note */
	{
		std::vector<Held *> alone = hold(cases);
		for (size_t i = 0; i < n; ++i) {
			Aligner::Tile tile;
			memset(&tile, 0, sizeof(tile));
			tile.corridor = alone[i]->lines.data(); tile.corridorHeight = (int) alone[i]->lines.size();
			tile.refSeq = alone[i]->reference(cases[i], true); tile.qrySeq = cases[i].qry.c_str(); tile.result = &alone[i]->a; tile.ret = -2;
			al.AlignTiles(&tile, 1);
			alone[i]->ret = tile.ret; alone[i]->failed = tile.failed;
			CHECK(alone[i]->window[0] == 'x');      /* decoded on the device: nothing wrote the caller's buffer */
			/* (a job of one tile without a region brings no checks: its empty note is the regions-only form) */
			if (on && brought[i].regions.empty() && first[i]->ret >= 0) { int z = -1; CHECK(Note::IsNote(alone[i]->a.nmPerPosition, alone[i]->a.nmPerPostionLength, z) && z == 0); }
			else CHECK(same_note(*first[i], *alone[i]));
		}
		free_all(alone);
	}

	/* the same tiles as one ladder job, and each alone through AlignLadders */
	{
		std::vector<Held *> lad = hold(cases), alone = hold(cases);
		std::vector<Brought> lb;
		CHECK(staged_ladders(al, cases, lad, lb));
		Totals tl;
		for (size_t i = 0; i < n; ++i) check_note(cases[i], *lad[i], lb[i], on, tl);
		report("  one ladder job", tl);
		check_coverage(tl, on);
		for (size_t i = 0; i < n; ++i) {
			Aligner::LadderTile tile;
			memset(&tile, 0, sizeof(tile));
			tile.refSeq = alone[i]->reference(cases[i], true); tile.qrySeq = cases[i].qry.c_str(); tile.result = &alone[i]->a;
			tile.ladder = ladder_of(); tile.ret = -2;
			al.AlignLadders(&tile, 1);
			alone[i]->ret = tile.ret; alone[i]->failed = tile.failed;
			if (on && lb[i].regions.empty() && lad[i]->ret >= 0) { int z = -1; CHECK(Note::IsNote(alone[i]->a.nmPerPosition, alone[i]->a.nmPerPostionLength, z) && z == 0); }
			else CHECK(same_note(*lad[i], *alone[i]));
		}
		free_all(lad);
		free_all(alone);
	}

	/* one plain reference string among the windows: the launch is materialised on the host and brings no checks */
	{
		std::vector<Held *> mixed = hold(cases);
		std::vector<Brought> mb;
		long const before = Convex::DeviceInvChecks::Stats().regionsOnlyAlignments;
		long wl0 = 0, wt0 = 0, wm0 = 0, wl1 = 0, wt1 = 0, wm1 = 0;
		Aligner::WindowStats(wl0, wt0, wm0);
		CHECK(!staged_tiles(al, cases, mixed, 4 /* clean */, mb));
		Aligner::WindowStats(wl1, wt1, wm1);
		CHECK(wm1 - wm0 == 1 && wl1 == wl0);
		Totals tm;
		int withRegions = 0;
		for (size_t i = 0; i < n; ++i) { check_note(cases[i], *mixed[i], mb[i], false, tm); withRegions += mixed[i]->ret >= 0 && !mb[i].regions.empty(); }
		report("  a launch with one plain reference", tm);
		CHECK(tm.plainNotes == 5 && tm.checksNotes == 0 && withRegions == 4);
		CHECK(Convex::DeviceInvChecks::Stats().regionsOnlyAlignments - before == (on ? withRegions : 0));
		for (size_t i = 0; i < n; ++i) if (mixed[i]->ret >= 0) CHECK(mb[i].regions.size() == brought[i].regions.size() &&
				(mb[i].regions.empty() || memcmp(mb[i].regions.data(), brought[i].regions.data(), mb[i].regions.size() * sizeof(cvx_nm_region)) == 0));
		free_all(mixed);
	}
	free_all(first);
}

static void without_inv_checks(std::vector<Case> const & cases) {
	printf("aligner with nmRegions only\n");
	Aligner al(0, 2.0f, -5.0f, -5.0f, -5.0f, -1.0f, 0.15f, 0, 0, false, true, false, false);
	CHECK(al.NmRegions() && !al.InvChecks());
	std::vector<Held *> held = hold(cases);
	std::vector<Brought> brought;
	long const before = Convex::DeviceInvChecks::Stats().regionsOnlyAlignments;
	CHECK(!staged_tiles(al, cases, held, -1, brought));
	Totals t;
	for (size_t i = 0; i < cases.size(); ++i) check_note(cases[i], *held[i], brought[i], false, t);
	report("  today's notes", t);
	CHECK(t.plainNotes == 5 && t.checksNotes == 0 && t.requestsKept == 1);
	CHECK(Convex::DeviceInvChecks::Stats().regionsOnlyAlignments == before);      /* nothing was expected of this aligner */
	free_all(held);
	/* invChecks without nmRegions means nothing */
	Aligner plain(0, 2.0f, -5.0f, -5.0f, -5.0f, -1.0f, 0.15f, 0, 0, false, false, false, true);
	CHECK(!plain.NmRegions() && !plain.InvChecks());
}

/* SharedAligner creates its handles with the flag when the binding is on: the same notes, one tile at a time */
static void through_shared(std::vector<Case> const & cases, bool on) {
	Convex::SharedAligner sh(0, 2.0f, -5.0f, -5.0f, -5.0f, -1.0f, 0.15f, 0, false);
	Aligner al(0, 2.0f, -5.0f, -5.0f, -5.0f, -1.0f, 0.15f, 0, 0, false, true, false, true);
	std::vector<Held *> want = hold(cases), got = hold(cases);
	std::vector<Brought> brought;
	(void) staged_tiles(al, cases, want, -1, brought);
	int same = 0;
	for (size_t i = 0; i < cases.size(); ++i) {
		Case const & c = cases[i];
		got[i]->ret = sh.SingleAlign(0, got[i]->lines.data(), (int) got[i]->lines.size(), got[i]->reference(c, true), c.qry.c_str(), got[i]->a, 0, 0, 0);
		bool ok;
		if (on && brought[i].regions.empty() && want[i]->ret >= 0) { int z = -1; ok = Note::IsNote(got[i]->a.nmPerPosition, got[i]->a.nmPerPostionLength, z) && z == 0; }
		else ok = same_note(*want[i], *got[i]);
		CHECK(ok);
		same += ok;
		if (on && want[i]->ret >= 0 && !brought[i].regions.empty()) { int z = -1; CHECK(Note::IsChecksNote(got[i]->a.nmPerPosition, got[i]->a.nmPerPostionLength, z)); }
	}
	printf("SharedAligner (%s): %d of %zu notes as the staged launch leaves them\n", on ? "inversion checks" : "regions only", same, cases.size());
	free_all(want);
	free_all(got);
}

int main() {
	for (int k = 0; k < 9000; ++k) genome.push_back("ACGT"[rnd() % 4]);
	for (int k = 7000; k < 7300; ++k) genome[(size_t) k] = 'A';
	{
		char const * sp[1] = { genome.c_str() };
		uint64_t lens[1] = { genome.size() };
		std::vector<uint8_t> enc((size_t) cvx_genome_encoded_bytes(1, lens));
		uint64_t nib = 0, st[2] = { 0, 0 };
		if (cvx_genome_encode(1, sp, lens, enc.data(), &nib, st, &nStarts) != CVX_OK || nStarts != 2 || (st[0] & 1) || st[0] == 0) { printf("encode failed\n"); return 1; }
		/* the leading spacer dropped: the contig starts at nibble 0 */
		bin.assign(enc.begin() + (long) (st[0] / 2), enc.end());
		nNibbles = nib - st[0];
		starts[0] = 0; starts[1] = st[1] - st[0];
	}
	Convex::DeviceWindows::SetGenome(bin.data(), nNibbles, (unsigned long long const *) starts, nStarts);
	if (!Convex::DeviceWindows::Enabled()) { printf("CVX_DEVICE_DECODE=0\n"); return 1; }

	/* the binding announces itself before the aligners are built */
	CHECK(!Convex::DeviceInvChecks::Enabled());
	Convex::DeviceInvChecks::Announce();
	CHECK(!Convex::DeviceInvChecks::Enabled());      /* not without the regions binding */
	Convex::DeviceRegions::Announce();
	char const * const off = getenv("CVX_DEVICE_INV_CHECKS");
	bool const on = !(off && atoi(off) == 0);
	CHECK(Convex::DeviceRegions::Enabled());
	CHECK(Convex::DeviceInvChecks::Enabled() == on);

	std::vector<Case> cases;
	{
		std::vector<int> m;
		for (int a = 90; a + 24 + 60 < 3000; a += 110) for (int k = 0; k < 24; ++k) m.push_back(a + k);
		cases.push_back(window_case("bursts", 500, 3000, m));
		m.clear();
		for (int k = 18; k < 66; k += 3) m.push_back(k);
		for (int k = 288; k < 312; ++k) m.push_back(k);
		for (int k = 600 - 66; k < 600 - 18; k += 3) m.push_back(k);
		cases.push_back(window_case("edges", 4000, 600, m));
		m.clear();
		for (int k = 0; k < 9; ++k) m.push_back(300 + 3 * k);
		cases.push_back(window_case("short", 5000, 700, m));
		m.clear();
		for (int k = 100; k < 124; ++k) m.push_back(k);
		cases.push_back(window_case("start", 0, 700, m));
		m.clear();
		cases.push_back(window_case("clean", 6000, 700, m));
		Case junk = window_case("invalid", 7050, 200, m);      /* a run of A in the genome against a read of C */
		junk.qry = std::string(180, 'C');
		cases.push_back(junk);
	}

	on_aligner("one launch of windows", cases, false, on);
	on_aligner("one launch of windows, jobText", cases, true, on);
	without_inv_checks(cases);
	through_shared(cases, on);
	if (fails) { printf("invchecks_shim_test: %d checks failed\n", fails); return 1; }
	printf("invchecks_shim_test: ok (%s)\n", on ? "inversion checks" : "regions only");
	return 0;
}
