/*
 * inv_note_test.cpp -- the checks form of the note (nm_regions_note.h) and the rules of the inversion-check binding
 * (inv_checks_binding_logic.h), no device, no library, no ngmlr (tests/test_inv_checks_binding_cpu.py).
 *
 *   inv_note_test                  every check below; exit code 0 = all as stated
 *   inv_note_test classes FILE     FILE holds "inversionLength midpointOnRead readLength" per line: prints inv_check_site_class of
 *                                  each, one per line (the test holds them to the calls recorded from the unmodified reference)
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "nm_regions_note.h"
#include "inv_checks_binding_logic.h"

typedef Convex::NmRegionsNote Note;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

struct Row { int32_t refPosition, readPosition, nm; Row() : refPosition(0), readPosition(0), nm(0) {} };      /* PositionNM's shape and constructor */

static Note::Region region(int i) { Note::Region r = { 100 * i + 7, 100 * i + 40, 90 * i + 3, 90 * i + 33 }; return r; }
static Note::Check check(int i) { Note::Check c = { 10.0f + (float) i, 3.0f + 0.5f * (float) i, i % 4, 500 + i }; return c; }

static bool all_zero(Row const * rows, int from, int to) {
	for (int i = from; i < to; ++i) if (rows[i].refPosition != 0 || rows[i].readPosition != 0 || rows[i].nm != 0) return false;
	return true;
}

static void fill(std::vector<Note::Region> & rg, std::vector<Note::Check> & ck, int n) {
	rg.clear(); ck.clear();
	for (int i = 0; i < n; ++i) { rg.push_back(region(i)); ck.push_back(check(i)); }
}

static void round_trips() {
	int const sizes[] = { 0, 1, 26, 200 };
	for (int n : sizes) {
		std::vector<Note::Region> rg;
		std::vector<Note::Check> ck;
		fill(rg, ck, n);
		int const need = Note::RowsForChecks(n);
		CHECK(need == 1 + (8 * n + 2) / 3 && need * 12 >= 12 + 32 * n);
		std::vector<Row> buf((size_t) need + 3);
		buf[(size_t) need].nm = 77;      /* the row behind the note: never written */
		/* one row short: nothing is written */
		if (need > 1) {
			CHECK(!Note::WriteChecks(buf.data(), need - 1, rg.data(), ck.data(), n));
			CHECK(all_zero(buf.data(), 0, need));
		}
		CHECK(Note::WriteChecks(buf.data(), need, rg.data(), ck.data(), n));
		int got = -1, other = -1;
		CHECK(Note::IsChecksNote(buf.data(), need, got) && got == n);
		CHECK(!Note::IsNote(buf.data(), need + 3, other) && other == -1);            /* never taken for the regions-only form */
		CHECK(!Note::IsRequest(buf.data(), need));
		CHECK(Note::Wanted(buf.data(), need));
		if (need > 1) { int m = -1; CHECK(!Note::IsChecksNote(buf.data(), need - 1, m)); CHECK(!Note::Wanted(buf.data(), need - 1)); }      /* a header whose records would not fit is no note */
		for (int i = 0; i < n; ++i) {
			Note::Region const r = Note::At(buf.data(), i), wr = region(i);
			Note::Check const c = Note::CheckAt(buf.data(), n, i), wc = check(i);
			CHECK(memcmp(&r, &wr, sizeof(r)) == 0);
			CHECK(memcmp(&c, &wc, sizeof(c)) == 0);
		}
		CHECK(buf[(size_t) need].nm == 77);
		/* the regions-only form of the same regions in a buffer large enough for the checks form: not a checks note */
		std::vector<Row> plain((size_t) need + 3);
		CHECK(Note::Write(plain.data(), need + 3, rg.data(), n));
		CHECK(Note::IsNote(plain.data(), need + 3, other) && other == n);
		got = -1;
		CHECK(!Note::IsChecksNote(plain.data(), need + 3, got) && got == -1);
		/* a stale checks note: Clear zeroes every one of its rows and nothing behind them */
		Note::Clear(buf.data(), need + 3);
		CHECK(all_zero(buf.data(), 0, need) && buf[(size_t) need].nm == 77);
		CHECK(!Note::Wanted(buf.data(), need + 3));
		printf("checks note of %d regions: %d rows, round trip and Clear ok\n", n, need);
	}
}

static void regrow() {
	/* the allocation binding's buffer: room for about thirty regions, a request in its first row */
	int cap = Note::RowsFor(30);
	CHECK(cap == 41 && Note::RowsForChecks(26) == 71);
	Row * rows = new Row[cap];
	Note::Request(rows);
	std::vector<Note::Region> rg;
	std::vector<Note::Check> ck;
	fill(rg, ck, 26);
	CHECK(Note::Begin(rows, cap, true));
	Note::PutChecks(rows, cap, rg.data(), ck.data(), 26);
	CHECK(cap == 82);      /* Put's rule: doubled until it fits */
	int n = -1;
	CHECK(Note::IsChecksNote(rows, cap, n) && n == 26);
	for (int i = 0; i < 26; ++i) {
		Note::Region const r = Note::At(rows, i), wr = region(i);
		Note::Check const c = Note::CheckAt(rows, 26, i), wc = check(i);
		CHECK(memcmp(&r, &wr, sizeof(r)) == 0 && memcmp(&c, &wc, sizeof(c)) == 0);
	}
	CHECK(all_zero(rows, 71, cap));
	/* a second answer into the buffer that holds the checks note: fits, no regrow; then a regions-only answer over it */
	Row * const before = rows;
	fill(rg, ck, 12);
	CHECK(Note::Begin(rows, cap, true));
	Note::PutChecks(rows, cap, rg.data(), ck.data(), 12);
	CHECK(rows == before && cap == 82 && Note::IsChecksNote(rows, cap, n) && n == 12);
	CHECK(Note::Begin(rows, cap, true));
	Note::Put(rows, cap, rg.data(), 12);
	CHECK(rows == before && Note::IsNote(rows, cap, n) && n == 12 && !Note::IsChecksNote(rows, cap, n));
	/* a small buffer of none: PutChecks allocates by Put's rule */
	delete[] rows;
	rows = 0; cap = 0;
	Note::PutChecks(rows, cap, rg.data(), ck.data(), 12);
	CHECK(rows != 0 && cap == 64 && Note::IsChecksNote(rows, cap, n) && n == 12);
	delete[] rows;
	printf("regrow from 41 rows ok\n");
}

static void stale_notes() {
	std::vector<Note::Region> rg;
	std::vector<Note::Check> ck;
	fill(rg, ck, 5);
	int const need = Note::RowsForChecks(5);
	/* Begin without regions: the stale checks note is cleared -- all of its rows -- and a profile follows */
	{
		std::vector<Row> buf(40);
		CHECK(Note::WriteChecks(buf.data(), 40, rg.data(), ck.data(), 5));
		CHECK(Note::Wanted(buf.data(), 40));
		CHECK(!Note::Begin(buf.data(), 40, false));
		CHECK(all_zero(buf.data(), 0, 40));
	}
	/* Begin with regions: wanted, nothing touched */
	{
		std::vector<Row> buf(40);
		CHECK(Note::WriteChecks(buf.data(), 40, rg.data(), ck.data(), 5));
		CHECK(Note::Begin(buf.data(), 40, true));
		int n = -1;
		CHECK(Note::IsChecksNote(buf.data(), 40, n) && n == 5);
	}
	/* BeginProfile: a buffer too small for the profile is replaced by a zeroed one of 2 * (readLength + 1) rows ... */
	{
		int cap = 40;
		Row * rows = new Row[cap];
		CHECK(Note::WriteChecks(rows, cap, rg.data(), ck.data(), 5));
		CHECK(Note::BeginProfile(rows, cap, 100));
		CHECK(cap == 202 && all_zero(rows, 0, cap));
		CHECK(!Note::BeginProfile(rows, cap, 100));      /* zeros: nobody asked */
		delete[] rows;
	}
	/* ... and one that is large enough is cleared in place, every row of the note */
	{
		int cap = 300;
		Row * rows = new Row[cap];
		Row * const before = rows;
		CHECK(Note::WriteChecks(rows, cap, rg.data(), ck.data(), 5));
		rows[need].nm = 9;
		CHECK(Note::BeginProfile(rows, cap, 100));
		CHECK(rows == before && cap == 300 && all_zero(rows, 0, need) && rows[need].nm == 9);
		delete[] rows;
	}
	printf("stale checks notes ok\n");
}

static void taken_for_neither() {
	int n = -1;
	/* zeros */
	std::vector<Row> zeros(100);
	CHECK(!Note::IsChecksNote(zeros.data(), 100, n) && !Note::IsNote(zeros.data(), 100, n) && !Note::IsRequest(zeros.data(), 100) && !Note::Wanted(zeros.data(), 100));
	/* profile rows: both positions >= 1, 0 <= nm <= 32 -- the magic words themselves in the positions included */
	int32_t const nms[] = { 0, 1, 32 };
	for (int32_t nm : nms) {
		std::vector<Row> prof(100);
		for (int i = 0; i < 100; ++i) { prof[(size_t) i].refPosition = 17 + i; prof[(size_t) i].readPosition = 1 + i; prof[(size_t) i].nm = nm; }
		CHECK(!Note::IsChecksNote(prof.data(), 100, n) && !Note::IsNote(prof.data(), 100, n) && !Note::Wanted(prof.data(), 100));
		prof[0].refPosition = Note::kMagicRef; prof[0].readPosition = Note::kMagicRead;      /* (no profile has them: negative) */
		CHECK(!Note::IsChecksNote(prof.data(), 100, n) && !Note::IsNote(prof.data(), 100, n) && !Note::Wanted(prof.data(), 100));
	}
	/* a request */
	std::vector<Row> req(100);
	Note::Request(req.data());
	CHECK(Note::IsRequest(req.data(), 100) && !Note::IsChecksNote(req.data(), 100, n) && !Note::IsNote(req.data(), 100, n));
	Note::Clear(req.data(), 100);
	CHECK(all_zero(req.data(), 0, 100));
	/* the headers between the two ranges, and at their edges */
	struct { int32_t third; bool note, checks; } const heads[] = {
		{ -1, true, false }, { -2, true, false }, { -1 - INT32_MAX / 8, false, false } /* (would not fit) */, { -2 - INT32_MAX / 8, false, false },
		{ Note::kChecksBase + 1, false, false }, { Note::kChecksBase, false, true }, { Note::kChecksBase - 1, false, true },
		{ Note::kChecksBase - INT32_MAX / 8 - 1, false, false }, { INT32_MIN + 1, false, false }, { 0, false, false }, { 5, false, false },
	};
	for (size_t k = 0; k < sizeof(heads) / sizeof(heads[0]); ++k) {
		std::vector<Row> buf(100);
		buf[0].refPosition = Note::kMagicRef; buf[0].readPosition = Note::kMagicRead; buf[0].nm = heads[k].third;
		int a = -1, b = -1;
		CHECK(Note::IsNote(buf.data(), 100, a) == heads[k].note);
		CHECK(Note::IsChecksNote(buf.data(), 100, b) == heads[k].checks);
		CHECK(!Note::IsRequest(buf.data(), 100));
	}
	CHECK(!Note::IsChecksNote(0, 10, n) && !Note::IsChecksNote(zeros.data(), 0, n));
	printf("profiles, zeros and requests are taken for neither form\n");
}

static void logic() {
	using namespace Convex;
	int const H = 1000;
	/* the site's class: inversionLength 10 / 11, the midpoint at 49 / 50, mid + 50 against H */
	CHECK(inv_check_site_class(10, 500, H) == kInvCheckTooShort);
	CHECK(inv_check_site_class(11, 500, H) == kInvCheckScored);
	CHECK(inv_check_site_class(0, 500, H) == kInvCheckTooShort && inv_check_site_class(-5, 500, H) == kInvCheckTooShort);
	CHECK(inv_check_site_class(11, 49, H) == kInvCheckNoRead);
	CHECK(inv_check_site_class(11, 50, H) == kInvCheckScored);          /* mid == 50: readCheckLength <= mid */
	CHECK(inv_check_site_class(11, 949, H) == kInvCheckScored);         /* mid + 50 == H - 1 */
	CHECK(inv_check_site_class(11, 950, H) == kInvCheckNoRead);         /* mid + 50 == H: not < H */
	CHECK(inv_check_site_class(11, 951, H) == kInvCheckNoRead);
	CHECK(inv_check_site_class(11, 50, 100) == kInvCheckNoRead && inv_check_site_class(11, 50, 101) == kInvCheckScored);
	CHECK(inv_check_site_class(11, 0, H) == kInvCheckNoRead);
	/* a uloc that wrapped below zero: 50 <= mid holds and mid + 50 wraps back below H -- the reference's unsigned arithmetic goes on
	 * to copy, so the site says so; a device record (int arithmetic: NO_READ) then disagrees and the reference's path runs */
	CHECK(inv_check_site_class(11, (uint64_t) -3, H) == kInvCheckScored);
	CHECK(inv_check_outcome(kInvCheckNoRead, 11, (uint64_t) -3, H) == kInvOutcomeOwnInconsistent);
	CHECK(inv_check_site_class(10, 49, H) == kInvCheckTooShort);       /* the length is asked first */
	/* every status against every class of the site */
	struct { int status, invLen; uint64_t mid; InvCheckOutcome want; } const cases[] = {
		{ kInvCheckScored, 11, 500, kInvOutcomeTakeScores }, { kInvCheckScored, 11, 50, kInvOutcomeTakeScores }, { kInvCheckScored, 11, 949, kInvOutcomeTakeScores },
		{ kInvCheckScored, 11, 49, kInvOutcomeOwnInconsistent }, { kInvCheckScored, 11, 950, kInvOutcomeOwnInconsistent }, { kInvCheckScored, 10, 500, kInvOutcomeOutside },
		{ kInvCheckNoRead, 11, 49, kInvOutcomeNoRead }, { kInvCheckNoRead, 11, 950, kInvOutcomeNoRead }, { kInvCheckNoRead, 11, 500, kInvOutcomeOwnInconsistent },
		{ kInvCheckNoRead, 11, 50, kInvOutcomeOwnInconsistent }, { kInvCheckNoRead, 10, 49, kInvOutcomeOutside },
		{ kInvCheckNoWindow, 11, 500, kInvOutcomeOwnNoWindow }, { kInvCheckNoWindow, 11, 49, kInvOutcomeOwnInconsistent }, { kInvCheckNoWindow, 10, 500, kInvOutcomeOutside },
		{ kInvCheckTooShort, 11, 500, kInvOutcomeOwnInconsistent }, { kInvCheckTooShort, 11, 49, kInvOutcomeOwnInconsistent }, { kInvCheckTooShort, 10, 500, kInvOutcomeOutside },
		{ 4, 11, 500, kInvOutcomeOwnInconsistent }, { -1, 11, 49, kInvOutcomeOwnInconsistent },
	};
	for (size_t k = 0; k < sizeof(cases) / sizeof(cases[0]); ++k) {
		InvCheckOutcome const got = inv_check_outcome(cases[k].status, cases[k].invLen, cases[k].mid, H);
		if (got != cases[k].want) printf("case %zu: status %d, length %d, mid %llu: outcome %d, want %d\n", k, cases[k].status, cases[k].invLen, (unsigned long long) cases[k].mid, (int) got, (int) cases[k].want);
		CHECK(got == cases[k].want);
	}
	/* the slot: a record lasts as long as its offer */
	InvCheckSlot slot;
	CHECK(slot.state == InvCheckSlot::kNone);
	{
		InvCheckOffer const offer(slot, 21.0f, 8.0f, kInvCheckScored);
		CHECK(slot.state == InvCheckSlot::kRecord && slot.scoreFwd == 21.0f && slot.scoreRev == 8.0f && slot.status == kInvCheckScored);
	}
	CHECK(slot.state == InvCheckSlot::kNone && slot.scoreFwd == 0.0f && slot.scoreRev == 0.0f);
	{
		InvCheckOffer const offer(slot);
		CHECK(slot.state == InvCheckSlot::kNoteWithoutChecks);
	}
	CHECK(slot.state == InvCheckSlot::kNone);
	/* verify mode: svType and the bits of both scores */
	CHECK(inv_check_agrees(kInvOutcomeTakeScores, 1, 21.0f, 8.0f, 1, true, 21.0f, 8.0f));
	CHECK(!inv_check_agrees(kInvOutcomeTakeScores, 1, 21.0f, 8.0f, 0, true, 21.0f, 8.0f));
	CHECK(!inv_check_agrees(kInvOutcomeTakeScores, 1, 21.0f, 8.0f, 1, true, 21.0f, 9.0f));
	CHECK(!inv_check_agrees(kInvOutcomeTakeScores, 1, 21.0f, 8.0f, 1, true, 20.0f, 8.0f));
	CHECK(!inv_check_agrees(kInvOutcomeTakeScores, 0, 0.0f, 8.0f, 0, true, -0.0f, 8.0f));      /* bits, not values */
	CHECK(!inv_check_agrees(kInvOutcomeTakeScores, 0, 21.0f, 8.0f, 0, false, 0.0f, 0.0f));      /* the reference skipped what the record scored */
	CHECK(inv_check_agrees(kInvOutcomeNoRead, 0, 0.0f, 0.0f, 0, false, 0.0f, 0.0f));
	CHECK(!inv_check_agrees(kInvOutcomeNoRead, 0, 0.0f, 0.0f, 0, true, 0.0f, 0.0f));
	CHECK(!inv_check_agrees(kInvOutcomeOwnNoWindow, 0, 0.0f, 0.0f, 0, true, 0.0f, 0.0f));
	printf("binding logic ok\n");
}

static int classes(char const * path) {
	FILE * f = fopen(path, "r");
	if (!f) { fprintf(stderr, "inv_note_test: cannot read %s\n", path); return 2; }
	long long invLen = 0, readLen = 0;
	unsigned long long mid = 0;
	while (fscanf(f, "%lld %llu %lld", &invLen, &mid, &readLen) == 3) printf("%d\n", Convex::inv_check_site_class((int) invLen, (uint64_t) mid, (int) readLen));
	fclose(f);
	return 0;
}

int main(int argc, char ** argv) {
	if (argc == 3 && strcmp(argv[1], "classes") == 0) return classes(argv[2]);
	round_trips();
	regrow();
	stale_notes();
	taken_for_neither();
	logic();
	if (fails) { printf("inv_note_test: %d checks failed\n", fails); return 1; }
	printf("inv_note_test: ok\n");
	return 0;
}
