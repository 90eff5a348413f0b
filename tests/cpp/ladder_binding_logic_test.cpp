/*
 * ladder_binding_logic_test.cpp -- the rules of ngmlr_amd/csrc/ladder_binding_logic.h as a program of its own (its own main, no
 * HIP, no ngmlr, no library): tests/test_ladder_binding_logic_cpu.py builds it plain and under -fsanitize=address,undefined.
 *
 * The left / right fill against a straightforward restatement over an array of anchors in which every binary32 operation is
 * carried out in double and rounded to float once (for +, -, * and / of two floats that is the correctly rounded binary32
 * result, whatever the compiler does with the expression), bit for bit, on engineered anchor sets -- no anchor, one anchor on
 * the line, anchors far left and far right, reverse-strand anchors, refLen != qryLen -- and on a random sweep; a few values by
 * hand.  The counters against the reference's loop run on a list of per-rung outcomes, for attempts 1 .. 5 x {last valid, last
 * failed, an alignment of another length}.
 */
#include <cstdio>
#include <cstring>
#include <stdint.h>
#include <vector>

#include "ladder_binding_logic.h"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

struct Anchor { int x, onRead; bool reverse; };

static float rn(double const v) { return (float) v; }
static uint32_t bits(float const f) { uint32_t u; memcpy(&u, &f, 4); return u; }

/* getCorridorEndpointsWithAnchors up to its multiplier, two passes over the array, every operation rounded once */
static void restated(std::vector<Anchor> const & anchors, int externalQStart, int readPartLength, int fullReadLength, int qryLen, int refLen, float & left, float & right) {
	float const k = rn((double) rn((double) (float) qryLen * 1.0) / (double) (float) refLen);
	std::vector<float> diffs;
	for (size_t i = 0; i < anchors.size(); ++i) {
		Anchor const & a = anchors[i];
		int const y = a.reverse ? fullReadLength - a.onRead - readPartLength - externalQStart : a.onRead - externalQStart;
		float const expect = rn((double) (float) y / (double) k);
		diffs.push_back(rn((double) expect - (double) (float) a.x));
	}
	left = 0.0f; right = 0.0f;
	for (size_t i = 0; i < diffs.size(); ++i) if (diffs[i] > 0 && diffs[i] > right) right = diffs[i];
	for (size_t i = 0; i < diffs.size(); ++i) if (!(diffs[i] > 0) && -diffs[i] > left) left = -diffs[i];
	left = rn((double) left + 128.0);
	right = rn((double) right + 128.0);
	left = rn((double) left + (double) rn((double) rn((double) left + (double) right) * (double) 0.1f));
	right = rn((double) right + (double) rn((double) rn((double) left + (double) right) * (double) 0.1f));
}

static void fill(std::vector<Anchor> const & anchors, int externalQStart, int readPartLength, int fullReadLength, int qryLen, int refLen, float & left, float & right) {
	Convex::LadderFill f(externalQStart, readPartLength, fullReadLength, qryLen, refLen);
	for (size_t i = 0; i < anchors.size(); ++i) f.Add(anchors[i].x, anchors[i].onRead, anchors[i].reverse);
	f.Finish(left, right);
}

static bool same_fill(char const * what, std::vector<Anchor> const & anchors, int externalQStart, int readPartLength, int fullReadLength, int qryLen, int refLen) {
	float l = -1.0f, r = -1.0f, wl = -2.0f, wr = -2.0f;
	fill(anchors, externalQStart, readPartLength, fullReadLength, qryLen, refLen, l, r);
	restated(anchors, externalQStart, readPartLength, fullReadLength, qryLen, refLen, wl, wr);
	bool const ok = bits(l) == bits(wl) && bits(r) == bits(wr);
	if (!ok) printf("  %s: left %a (want %a), right %a (want %a)\n", what, (double) l, (double) wl, (double) r, (double) wr);
	return ok;
}

static uint32_t rs = 4711;
static uint32_t rnd() { rs = rs * 1664525u + 1013904223u; return rs >> 8; }

/* the reference's loop (src/AlignmentBuffer.cpp:291-425) on a list of what each rung's SingleAlign returns */
struct Loop { bool valid; int alignmentIds, invalid, multiplier; };
static Loop reference_loop(std::vector<int> const & rets, int fullReadLength) {
	Loop o = { false, 0, 0, 1 };
	size_t rung = 0;
	while (!o.valid && rung < rets.size()) {
		int const cigarLength = rets[rung++];
		o.alignmentIds += 1;
		o.valid = cigarLength == fullReadLength;
		if (!o.valid) { o.multiplier += 1; o.invalid += 1; }
	}
	return o;
}

int main() {
	/* ---- the fill */
	{
		std::vector<Anchor> none;
		float l = 0.0f, r = 0.0f;
		fill(none, 0, 256, 10000, 1000, 1000, l, r);
		CHECK(bits(l) == bits(153.6f) && bits(r) == bits(156.16f));      /* 128 + 25.6; 128 + (153.6 + 128) / 10: the recordings' most frequent pair */
		CHECK(same_fill("no anchor", none, 0, 256, 10000, 1000, 1000));
		CHECK(same_fill("no anchor, other lengths", none, 17, 256, 9000, 700, 1300));
	}
	{
		std::vector<Anchor> one(1);
		one[0].x = 400; one[0].onRead = 400; one[0].reverse = false;      /* on the line from corner to corner: moves neither side */
		float l = 0.0f, r = 0.0f;
		fill(one, 0, 256, 10000, 1000, 1000, l, r);
		CHECK(bits(l) == bits(153.6f) && bits(r) == bits(156.16f));
		CHECK(same_fill("one anchor on the line", one, 0, 256, 10000, 1000, 1000));
		one[0].x = 100;      /* 300 columns to the left of where the line expects it: the right side grows */
		fill(one, 0, 256, 10000, 1000, 1000, l, r);
		CHECK(bits(l) == bits(183.6f) && bits(r) == bits(489.16f));      /* 128 + 55.6; 428 + 61.16 */
		CHECK(same_fill("one anchor 300 to the right", one, 0, 256, 10000, 1000, 1000));
		one[0].x = 900;      /* and 500 to the other side */
		fill(one, 0, 256, 10000, 1000, 1000, l, r);
		CHECK(l > 628.0f && r > 128.0f && r < l);
		CHECK(same_fill("one anchor 500 to the left", one, 0, 256, 10000, 1000, 1000));
	}
	{
		std::vector<Anchor> far;
		int const xs[] = { 10, 5000, 2500, 9000, 40 }, ys[] = { 4000, 300, 2500, 8990, 41 };
		for (int i = 0; i < 5; ++i) { Anchor a = { xs[i], ys[i] + 123, false }; far.push_back(a); }
		CHECK(same_fill("anchors far left and far right", far, 123, 256, 30000, 9100, 9100));
		CHECK(same_fill("anchors far left and far right, refLen > qryLen", far, 123, 256, 30000, 9100, 11873));
		CHECK(same_fill("anchors far left and far right, refLen < qryLen", far, 123, 256, 30000, 9100, 7001));
	}
	{
		/* reverse-strand anchors count from the other end of the full read, a read part further in */
		std::vector<Anchor> rev;
		int const full = 20000, part = 256, start = 3000;
		int const xs[] = { 100, 1500, 2900 }, ys[] = { 130, 1400, 3100 };
		for (int i = 0; i < 3; ++i) { Anchor a = { xs[i], full - ys[i] - part - start, true }; rev.push_back(a); }
		float l = 0.0f, r = 0.0f, fl = 0.0f, fr = 0.0f;
		fill(rev, start, part, full, 4000, 4100, l, r);
		std::vector<Anchor> fwd;
		for (int i = 0; i < 3; ++i) { Anchor a = { xs[i], ys[i] + start, false }; fwd.push_back(a); }
		fill(fwd, start, part, full, 4000, 4100, fl, fr);
		CHECK(bits(l) == bits(fl) && bits(r) == bits(fr));      /* the same points of the tile either way */
		CHECK(same_fill("reverse-strand anchors", rev, start, part, full, 4000, 4100));
		rev.push_back(fwd[1]);
		CHECK(same_fill("both strands", rev, start, part, full, 4000, 4100));
	}
	{
		int ok = 0, n = 0;
		for (int c = 0; c < 4000; ++c) {
			int const qryLen = 1 + (int) (rnd() % 12000), refLen = 1 + (int) (rnd() % 14000);
			int const full = qryLen + (int) (rnd() % 30000), part = 256, start = (int) (rnd() % 5000);
			std::vector<Anchor> as;
			for (int i = (int) (rnd() % 9); i > 0; --i) {
				Anchor a = { (int) (rnd() % (uint32_t) (refLen + 200)) - 100, (int) (rnd() % (uint32_t) (full + 1)), (rnd() & 1) != 0 };
				as.push_back(a);
			}
			ok += same_fill("sweep", as, start, part, full, qryLen, refLen);
			n += 1;
		}
		printf("  fill: %d of %d random anchor sets bit for bit as restated\n", ok, n);
		CHECK(ok == n);
	}

	/* ---- acceptance and the counters */
	int const full = 9876;
	for (int attempts = 1; attempts <= 5; ++attempts) {
		{      /* the reported rung is valid */
			std::vector<int> rets((size_t) attempts, -1);
			rets.back() = full;
			Loop const w = reference_loop(rets, full);
			Convex::LadderOutcome const o = Convex::ladder_outcome(full, full, attempts, attempts, 5);
			CHECK(o.valid && w.valid);
			CHECK(o.alignmentIds == w.alignmentIds && o.invalidAlignments == w.invalid && o.corridorMultiplier == w.multiplier);
			CHECK(o.invalidAlignments == attempts - 1 && o.widthsCounted == attempts);
		}
		{      /* the last rung failed too: the ladder has `attempts` rungs */
			std::vector<int> rets((size_t) attempts, -1);
			Loop const w = reference_loop(rets, full);
			Convex::LadderOutcome const o = Convex::ladder_outcome(-1, full, attempts, attempts, attempts);
			CHECK(!o.valid && !w.valid);
			CHECK(o.alignmentIds == w.alignmentIds && o.invalidAlignments == w.invalid && o.corridorMultiplier == w.multiplier);
			CHECK(o.invalidAlignments == attempts && o.widthsCounted == attempts);
		}
		for (int rungs = attempts; rungs <= 5; ++rungs) {      /* an alignment of another length at the reported rung: the loop tries every rung there is, each returns that length */
			std::vector<int> rets((size_t) rungs, full - 7);
			for (int m = 0; m + 1 < attempts; ++m) rets[(size_t) m] = -1;
			Loop const w = reference_loop(rets, full);
			Convex::LadderOutcome const o = Convex::ladder_outcome(full - 7, full, attempts, attempts, rungs);
			CHECK(!o.valid && !w.valid);
			CHECK(o.invalidAlignments == w.invalid && o.invalidAlignments == rungs && o.corridorMultiplier == w.multiplier);
			CHECK(o.alignmentIds == attempts && o.widthsCounted == attempts);      /* by the attempts the device made */
		}
	}
	CHECK(Convex::ladder_outcome(0, 0, 1, 1, 5).valid);      /* fullReadLength 0 is a length like any other */
	{
		int asked = 0;
		long const sum = Convex::ladder_corridor_len(3, [&](int const m) { asked += 1; return 100 * m + 1; });
		CHECK(sum == 101 + 201 + 301 && asked == 3);
		CHECK(Convex::ladder_corridor_len(0, [&](int const) { return 5; }) == 0);
	}
	if (fails) { printf("ladder_binding_logic_test: %d failures\n", fails); return 1; }
	printf("ladder_binding_logic_test: ok\n");
	return 0;
}
