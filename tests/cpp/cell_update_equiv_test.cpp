/*
 * cell_update_equiv_test.cpp -- the run register of one slot of the ring fill (ngmlr_amd/csrc/cvx_fill_ring.inc), restated on the
 * host in the two forms the kernel has: the plain table form (a table of penalties, a register that holds 4 * (run + 1), is
 * incremented per cell and clamped once per 32 steps) and the FAST form (a table of {penalty, next address} pairs: the register of
 * the new cell is loaded with its penalty).  No device code: built with -fsanitize=address,undefined and -ffp-contract=off by
 * tests/test_cell_update_equiv_cpu.py.
 *
 *   1. one slot and the slot above it over random histories of the events a cell can be (extends the deletion on its left,
 *      extends the insertion above, opens a gap, no gap), long runs included: the penalty either form looks up is the same bit
 *      pattern at every step, and every address stays inside its table (the tables are allocated to the byte).
 *   2. the chain of next addresses against the arithmetic penalty, runs 0..300, for every scoring that enables the table.
 *
 * The other change the same proposal made to the cell update -- max3 without the zero, the sign of the maximum folded into the
 * activity test -- is not in the kernel (bit-identical, and slower), so nothing restates it here.
 */
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "cvx_types.h"

using namespace cvx;

static int g_bad = 0;
#define CHECK(c, ...) do { if (!(c)) { if (++g_bad <= 20) { printf("FAIL %s:%d %s  ", __FILE__, __LINE__, #c); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
struct Sc { float mat, mis, go, ge, gem, decay; };
static const Sc kScorings[] = {
	{2, -5, -5, -5, -1, 0.15f},            /* the default (PacBio; the ont preset changes nothing that is compiled in) */
	{1, -1, -1, -1, -0.5f, 0.15f},         /* the ont preset's commented-out values */
	{3, -3, -1, -1, -0.5f, 0.15f},
	{2, -5, -5, -2, -2, 0.0f},
	{2, -5, -5, -5, -1, 0.0f},             /* gap_open equal to the first extension penalty */
	{2, -5, -5, -5, -1, 0.01f}, {2, -5, -5, -5, -1, 0.07f}, {2, -5, -5, -5, -1, 0.5f},
	{5, -4, -8, -6, -0.25f, 0.2f},
	{2, -10, -5, -5, -1, 0.15f}, {2, -6, -5, -5, -1, 0.15f}, {2, -7, -4, -3, -2, 0.5f}, {1, -4, -1, -1, -0.5f, 0.05f}, {3, -20, -2, -6, -1, 0.3f},
	{2, 0, -5, -5, -1, 0.15f},             /* mismatch = 0 */
};

/* cvx_create's condition for the table form (cvx_runtime.cpp): the penalty is constant from run kPenClamp on */
static bool table_enabled(float gext, float gem, float decay) {
	volatile float prod = (float) kPenClamp * decay;
	volatile float at_clamp = gext + prod;
	const bool reached = !(at_clamp < gem);
	return (decay >= 0.0f) && (reached || decay == 0.0f);
}

static void test_next_chain() {
	int enabled = 0;
	for (const Sc &s : kScorings) {
		if (!table_enabled(s.ge, s.gem, s.decay)) continue;
		enabled += 1;
		/* the table as the kernel's lanes write it */
		struct Pair { float pen; int32_t next; };
		std::vector<Pair> tab(kPenPairs);      /* (exactly as large as the kernel's: a read past it is the sanitizer's) */
		for (int lane = 0; lane < kPenPairs; ++lane) {
			const int nx = lane + 1 < kPenClamp ? lane + 1 : kPenClamp;
			tab[lane].pen = fminf(s.gem, s.ge + (float) lane * s.decay);
			tab[lane].next = kPenPairStride * nx;
		}
		/* a gap: the opening cell has run 1 and reads entry 1; every extension reads the entry its predecessor loaded */
		int addr = kPenPairStride;
		for (int run = 1; run <= 300; ++run) {
			CHECK(addr % kPenPairStride == 0 && addr >= kPenPairStride && addr / kPenPairStride < kPenPairs, "address %d at run %d", addr, run);
			const Pair p = tab.at(addr / kPenPairStride);
			const float want = fminf(s.gem, s.ge + (float) run * s.decay);
			CHECK(bits(p.pen) == bits(want), "penalty of run %d: %08x vs %08x (ge %g gem %g decay %g)", run, bits(p.pen), bits(want), s.ge, s.gem, s.decay);
			addr = p.next;
		}
		/* run 0 (entry 0 is written, never selected by a gap cell) */
		CHECK(bits(tab[0].pen) == bits(fminf(s.gem, s.ge + 0.0f * s.decay)), "entry 0");
	}
	CHECK(enabled >= 10, "only %d scorings enable the table", enabled);
	CHECK(!table_enabled(-5.0f, -1.0f, 0.01f), "a tiny decay must keep the arithmetic form");
	printf("next chain: %d scorings with the table\n", enabled);
}

/* the two forms of one slot's register over a history of events; `up` is the register of the slot above (its own history) */
struct Pair { float pen; int32_t next; };
static void test_histories() {
	long steps = 0;
	uint64_t rs = 0x9e3779b97f4a7c15ull;
	auto rnd = [&]() { rs ^= rs << 13; rs ^= rs >> 7; rs ^= rs << 17; return (uint32_t) (rs >> 32); };
	for (const Sc &s : kScorings) {
		if (!table_enabled(s.ge, s.gem, s.decay)) continue;
		std::vector<float> told(kPenEntries);
		for (int i = 0; i < kPenEntries; ++i) told[i] = fminf(s.gem, s.ge + (float) i * s.decay);
		std::vector<Pair> tnew(kPenPairs);
		for (int lane = 0; lane < kPenPairs; ++lane) {
			tnew[lane].pen = fminf(s.gem, s.ge + (float) lane * s.decay);
			tnew[lane].next = kPenPairStride * (lane + 1 < kPenClamp ? lane + 1 : kPenClamp);
		}
		for (int h = 0; h < 200; ++h) {
			/* registers of the slot and of the slot above in either form (the kernel starts them at 0: never selected), and
			 * whether the latest cell of each is a deletion / an insertion */
			int o_reg = 0, o_up = 0, n_reg = 0, n_up = 0;
			bool isD = false, upI = false;
			const uint32_t stay = 2 + rnd() % 120;      /* mean length of the runs of this history */
			for (int step = 0; step < 1500; ++step, ++steps) {
				if (step % kPenClampSteps == 0 && step) {      /* the plain form's clamp, where the direction words are flushed */
					o_reg = o_reg < 4 * kPenClamp ? o_reg : 4 * kPenClamp;
					o_up = o_up < 4 * kPenClamp ? o_up : 4 * kPenClamp;
				}
				/* the slot above moves on by itself: an insertion run there grows or ends */
				const bool up_ext = upI && (rnd() % stay) != 0, up_open = !up_ext && (rnd() % 4) == 0;
				const int o_ura = up_ext ? o_up : 4, n_ura = up_ext ? n_up : kPenPairStride;
				/* this slot: extend the deletion on the left, extend the insertion above (the register of the step before), open, or none */
				const uint32_t e = rnd() % stay;
				const bool extD = isD && e != 0, extI = !extD && upI && (rnd() % 3) == 0;
				const bool gap = extD || extI || (rnd() % 3) == 0;
				const int o_ra = extD ? o_reg : (extI ? o_up : 4);
				const int n_ra = extD ? n_reg : (extI ? n_up : kPenPairStride);
				CHECK(o_ra % 4 == 0 && o_ra / 4 < kPenEntries, "plain address %d", o_ra);
				CHECK(n_ra % kPenPairStride == 0 && n_ra / kPenPairStride < kPenPairs, "pair address %d", n_ra);
				const float o_pen = told.at(o_ra / 4);
				const Pair n_p = tnew.at(n_ra / kPenPairStride);
				CHECK(bits(o_pen) == bits(n_p.pen), "step %d: penalty %08x vs %08x (addresses %d, %d; ge %g gem %g decay %g)", step, bits(o_pen), bits(n_p.pen), o_ra, n_ra, s.ge, s.gem, s.decay);
				CHECK(bits(told.at(o_ura / 4)) == bits(tnew.at(n_ura / kPenPairStride).pen), "step %d: penalty of the slot above", step);
				o_reg = o_ra + 4; n_reg = n_p.next;
				o_up = o_ura + 4; n_up = tnew.at(n_ura / kPenPairStride).next;
				isD = gap && (extD || (!extI && (rnd() & 1)));
				upI = up_ext || up_open;
			}
		}
	}
	printf("histories: %ld steps\n", steps);
}

int main() {
	test_histories();
	test_next_chain();
	if (g_bad) { printf("cell_update_equiv_test: %d FAILED\n", g_bad); return 1; }
	printf("cell_update_equiv_test: ok\n");
	return 0;
}
