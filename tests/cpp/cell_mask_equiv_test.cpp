/*
 * cell_mask_equiv_test.cpp -- the lane-mask network of the FAST ring fill's cell update (ngmlr_amd/csrc/cvx_fill_ring.inc, phase2 /
 * phase3) and the way a lane's row activity enters it, restated on the host for one lane (a lane mask is one bit here).  No device
 * code: built with -fsanitize=address,undefined and -ffp-contract=off by tests/test_cell_mask_equiv_cpu.py.
 *
 * Two ways of applying the activity act = (unsigned) cnt < (unsigned) len:
 *
 *   select form   the maximum and the three equalities are computed on every lane; sc = act ? mx : 0, and nD, nI carry `& act`
 *   masked form   the maximum and the equalities are written under EXEC = act into registers that hold zero: sc is +0 and the
 *                 equalities are clear outside the row, nD and nI carry no `& act`
 *
 * and two ways of writing the network behind the equalities:
 *
 *   chain form    extD = nD & isDl, extI = nI & isIu, plane 1 = nI | (eG & ~nD)
 *   short form    extD = eL & isDl, extI = (isIu & eU) & ~nD, plane 1 = (eG | eU) & ~nD: nothing waits for nI
 *
 *   (a) all 64 combinations of (eL, eU, eG, act, isDl, isIu): nD and nI of the short form equal the chain form's always; extD, extI
 *       and both planes wherever act is set; with equalities cleared outside the row the `& act`-free forms equal the select form's.
 *   (b) one slot with the slot above it over random histories -- rows that start and end, +0 and -0 scores, exact ties between all
 *       three candidates, the slot above scoring positive beside a lane outside its row: the masked form's score and equalities
 *       against the select form's bit pattern for bit pattern, and the state either network leaves (score, masks, the penalty a gap
 *       cell pays, the planes inside rows) step for step.
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

struct Net { bool nD, nI, extD, extI, gap, cread; };
/* the parent's network: everything behind nD and nI */
static Net chain_form(bool eL, bool eU, bool eG, bool act, bool isDl, bool isIu, bool with_act) {
	Net n;
	const bool c2 = isIu && eU;
	n.nD = eL && (isDl || !(c2 || eG)) && (act || !with_act);
	n.nI = !n.nD && eU && (isIu || !eG) && (act || !with_act);
	n.gap = n.nD || n.nI;
	n.cread = n.nI || (eG && !n.nD);
	n.extD = n.nD && isDl;
	n.extI = n.nI && isIu;
	return n;
}
static Net short_form(bool eL, bool eU, bool eG, bool act, bool isDl, bool isIu, bool with_act) {
	Net n;
	const bool c2 = isIu && eU;
	n.nD = eL && (isDl || !(c2 || eG)) && (act || !with_act);
	n.nI = !n.nD && eU && (isIu || !eG) && (act || !with_act);
	n.gap = n.nD || n.nI;
	n.cread = (eG || eU) && !n.nD;
	n.extD = eL && isDl;
	n.extI = c2 && !n.nD;
	return n;
}

static void test_combinations() {
	for (int v = 0; v < 64; ++v) {
		const bool eL = v & 1, eU = v & 2, eG = v & 4, act = v & 8, isDl = v & 16, isIu = v & 32;
		const Net p = chain_form(eL, eU, eG, act, isDl, isIu, true);
		/* the short form on the same masks, `& act` kept */
		const Net a = short_form(eL, eU, eG, act, isDl, isIu, true);
		CHECK(a.nD == p.nD && a.nI == p.nI, "combination %d: nD / nI", v);
		if (act) CHECK(a.extD == p.extD && a.extI == p.extI && a.gap == p.gap && a.cread == p.cread, "combination %d: short form inside the row", v);
		/* equalities cleared outside the row, no `& act`: either form */
		const Net b = chain_form(eL && act, eU && act, eG && act, act, isDl, isIu, false);
		const Net ab = short_form(eL && act, eU && act, eG && act, act, isDl, isIu, false);
		for (const Net *q : {&b, &ab}) {
			CHECK(q->nD == p.nD && q->nI == p.nI && q->gap == p.gap, "combination %d: nD / nI / plane 0 without & act", v);
			CHECK(q->extD == p.extD && q->extI == p.extI, "combination %d: extensions without & act", v);
			if (act) CHECK(q->cread == p.cread, "combination %d: plane 1 without & act", v);
			if (!act) CHECK(!q->nD && !q->nI && !q->extD && !q->extI && !q->gap && !q->cread, "combination %d: a lane outside its row fires", v);
		}
	}
	printf("combinations: 64\n");
}

struct Sc { float mat, mis, go, ge, gem, decay; };
static const Sc kScorings[] = {      /* the scorings of cell_update_equiv_test.cpp */
	{2, -5, -5, -5, -1, 0.15f},
	{1, -1, -1, -1, -0.5f, 0.15f},
	{3, -3, -1, -1, -0.5f, 0.15f},
	{2, -5, -5, -2, -2, 0.0f},
	{2, -5, -5, -5, -1, 0.0f},
	{2, -5, -5, -5, -1, 0.01f}, {2, -5, -5, -5, -1, 0.07f}, {2, -5, -5, -5, -1, 0.5f},
	{5, -4, -8, -6, -0.25f, 0.2f},
	{2, -10, -5, -5, -1, 0.15f}, {2, -6, -5, -5, -1, 0.15f}, {2, -7, -4, -3, -2, 0.5f}, {1, -4, -1, -1, -0.5f, 0.05f}, {3, -20, -2, -6, -1, 0.3f},
	{2, 0, -5, -5, -1, 0.15f},
};
static bool table_enabled(float gext, float gem, float decay) {
	volatile float prod = (float) kPenClamp * decay;
	volatile float at_clamp = gext + prod;
	const bool reached = !(at_clamp < gem);
	return (decay >= 0.0f) && (reached || decay == 0.0f);
}

/* v_max3_f32 ... clamp: the maximum clamped to [0, 1]; the sign of a zero result is the instruction's business, so every test runs
 * with a clamp that returns +0, one that returns -0 and one that keeps the sign of its input's zero */
static float max3_clamp(float a, float b, float c, int zero_mode) {
	float m = a > b ? a : b;
	m = m > c ? m : c;
	if (m > 1.0f) return 1.0f;
	if (m > 0.0f) return m;
	if (zero_mode == 0) return 0.0f;
	if (zero_mode == 1) return -0.0f;
	return (m == 0.0f) ? m : 0.0f;
}

struct PenPair { float pen; int32_t next; };
/* one slot's state (cvx_fill_ring.inc: S, dg, the run register, the penalty on its way from LDS, mD, mI, cnt, len) */
struct Slot {
	float S = 0.0f, dg = 0.0f, penp = 0.0f;
	int run = 0;
	bool mD = false, mI = false;
	int cnt = 0, len = 0;
	uint32_t accA = 0, accB = 0, in_row = 0;      /* planes, and which of their bits belong to cells inside a row */
};
/* what the slot above offers: its state of the step before */
struct Up { float S; float penp; int run; bool mI; };

/* one cell update of slot s, in the form (masked, shortened); match = the score the diagonal adds */
static void cell(Slot &s, const Up &u, const std::vector<PenPair> &tab, const float go, const float match, const bool masked, const bool shortened, const int zero_mode,
		float *sc_out, bool *eq_out) {
	auto offer_E = [](float S, float pen) { const float a = S + pen, b = -S; return a > b ? a : b; };
	const float uc = u.mI ? offer_E(u.S, u.penp) : u.S + go;
	const float lc = s.mD ? offer_E(s.S, s.penp) : s.S + go;
	const float dc = s.dg + match;
	const bool act = (unsigned) s.cnt < (unsigned) s.len;
	float sc;
	bool eL, eU, eG;
	if (masked) {
		sc = 0.0f; eL = eU = eG = false;      /* the registers the block writes into hold zero */
		if (act) { sc = max3_clamp(lc, dc, uc, zero_mode); eL = sc == lc; eU = sc == uc; eG = sc == dc; }
	} else {
		const float mx = max3_clamp(lc, dc, uc, zero_mode);
		eL = mx == lc; eU = mx == uc; eG = mx == dc;
		sc = act ? mx : 0.0f;
	}
	const Net n = shortened ? short_form(eL, eU, eG, act, s.mD, u.mI, !masked) : chain_form(eL, eU, eG, act, s.mD, u.mI, !masked);
	const int t1 = n.extI ? u.run : kPenPairStride;
	const int ra = n.extD ? s.run : t1;
	CHECK(ra % kPenPairStride == 0 && ra >= 0 && ra / kPenPairStride < kPenPairs, "table address %d", ra);
	const PenPair pn = tab.at((size_t) (ra / kPenPairStride));
	s.dg = u.S;
	s.S = sc;
	s.run = pn.next;
	s.penp = pn.pen;
	s.mD = n.nD; s.mI = n.nI;
	s.cnt += 1;
	s.accA = (s.accA << 1) | (n.gap ? 1u : 0u);
	s.accB = (s.accB << 1) | (n.cread ? 1u : 0u);
	s.in_row = (s.in_row << 1) | (act ? 1u : 0u);
	if (sc_out) *sc_out = sc;
	if (eq_out) { eq_out[0] = eL && act; eq_out[1] = eU && act; eq_out[2] = eG && act; }
}

static void test_histories() {
	long steps = 0, ties3 = 0, zero_neg = 0, zero_pos = 0, beside = 0, gaps = 0;
	uint64_t rs = 0x2545f4914f6cdd1dull;
	auto rnd = [&]() { rs ^= rs << 13; rs ^= rs >> 7; rs ^= rs << 17; return (uint32_t) (rs >> 32); };
	for (const Sc &s0 : kScorings) {
		if (!table_enabled(s0.ge, s0.gem, s0.decay)) continue;
		std::vector<PenPair> tab((size_t) kPenPairs);
		for (int e = 0; e < kPenPairs; ++e) {
			tab[(size_t) e].pen = fminf(s0.gem, s0.ge + (float) e * s0.decay) * kScoreScale;
			tab[(size_t) e].next = kPenPairStride * (e + 1 < kPenClamp ? e + 1 : kPenClamp);
		}
		const float go = s0.go * kScoreScale, mat = s0.mat * kScoreScale, mis = s0.mis * kScoreScale;
		for (int zero_mode = 0; zero_mode < 3; ++zero_mode) {
			for (int h = 0; h < 40; ++h) {
				/* four copies of the pair (slot above, slot): select + chain (the parent), select + short, masked + chain, masked + short */
				Slot up[4], sl[4];
				const uint32_t match_odds = 2 + rnd() % 4;
				for (int step = 0; step < 600; ++step, ++steps) {
					/* rows start and end: a slot outside its row takes a new one now and then; the slot above independently, so that it is
					 * often live (and positive) beside a slot that is outside its row */
					if ((unsigned) sl[0].cnt >= (unsigned) sl[0].len && rnd() % 6 == 0) {
						const int len = (int) (rnd() % 4 == 0 ? rnd() % 2 : 1 + rnd() % 40), cnt = -(int) (rnd() % 5);
						for (int f = 0; f < 4; ++f) { sl[f].len = len; sl[f].cnt = cnt; }
					}
					if ((unsigned) up[0].cnt >= (unsigned) up[0].len && rnd() % 4 == 0) {
						const int len = (int) (1 + rnd() % 60), cnt = -(int) (rnd() % 3);
						for (int f = 0; f < 4; ++f) { up[f].len = len; up[f].cnt = cnt; }
					}
					/* what the slot above has above it: the empty element, or an engineered offer */
					Up top;
					top.S = (rnd() % 3 == 0) ? (float) (rnd() % 9) * mat : 0.0f;
					top.mI = rnd() % 5 == 0 && top.S > 0.0f;
					top.run = kPenPairStride * (int) (1 + rnd() % kPenClamp);
					top.penp = tab[(size_t) (top.run / kPenPairStride)].pen;
					const float m_up = (rnd() % match_odds) ? mat : mis, m_sl = (rnd() % match_odds) ? mat : mis;
					/* now and then every candidate of the slot is made the same value: +0, -0 or a positive tie */
					const uint32_t forced = rnd() % 16;
					float sc[4]; bool eq[4][3];
					for (int f = 0; f < 4; ++f) {
						const bool masked = f >= 2, shortened = f & 1;
						const Up u = {up[f].S, up[f].penp, up[f].run, up[f].mI};
						if (forced < 3) {
							/* a three-way tie: S, dg and the neighbour's S set so that lc = dc = uc (all through the opening offer) */
							const float v = forced == 0 ? 0.0f : (forced == 1 ? -0.0f : 4.0f * mat);
							sl[f].mD = false; up[f].mI = false;
							sl[f].S = v - go; up[f].S = v - go; sl[f].dg = v - m_sl;
						}
						const Up u2 = {up[f].S, up[f].penp, up[f].run, up[f].mI};
						cell(sl[f], forced < 3 ? u2 : u, tab, go, m_sl, masked, shortened, zero_mode, &sc[f], eq[f]);
						cell(up[f], top, tab, go, m_up, masked, shortened, zero_mode, nullptr, nullptr);
					}
					const bool act = (unsigned) (sl[0].cnt - 1) < (unsigned) sl[0].len;
					if (act && eq[0][0] && eq[0][1] && eq[0][2]) ties3 += 1;
					if (act && sc[0] == 0.0f) { if (std::signbit(sc[0])) zero_neg += 1; else zero_pos += 1; }
					if (!act && up[0].S > 0.0f) beside += 1;
					if (sl[0].mD || sl[0].mI) gaps += 1;
					for (int f = 1; f < 4; ++f) {
						CHECK(bits(sc[f]) == bits(sc[0]), "step %d form %d: score %08x against %08x", step, f, bits(sc[f]), bits(sc[0]));
						CHECK(eq[f][0] == eq[0][0] && eq[f][1] == eq[0][1] && eq[f][2] == eq[0][2], "step %d form %d: equalities", step, f);
						for (const Slot *pair : {sl, up}) {
							const Slot &a = pair[f], &b = pair[0];
							CHECK(bits(a.S) == bits(b.S) && bits(a.dg) == bits(b.dg), "step %d form %d: state", step, f);
							CHECK(a.mD == b.mD && a.mI == b.mI, "step %d form %d: masks", step, f);
							CHECK(a.accA == b.accA, "step %d form %d: plane 0", step, f);      /* (zero outside rows in every form) */
							CHECK(((a.accB ^ b.accB) & b.in_row) == 0u, "step %d form %d: plane 1 inside rows", step, f);
							/* the run register and the penalty are read only through mD / mI */
							if (b.mD || b.mI) CHECK(a.run == b.run && bits(a.penp) == bits(b.penp), "step %d form %d: run register of a gap cell", step, f);
						}
					}
					if (!act) CHECK(bits(sc[2]) == 0u && bits(sc[3]) == 0u, "step %d: +0 outside the row", step);
				}
			}
		}
	}
	CHECK(ties3 > 1000 && zero_neg > 100 && zero_pos > 1000 && beside > 10000 && gaps > 10000, "coverage: %ld three-way ties, %ld / %ld zeros, %ld positive neighbours beside an idle lane, %ld gap cells",
	      ties3, zero_neg, zero_pos, beside, gaps);
	printf("histories: %ld steps, %ld three-way ties, %ld -0 and %ld +0 scores inside rows, %ld positive neighbours beside a lane outside its row, %ld gap cells\n",
	       steps, ties3, zero_neg, zero_pos, beside, gaps);
}

int main() {
	test_combinations();
	test_histories();
	if (g_bad) { printf("cell_mask_equiv_test: %d FAILED\n", g_bad); return 1; }
	printf("cell_mask_equiv_test: ok\n");
	return 0;
}
