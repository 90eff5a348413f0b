/*
 * cell_scale_equiv_test.cpp -- the cell update of the FAST ring fill (ngmlr_amd/csrc/cvx_fill_ring.inc) restated on the host for
 * whole small tiles in the two domains the kernel text has:
 *
 *   plain    unscaled scores; the gap-extension offer max(S + pen, S * -2^100); the maximum max(max3(lc, dc, uc), 0)
 *   scaled   every scoring value and table penalty times kScoreScale = 2^-64 (the penalties computed unscaled first); the offer
 *            max(S + pen, -S); the maximum med3(max(max(lc, dc), uc), 0, 1) -- the clamp bit of v_max3_f32
 *
 * Per cell the lane masks the kernel derives (eL, eU, eG and the nD / nI outcome) must be identical and S_scaled * 2^64 bit-equal
 * to S.  The sign of a zero maximum is the instruction's business: the scaled form is run with a clamp that returns +0, -0 and
 * the sign of its input for a zero; with +0 every score is bit-equal, with the other two every nonzero score is and a zero is a
 * zero of either sign -- masks identical throughout, which is what "the sign of a zero is not observable" means.
 * Also score_scale_exact() (cvx_host_logic.h), the host's condition for the scaled form.
 * No device code: built with -fsanitize=address,undefined and -ffp-contract=off by tests/test_cell_scale_equiv_cpu.py.
 */
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "cvx_host_logic.h"

using namespace cvx;

static int g_bad = 0;
#define CHECK(c, ...) do { if (!(c)) { if (++g_bad <= 20) { printf("FAIL %s:%d %s  ", __FILE__, __LINE__, #c); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
struct Sc { float mat, mis, go, ge, gem, decay; };
/* the default (every preset: pacbio and ont differ in nothing the fill reads), then the scorings of tools/fuzz_parity.py's scoring mode */
static const Sc kScorings[] = {
	{2, -5, -5, -5, -1, 0.15f},
	{2, -10, -5, -5, -1, 0.15f}, {2, -6, -5, -5, -1, 0.15f}, {2, -7, -4, -3, -2, 0.5f}, {1, -4, -1, -1, -0.5f, 0.05f}, {3, -20, -2, -6, -1, 0.3f},
	{2, -5, -5, -5, -1, 0.0f}, {2, -5, -5, -5, -1, 0.01f}, {2, -5, -5, -5, -1, 0.07f}, {2, -5, -5, -5, -1, 0.5f},
	{2, -5, -5, -2, -2, 0.0f},
	{1, -1, -1, -1, -0.5f, 0.15f},
	{3, -3, -1, -1, -0.5f, 0.15f},
	{5, -4, -8, -6, -0.25f, 0.2f},
};
/* the edges of the admitted range: match + mismatch = 2^-43, the quantum itself (scaled: 2^-107, the smallest value the scaled
 * domain ever holds); and the largest admitted magnitudes */
static const Sc kEdgeScorings[] = {
	{0x1.000002p-20f, -0x1p-20f, -0x1p-20f, -0x1p-20f, -0x1p-20f, 0.0f},
	{0x1.000002p-20f, -0x1p-20f, -0x1.8p-20f, -0x1.8p-20f, -0x1p-20f, 0x1p-24f},
	{0x1.fffffep20f, -0x1.fffffep20f, -0x1.fffffep20f, -0x1.fffffep20f, -0x1p20f, 0x1p15f},
	{0x1p20f, -0x1.000002p20f, -0x1p-20f, -0x1p20f, -0x1p-20f, 0x1p16f},
};

/* a maximum that prefers +0 among zeros (what the parent's v_max_f32 against the constant 0 returns), so that the plain domain is
 * one deterministic function on the host */
static float max_pz(float a, float b) { return a > b ? a : (b > a ? b : (std::signbit(a) ? b : a)); }
/* the host's maximum as the compiler leaves it: either zero may come back */
static float max_any(float a, float b) { return a > b ? a : b; }

enum ZeroSign { kPlus, kMinus, kInput };
struct Cell { float S; bool isD, isI; int run; float pen; };      /* run: the table entry the cell read (1 unless it extends a gap) */
struct Masks { bool eL, eU, eG, nD, nI; };

struct Domain {
	bool scaled; ZeroSign zs;
	float mat, mis, go;
	float pen[kPenPairs];
	Domain(const Sc &s, bool scaled_, ZeroSign zs_) : scaled(scaled_), zs(zs_) {
		const float k = scaled ? kScoreScale : 1.0f;
		mat = s.mat * k; mis = s.mis * k; go = s.go * k;
		for (int e = 0; e < kPenPairs; ++e) pen[e] = fminf(s.gem, s.ge + (float) e * s.decay) * k;
	}
	float offer_E(const Cell &c) const { return scaled ? max_any(c.S + c.pen, -c.S) : max_any(c.S + c.pen, c.S * -0x1p100f); }
	float maximum(float lc, float dc, float uc) const {
		const float m3 = max_any(max_any(lc, dc), uc);
		if (!scaled) return max_pz(m3, 0.0f);
		if (m3 > 1.0f) return 1.0f;      /* (never: checked by the caller) */
		if (m3 > 0.0f) return m3;
		return zs == kPlus ? 0.0f : (zs == kMinus ? -0.0f : (m3 == 0.0f ? m3 : 0.0f));
	}
};

/* one tile, full matrix; `zero_in`: the sign of the empty element's score outside the matrix (the kernel's is +0; -0 feeds the other
 * zero into the first row's and column's offers) */
static void run_tile(const Domain &d, const std::string &ref, const std::string &qry, float zero_in, std::vector<Cell> &cells, std::vector<Masks> &masks) {
	const int W = (int) ref.size(), H = (int) qry.size();
	cells.assign((size_t) W * H, Cell());
	masks.assign((size_t) W * H, Masks());
	Cell empty; empty.S = zero_in; empty.isD = empty.isI = false; empty.run = 1; empty.pen = d.pen[1];
	auto at = [&](int y, int x) -> const Cell & { return (y < 0 || x < 0) ? empty : cells[(size_t) y * W + x]; };
	for (int y = 0; y < H; ++y) for (int x = 0; x < W; ++x) {
		const Cell &L = at(y, x - 1), &U = at(y - 1, x), &G = at(y - 1, x - 1);
		const float lc = L.isD ? d.offer_E(L) : L.S + d.go;
		const float uc = U.isI ? d.offer_E(U) : U.S + d.go;
		const float dc = G.S + (ref[x] == qry[y] ? d.mat : d.mis);
		const float mx = d.maximum(lc, dc, uc);
		Masks m;
		m.eL = mx == lc; m.eU = mx == uc; m.eG = mx == dc;
		const bool c2 = U.isI && m.eU;
		m.nD = m.eL && (L.isD || !(c2 || m.eG));
		m.nI = !m.nD && m.eU && (U.isI || !m.eG);
		Cell c;
		c.S = mx; c.isD = m.nD; c.isI = m.nI;
		const int ext = (m.nD && L.isD) ? L.run : ((m.nI && U.isI) ? U.run : 0);
		c.run = ext + 1 < kPenClamp ? ext + 1 : kPenClamp;      /* the saturating next address */
		c.pen = d.pen[c.run];
		cells[(size_t) y * W + x] = c;
		masks[(size_t) y * W + x] = m;
	}
}

static long g_cells = 0, g_zero_ext = 0, g_quantum = 0, g_tiles = 0;

static void compare_tile(const Sc &s, const std::string &ref, const std::string &qry, const char *what) {
	std::vector<Cell> pc, sc; std::vector<Masks> pm, sm;
	const Domain plain(s, false, kPlus);
	run_tile(plain, ref, qry, 0.0f, pc, pm);
	const int W = (int) ref.size();
	bool any_pos = false;
	for (size_t i = 0; i < pc.size(); ++i) {
		any_pos = any_pos || pc[i].S > 0.0f;
		/* a zero-score gap cell that extends a zero-score gap cell: the offer is a zero, not score + penalty */
		if (pc[i].S == 0.0f && ((pc[i].isD && i % W && pc[i - 1].isD && pc[i - 1].S == 0.0f) || (pc[i].isI && i >= (size_t) W && pc[i - W].isI && pc[i - W].S == 0.0f))) g_zero_ext += 1;
		if (pc[i].S != 0.0f && fabsf(pc[i].S) <= 0x1p-43f) g_quantum += 1;
	}
	(void) any_pos;
	for (int zs = kPlus; zs <= kInput; ++zs) for (int zin = 0; zin < 2; ++zin) {
		const Domain scaled(s, true, (ZeroSign) zs);
		run_tile(scaled, ref, qry, zin ? -0.0f : 0.0f, sc, sm);
		for (size_t i = 0; i < pc.size(); ++i) {
			const Masks &a = pm[i], &b = sm[i];
			CHECK(a.eL == b.eL && a.eU == b.eU && a.eG == b.eG && a.nD == b.nD && a.nI == b.nI,
			      "%s cell (%zu, %zu) masks %d%d%d %d%d vs %d%d%d %d%d (zero %d, in %d; match %a mismatch %a)", what, i / W, i % W,
			      a.eL, a.eU, a.eG, a.nD, a.nI, b.eL, b.eU, b.eG, b.nD, b.nI, zs, zin, s.mat, s.mis);
			CHECK(!(sc[i].S > 1.0f), "%s: scaled score above the clamp", what);
			CHECK(sc[i].S == 0.0f || std::fpclassify(sc[i].S) == FP_NORMAL, "%s: scaled score %a is subnormal", what, sc[i].S);
			const float back = sc[i].S * kScoreUnscale;
			if (zs == kPlus || pc[i].S != 0.0f) CHECK(bits(back) == bits(pc[i].S), "%s cell (%zu, %zu): %a scaled back vs %a (zero %d, in %d)", what, i / W, i % W, back, pc[i].S, zs, zin);
			else CHECK(back == 0.0f, "%s cell (%zu, %zu): %a scaled back vs zero", what, i / W, i % W, back);
		}
	}
	g_cells += (long) pc.size();
	g_tiles += 1;
}

static bool tile_has_positive(const Sc &s, const std::string &ref, const std::string &qry) {
	std::vector<Cell> pc; std::vector<Masks> pm;
	run_tile(Domain(s, false, kPlus), ref, qry, 0.0f, pc, pm);
	for (const Cell &c : pc) if (c.S > 0.0f) return true;
	return false;
}

static void test_tiles() {
	uint64_t rs = 0x2545f4914f6cdd1dull;
	auto rnd = [&]() { rs ^= rs << 13; rs ^= rs >> 7; rs ^= rs << 17; return (uint32_t) (rs >> 32); };
	auto random_seq = [&](int n) { std::string q; for (int i = 0; i < n; ++i) q.push_back("ACGT"[rnd() & 3]); return q; };
	auto mutate = [&](const std::string &r, unsigned per_mille) {
		std::string q;
		for (char c : r) {
			const unsigned u = rnd() % 1000;
			if (u < per_mille / 3) continue;                                          /* deletion */
			if (u < 2 * per_mille / 3) { q.push_back("ACGT"[rnd() & 3]); q.push_back(c); continue; }      /* insertion */
			q.push_back(u < per_mille ? "ACGT"[rnd() & 3] : c);
		}
		if (q.size() > 64) q.resize(64);
		if (q.empty()) q = "A";
		return q;
	};
	std::vector<Sc> all(kScorings, kScorings + sizeof(kScorings) / sizeof(kScorings[0]));
	all.insert(all.end(), kEdgeScorings, kEdgeScorings + sizeof(kEdgeScorings) / sizeof(kEdgeScorings[0]));
	for (const Sc &s : all) {
		CHECK(score_scale_exact(s.mat, s.mis, 0.0f, s.go, s.ge, s.gem, s.decay), "scoring match %a mismatch %a must be admitted", s.mat, s.mis);
		/* random tiles: clean, noisy and unrelated pairs, odd shapes */
		for (int k = 0; k < 24; ++k) {
			const std::string ref = random_seq(5 + (int) (rnd() % 60));
			const std::string qry = (k % 4 == 3) ? random_seq(3 + (int) (rnd() % 62)) : mutate(ref, 50 + 150 * (unsigned) (k % 3));
			compare_tile(s, ref, qry, "random");
		}
		/* engineered: a gap that runs through zero-score cells along a whole row (deletion) and a whole column (insertion): a lead
		 * that scores exactly -gap_open where the scoring allows one (the default: four matches, a mismatch, a match), then 56
		 * bases of 'T' on one side only */
		const std::string flank = "ACGGACGACCAG";
		compare_tile(s, std::string("ACGACG") + std::string(56, 'T') + flank.substr(0, 2), std::string("ACGAAG") + flank.substr(0, 2), "zero run D");
		compare_tile(s, std::string("ACGAAG") + flank.substr(0, 2), std::string("ACGACG") + std::string(56, 'T') + flank.substr(0, 2), "zero run I");
		/* long mismatch stretches between matching blocks: the score returns to zero again and again */
		{
			std::string ref, qry;
			for (int b = 0; b < 5; ++b) { const std::string blk = random_seq(4 + b); ref += blk + "AAAAAAA"; qry += blk + "CCCCCCC"; }
			ref.resize(60); qry.resize(60);
			compare_tile(s, ref, qry, "returns to zero");
		}
		/* no positive score anywhere; and one whose only positive score is a single match */
		compare_tile(s, std::string(40, 'A'), std::string(33, 'C'), "no positive score");
		CHECK(!tile_has_positive(s, std::string(40, 'A'), std::string(33, 'C')), "the all-mismatch tile has a positive score");
		compare_tile(s, std::string(20, 'A') + "G" + std::string(20, 'A'), std::string(15, 'C') + "G" + std::string(15, 'C'), "one match");
		/* alternating match / mismatch: under the edge scorings the score after each pair is a small multiple of the quantum */
		{
			std::string ref, qry;
			for (int i = 0; i < 48; ++i) { ref.push_back("ACGT"[i & 3]); qry.push_back((i & 1) ? (ref.back() == 'A' ? 'C' : 'A') : ref.back()); }
			compare_tile(s, ref, qry, "alternating");
		}
	}
	CHECK(g_zero_ext >= 100, "only %ld zero-score extensions", g_zero_ext);
	CHECK(g_quantum >= 100, "only %ld cells at the quantum", g_quantum);
	printf("tiles: %ld tiles, %ld cells x 6 scaled runs; %ld zero-score extensions, %ld cells within one quantum of zero\n", g_tiles, g_cells, g_zero_ext, g_quantum);
}

static void test_predicate() {
	const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN(), sub = 0x1p-130f;
	for (const Sc &s : kScorings) {
		CHECK(score_scale_exact(s.mat, s.mis, 0.0f, s.go, s.ge, s.gem, s.decay), "preset / fuzz scoring refused (match %g mismatch %g)", s.mat, s.mis);
		CHECK(score_scale_exact(s.mat, s.mis, twin_mismatch_x(s.mis), s.go, s.ge, s.gem, s.decay), "twin scoring refused (match %g mismatch %g)", s.mat, s.mis);
	}
	const Sc d = kScorings[0];
	CHECK(!score_scale_exact(0x1p21f, d.mis, 0.0f, d.go, d.ge, d.gem, d.decay), "match 2^21");
	CHECK(score_scale_exact(0x1.fffffep20f, d.mis, 0.0f, d.go, d.ge, d.gem, d.decay), "match just below 2^21");
	CHECK(!score_scale_exact(0x1p-21f, d.mis, 0.0f, d.go, d.ge, d.gem, d.decay), "match 2^-21");
	CHECK(score_scale_exact(0x1p-20f, d.mis, 0.0f, d.go, d.ge, d.gem, d.decay), "match 2^-20");
	CHECK(!score_scale_exact(d.mat, -0x1p-21f, 0.0f, d.go, d.ge, d.gem, d.decay), "mismatch -2^-21");
	CHECK(!score_scale_exact(d.mat, d.mis, -0x1p22f, d.go, d.ge, d.gem, d.decay), "x mismatch -2^22");
	CHECK(!score_scale_exact(d.mat, d.mis, 0.0f, -0x1p21f, d.ge, d.gem, d.decay), "gap open -2^21");
	for (const float v : {sub, -sub, inf, -inf, nan}) {
		CHECK(!score_scale_exact(v, d.mis, 0.0f, d.go, d.ge, d.gem, d.decay), "match %a", v);
		CHECK(!score_scale_exact(d.mat, v, 0.0f, d.go, d.ge, d.gem, d.decay), "mismatch %a", v);
		CHECK(!score_scale_exact(d.mat, d.mis, 0.0f, v, d.ge, d.gem, d.decay), "gap open %a", v);
		/* (gap_extend_min = +inf or NaN: min() returns the other operand, the table holds no such value) */
		if (v != inf && !std::isnan(v)) CHECK(!score_scale_exact(d.mat, d.mis, 0.0f, d.go, d.ge, v, d.decay), "gap_extend_min %a", v);
	}
	/* a decay that takes a table entry out of the range: -5 + 20 * 0.25 is an exact zero (admitted: zero is always exact), but
	 * -5 + run * 0.2499999 passes within 2^-21 of zero at run 20 */
	CHECK(score_scale_exact(d.mat, d.mis, 0.0f, d.go, -5.0f, 1.0f, 0.25f), "exact zero in the table");
	CHECK(!score_scale_exact(d.mat, d.mis, 0.0f, d.go, -5.0f, 1.0f, 0.24999999f), "a table entry of magnitude below 2^-20");
	CHECK(!score_scale_exact(d.mat, d.mis, 0.0f, d.go, -0x1p20f, -1.0f, -0x1p16f), "a table entry of magnitude above 2^21");
	/* for every admitted scoring the table scaled and scaled back is the table, and no scaled entry is subnormal */
	std::vector<Sc> all(kScorings, kScorings + sizeof(kScorings) / sizeof(kScorings[0]));
	all.insert(all.end(), kEdgeScorings, kEdgeScorings + sizeof(kEdgeScorings) / sizeof(kEdgeScorings[0]));
	uint64_t rs = 88172645463325252ull;
	auto rnd = [&]() { rs ^= rs << 13; rs ^= rs >> 7; rs ^= rs << 17; return (uint32_t) (rs >> 32); };
	for (int k = 0; k < 2000; ++k) {      /* random scorings across the range and beyond it */
		auto val = [&](bool neg) { const float m = 1.0f + (float) (rnd() & 0x7fffff) * 0x1p-23f; const float v = ldexpf(m, (int) (rnd() % 50) - 25); return neg ? -v : v; };
		all.push_back(Sc{val(false), val(true), val(true), val(true), val(true), (rnd() & 1) ? 0.0f : fabsf(val(false))});
	}
	int admitted = 0;
	for (const Sc &s : all) {
		if (!score_scale_exact(s.mat, s.mis, 0.0f, s.go, s.ge, s.gem, s.decay)) continue;
		admitted += 1;
		for (const float v : {s.mat, s.mis, s.go}) {
			volatile float sv = v * kScoreScale;
			CHECK(bits(sv * kScoreUnscale) == bits(v) && (v == 0.0f || std::fpclassify((float) sv) == FP_NORMAL), "value %a", v);
		}
		for (int e = 0; e < kPenPairs; ++e) {
			const float pen = fminf(s.gem, s.ge + (float) e * s.decay);
			volatile float sp = pen * kScoreScale;
			CHECK(bits(sp * kScoreUnscale) == bits(pen), "entry %d: %a scaled and back is %a", e, pen, sp * kScoreUnscale);
			CHECK(pen == 0.0f || std::fpclassify((float) sp) == FP_NORMAL, "entry %d: %a scaled is not normal", e, pen);
		}
	}
	CHECK(admitted >= 100 && admitted < (int) all.size(), "%d of %zu scorings admitted", admitted, all.size());
	printf("predicate: %d of %zu scorings admitted\n", admitted, all.size());
}

int main() {
	test_tiles();
	test_predicate();
	if (g_bad) { printf("cell_scale_equiv_test: %d FAILED\n", g_bad); return 1; }
	printf("cell_scale_equiv_test: ok\n");
	return 0;
}
