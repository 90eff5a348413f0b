// CPU test of the scalar twin's share of the host logic (ngmlr_amd/csrc/cvx_host_logic.h): which fill a handle's scoring gets in
// either mode (fill_semantics), the twin's mismatch against 'x' (twin_mismatch_x), and the kernel classes host_plan gives a
// twin handle's tiles.  Built with plain g++ by tests/test_twin_fixtures_cpu.py.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "cvx_host_logic.h"

using namespace cvx;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

static PlanTuning tuning_of(const FillSemantics &s, const bool gangs_knob) {
	// as the runtime fills it in: cvx_create_ex clears the gang knob of a handle whose semantics build no gangs
	PlanTuning t;
	t.force_generic = s.force_generic ? 1 : 0;
	t.no_gangs = (gangs_knob && !s.no_gangs) ? 0 : 1;
	return t;
}

int main() {
	// ---------------------------------------------------------------- fill semantics
	{	// the default scoring: rings in both modes; the twin has no gangs and no matrix cap
		const FillSemantics d = fill_semantics(2.0f, -5.0f, -5.0f, -5.0f, -1.0f, 0.15f, false);
		const FillSemantics t = fill_semantics(2.0f, -5.0f, -5.0f, -5.0f, -1.0f, 0.15f, true);
		CHECK(d.ring_signs && !d.sse_variant && !d.force_generic && !d.no_gangs && d.matrix_cap);
		CHECK(t.ring_signs && !t.sse_variant && !t.force_generic && t.no_gangs && !t.matrix_cap);
	}
	// outside the fast regime (gap_open + gap_ext_min >= mismatch) with the rings' sign structure intact: a default handle takes the
	// SSE variant of the catch-all kernel, a twin handle the rings
	const float outside[4][6] = { {2.0f, -10.0f, -5.0f, -5.0f, -1.0f, 0.15f}, {1.0f, -4.0f, -2.0f, -2.0f, -1.0f, 0.05f},
			{3.0f, -2.0f, -1.0f, -4.0f, -0.5f, 0.3f}, {2.0f, -6.0f, -5.0f, -5.0f, -1.0f, 0.15f} };
	for (const float *p : outside) {
		const FillSemantics d = fill_semantics(p[0], p[1], p[2], p[3], p[4], p[5], false);
		const FillSemantics t = fill_semantics(p[0], p[1], p[2], p[3], p[4], p[5], true);
		CHECK(d.ring_signs && d.sse_variant && d.force_generic);
		CHECK(t.ring_signs && !t.sse_variant && !t.force_generic);
	}
	// each of the seven sign clauses broken in turn: no rings for anybody; the twin takes the catch-all kernel with SCALAR rules
	const float broken[7][6] = { {0.0f, -5.0f, -5.0f, -5.0f, -1.0f, 0.15f}, {2.0f, 0.0f, -5.0f, -5.0f, -1.0f, 0.15f},
			{2.0f, -5.0f, 0.0f, -5.0f, -1.0f, 0.15f}, {2.0f, -5.0f, -5.0f, 0.5f, 1.0f, 0.15f}, {2.0f, -5.0f, -5.0f, -5.0f, 0.0f, 0.15f},
			{2.0f, -5.0f, -5.0f, -5.0f, -1.0f, -0.1f}, {2.0f, -5.0f, -5.0f, -1.0f, -3.0f, 0.15f} };
	for (const float *p : broken) {
		const FillSemantics d = fill_semantics(p[0], p[1], p[2], p[3], p[4], p[5], false);
		const FillSemantics t = fill_semantics(p[0], p[1], p[2], p[3], p[4], p[5], true);
		CHECK(!d.ring_signs && d.sse_variant && d.force_generic);
		CHECK(!t.ring_signs && !t.sse_variant && t.force_generic);
	}
	// ---------------------------------------------------------------- mismatch against 'x': one binary32 multiply
	{
		CHECK(twin_mismatch_x(-5.0f) == -500.0f && twin_mismatch_x(-10.0f) == -1000.0f);
		const float vals[] = {-0.1f, -4.3f, -1e-3f, -7.77f, -3.3333333f};
		for (const float v : vals) {
			volatile float a = v;
			volatile float single = a * 100.0f;                       // rounded once, to binary32
			const float got = twin_mismatch_x(v);
			CHECK(memcmp(&got, (const void *) &single, 4) == 0);
		}
		// (where the double product rounds to another float the two differ: the reference multiplies in binary32)
		volatile float a = -0.1f;
		CHECK((double) twin_mismatch_x(-0.1f) != (double) a * 100.0);
	}
	// ---------------------------------------------------------------- kernel classes of a twin handle's tiles
	{
		const FillSemantics d = fill_semantics(2.0f, -5.0f, -5.0f, -5.0f, -1.0f, 0.15f, false);
		const FillSemantics t = fill_semantics(2.0f, -5.0f, -5.0f, -5.0f, -1.0f, 0.15f, true);
		const int H = 900, W = 1000, w = 600;              // slope-1 band of 300 live rows: a gang's ring, or 64-row blocks
		std::vector<RowDesc> rows((size_t) H);
		for (int y = 0; y < H; ++y) { rows[(size_t) y].off = y - w / 2; rows[(size_t) y].len = w; }
		TilePlan p[3]; memset(p, 0, sizeof(p));
		TileIn in[3]; memset(in, 0, sizeof(in));
		for (int i = 0; i < 3; ++i) {
			p[i].r0 = 0; p[i].rend = (H - 1) + W; p[i].cells = (uint64_t) H * w; p[i].active = p[i].cells;
			in[i].H = H; in[i].W = W; in[i].row_off = 0;
		}
		p[0].need = 300;                                   // wider than the widest one-wave ring (256)
		p[1].need = 170;                                   // an M = 3 ring
		p[2].need = 150; p[2].flags = kPlanIrregular;      // no ring kernel
		// (small_batch = 1 below: three tiles are not treated as a batch too small to fill the device)
		HostPlan hp;
		{ PlanTuning tn = tuning_of(d, true); tn.small_batch = 1; host_plan(3, p, in, rows.data(), tn, hp); }
		CHECK(hp.n_chained == 0 && hp.n_fast == 2 && hp.generic.size() == 1 && hp.trun[0].mnw == 3 && hp.trun[1].mnw == 3);
		CHECK(hp.trun[0].ring == 384);                     // the gang of two waves, for a default handle that asks for gangs
		{ PlanTuning tn = tuning_of(t, true); tn.small_batch = 1; host_plan(3, p, in, rows.data(), tn, hp); }
		CHECK(hp.n_chained == 1 && hp.n_fast == 1 && hp.generic.size() == 1);      // the twin handle ignores the gang knob: chained
		CHECK(hp.trun[0].chain_nblk > 1 && hp.trun[1].mnw == 3 && hp.trun[1].ring == 192 && hp.generic[0] == 2);
		for (size_t c = 0; c < hp.cls.size(); ++c) if (!hp.cls[c].empty()) CHECK(kClasses[c / 2].gang == 1);
		// a twin handle whose scoring lacks the sign structure: everything to the catch-all kernel
		const FillSemantics g = fill_semantics(2.0f, -5.0f, -5.0f, -1.0f, -3.0f, 0.15f, true);
		{ PlanTuning tn = tuning_of(g, true); tn.small_batch = 1; host_plan(3, p, in, rows.data(), tn, hp); }
		CHECK(hp.n_chained == 0 && hp.n_fast == 0 && hp.generic.size() == 3);
	}
	if (fails) { printf("twin_host_logic_test: %d checks failed\n", fails); return 1; }
	printf("twin_host_logic_test: ok\n");
	return 0;
}
