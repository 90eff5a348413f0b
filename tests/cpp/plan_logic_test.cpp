/*
 * plan_logic_test -- the corridor analysis of plan_kernel on the host (ngmlr_amd/csrc/cvx_plan_logic.h): the strip form
 * (plan_kernel<256>) and the on-demand form (plan_kernel<64>) against the brute-force restatement, field for field.
 *
 *   plan_logic_test                    the corridor families below; prints one line per family, exit status 1 on a difference
 *   plan_logic_test --plans IN OUT     the brute-force plans of the corridors described in IN, as TilePlan records
 *                                      (tests/test_gpu_plan_records.py compares the device's records with them)
 *
 * IN: int32 n, uint64 max_matrix_mb, then per tile int32 fmt, W, H, width, off0, float k, d, right and, for
 * fmt = kRowsExplicit, H pairs of int32 (offset, length).
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "cvx_plan_logic.h"

using namespace cvx;

struct Corridor {
	int fmt = kRowsAffine, W = 0, H = 0, width = 0, off0 = 0;
	float k = 1.0f, d = 0.0f, right = 0.0f;
	std::vector<RowDesc2> rows;      /* kRowsExplicit */
	std::string tag;
	PlanRows view() const {
		PlanRows p;
		p.rows = rows.data(); p.fmt = fmt; p.width = width; p.off0 = off0; p.k = k; p.d = d; p.right = right;
		return p;
	}
};

static const unsigned long long kMaxMb = 10000;

static bool same(const TilePlan &a, const TilePlan &b) {
	return a.r0 == b.r0 && a.rend == b.rend && a.need == b.need && a.flags == b.flags && a.cells == b.cells && a.active == b.active;
}
static void show(const char *what, const TilePlan &p) {
	printf("    %-9s r0 %d rend %d need %d flags %d cells %llu active %llu\n", what, p.r0, p.rend, p.need, p.flags,
			(unsigned long long) p.cells, (unsigned long long) p.active);
}

struct Tally { int tiles = 0, bad = 0, irregular = 0, empty = 0, wrap = 0, beyond_stretch = 0; };

static void check(const Corridor &c, Tally &t, unsigned long long max_mb = kMaxMb) {
	const PlanRows p = c.view();
	const TilePlan want = plan_tile_brute(p, c.W, c.H, max_mb);
	const TilePlan strips = plan_tile_strips(p, c.W, c.H, max_mb);
	const TilePlan ondemand = plan_tile_ondemand(p, c.W, c.H, max_mb);
	t.tiles += 1;
	t.irregular += (want.flags & kPlanIrregular) != 0;
	t.empty += (want.flags & kPlanEmpty) != 0;
	t.wrap += (want.flags & kPlanWrap16) != 0;
	t.beyond_stretch += want.need > kPlanAhead + 1;
	if (!same(want, strips) || !same(want, ondemand)) {
		if (t.bad < 5) {
			printf("  DIFFERENT: %s (fmt %d W %d H %d width %d off0 %d k %.9g d %.9g right %.9g)\n", c.tag.c_str(), c.fmt, c.W, c.H, c.width, c.off0, c.k, c.d, c.right);
			show("brute", want); show("strips", strips); show("on demand", ondemand);
		}
		t.bad += 1;
	}
}

static Corridor affine(int H, int W, float k, float d, float right, int width, const char *tag) {
	Corridor c;
	c.fmt = kRowsAffine; c.H = H; c.W = W; c.k = k; c.d = d; c.right = right; c.width = width; c.tag = tag;
	return c;
}
static Corridor constant(int H, int W, int off0, int width, const char *tag) {
	Corridor c;
	c.fmt = kRowsConst; c.H = H; c.W = W; c.off0 = off0; c.width = width; c.tag = tag;
	return c;
}
/* the rows of a closed form written out, then bent by the caller */
static Corridor explicit_from(const Corridor &src, const char *tag) {
	Corridor c;
	c.fmt = kRowsExplicit; c.H = src.H; c.W = src.W; c.tag = tag;
	const PlanRows p = src.view();
	for (int y = 0; y < src.H; ++y) c.rows.push_back(plan_row_at(p, y));
	return c;
}

static const int kHeights[] = { 1, 2, 63, 64, 65, 255, 256, 257, kPlanStrip - 1, kPlanStrip, kPlanStrip + 1, kPlanStrip + kPlanAhead,
		kPlanStrip + kPlanAhead + 1, 2 * kPlanStrip + 3 };
static const float kSlopes[] = { 0.5f, 0.957f, 1.0f, 1.045f, 2.0f };
static const int kWidths[] = { 1, 40, 340, 369, 420, 2048, 8192 };

static int report(const char *family, const Tally &t) {
	printf("%-34s %5d tiles, %4d irregular, %4d empty, %3d wrap16, %4d with need beyond the staged stretch: %s\n", family, t.tiles, t.irregular, t.empty,
			t.wrap, t.beyond_stretch, t.bad ? "DIFFERENT" : "equal");
	return t.bad;
}

static int self_test() {
	int bad = 0;
	{	/* the reference's corridor builders: endpoints (d = width / 2, no shift) and anchors (d = 0, a shift to the right); the window
		 * as long as the read asks for, and a fifth shorter so that rows are clipped on the right for most of the tile */
		Tally t;
		for (float k : kSlopes) for (int w : kWidths) for (int H : kHeights) {
			const int W = (int) ((float) H / k) + 1;
			check(affine(H, W, k, (float) w / 2.0f, 0.0f, w, "endpoints"), t);
			check(affine(H, W, k, 0.0f, (float) w * 0.55f, w, "anchors"), t);
			check(affine(H, W - W / 5, k, (float) w / 2.0f, 0.0f, w, "endpoints, short window"), t);
			check(affine(H, W + 3 * w, k, 0.0f, (float) -w, w, "anchors, starts inside"), t);
		}
		bad += report("affine closed forms", t);
	}
	{
		Tally t;
		for (int off0 : { -700, -10, 0, 50 }) for (int w : kWidths) for (int H : kHeights) {
			check(constant(H, 600, off0, w, "constant"), t);
			check(constant(H, H + w, off0, w, "constant, wide window"), t);
		}
		bad += report("constant corridors", t);
	}
	{
		Tally t;
		for (int H : kHeights) for (int w : { 40, 369, 700 }) {
			const Corridor base = affine(H, H + 1, 1.0f, (float) w / 2.0f, 0.0f, w, "");
			Corridor c = explicit_from(base, "one decreasing row start");
			if (H > 2) c.rows[H / 2].x -= 3;
			check(c, t);
			c = explicit_from(base, "one row start that stays");
			if (H > 2) c.rows[H / 2].x = c.rows[H / 2 - 1].x - 1;
			check(c, t);
			c = explicit_from(base, "a shrinking row end");
			if (H > 2) c.rows[(2 * H) / 3].y -= 5;
			check(c, t);
			c = explicit_from(base, "zero-length rows");
			for (int y = 0; y < H; y += 7) c.rows[y].y = 0;
			check(c, t);
			c = explicit_from(base, "negative lengths");
			for (int y = 3; y < H; y += 11) c.rows[y].y = -2;
			check(c, t);
			c = explicit_from(base, "entirely right of the window");
			for (int y = 0; y < H; ++y) c.rows[y].x += H + w + 10;
			check(c, t);
			c = explicit_from(base, "entirely left of the window");
			for (int y = 0; y < H; ++y) c.rows[y].x -= H + 2 * w + 10;
			check(c, t);
			c = explicit_from(base, "zigzag");
			for (int y = 0; y < H; ++y) if (y % 50 >= 25) c.rows[y].x -= 60;
			check(c, t);
			c = explicit_from(base, "ragged lengths");
			for (int y = 0; y < H; ++y) c.rows[y].y += (y % 7) * 3;
			check(c, t);
			check(explicit_from(base, "regular, as arrays"), t);
		}
		Corridor none;
		none.fmt = kRowsExplicit; none.H = 0; none.W = 100; none.tag = "no rows";
		check(none, t);
		bad += report("explicit rows", t);
	}
	{	/* H > 32767: the insertion-extent search and kPlanWrap16 */
		Tally t;
		check(affine(40000, 40400, 0.99f, 200.0f, 0.0f, 400, "tall"), t);
		check(affine(40000, 40400, 0.99f, 200.0f, 0.0f, 400, "tall, refused by size"), t, 10);
		Corridor c;      /* a band that runs straight down for 33 000 rows: a column that long can carry an insertion past SHRT_MAX */
		c.fmt = kRowsExplicit; c.H = 40000; c.W = 8000; c.tag = "tall, vertical stretch";
		for (int y = 0; y < c.H; ++y) {
			RowDesc2 r;
			r.x = y < 3000 ? y - 200 : y < 36000 ? 2800 : y - 33200;
			r.y = 400;
			c.rows.push_back(r);
		}
		check(c, t);
		c.tag = "tall, irregular";
		c.rows[20000].x -= 5;
		check(c, t);
		check(constant(40000, 500, 0, 33000, "tall, rows past SHRT_MAX"), t);
		bad += report("40 000 rows", t);
		if (t.wrap < 3) { printf("  the tall corridors do not reach kPlanWrap16\n"); bad += 1; }
	}
	{
		Tally t;
		std::mt19937_64 rng(20251);
		auto uni = [&](int lo, int hi) { return (int) (lo + (long long) (rng() % (unsigned long long) (hi - lo + 1))); };
		for (int i = 0; i < 2000; ++i) {
			const int H = (i % 5 == 0) ? uni(1, 4000) : uni(1, 900);
			const float k = 0.4f + (float) uni(0, 1700) / 1000.0f;
			const int w = (i % 9 == 0) ? uni(1, 1500) : uni(1, 450);
			const int W = (int) ((float) H / k) + uni(-H / 4, H / 4 + 40);
			Corridor c;
			switch (i % 4) {
			case 0: c = affine(H, W < 1 ? 1 : W, k, (float) w / 2.0f, 0.0f, w, "random endpoints"); break;
			case 1: c = affine(H, W < 1 ? 1 : W, k, 0.0f, (float) uni(-w, 2 * w) + 0.25f * (float) uni(0, 3), w, "random anchors"); break;
			case 2: c = constant(H, W < 1 ? 1 : W, uni(-w, 60), w, "random constant"); break;
			default: {
				c = explicit_from(affine(H, W < 1 ? 1 : W, k, (float) w / 2.0f, 0.0f, w, ""), "random rows");
				const int jitter = (i % 8 == 3) ? 0 : uni(1, 40);      /* half of them stay regular but for their lengths */
				for (int y = 0; y < H; ++y) {
					if (jitter) c.rows[y].x += uni(-jitter, jitter);
					c.rows[y].y += (i % 16 == 7) ? uni(-w, 20) : uni(0, 20);
				}
				if (!jitter) for (int y = 1; y < H; ++y) {      /* lengths that never let a row end before the one above */
					const long long pe = (long long) c.rows[y - 1].x + c.rows[y - 1].y;
					if ((long long) c.rows[y].x + c.rows[y].y < pe) c.rows[y].y = (int) (pe - c.rows[y].x);
				}
			}
			}
			check(c, t);
		}
		bad += report("2 000 random corridors", t);
	}
	printf(bad ? "FAILED: %d corridors differ\n" : "ok\n", bad);
	return bad ? 1 : 0;
}

static int plans_mode(const char *in_path, const char *out_path) {
	FILE *in = fopen(in_path, "rb");
	if (!in) { perror(in_path); return 2; }
	int32_t n = 0;
	uint64_t max_mb = 0;
	if (fread(&n, 4, 1, in) != 1 || fread(&max_mb, 8, 1, in) != 1 || n < 0) { fprintf(stderr, "%s: bad header\n", in_path); return 2; }
	std::vector<TilePlan> out;
	for (int i = 0; i < n; ++i) {
		int32_t hdr[5];
		float f[3];
		if (fread(hdr, 4, 5, in) != 5 || fread(f, 4, 3, in) != 3) { fprintf(stderr, "%s: tile %d truncated\n", in_path, i); return 2; }
		Corridor c;
		c.fmt = hdr[0]; c.W = hdr[1]; c.H = hdr[2]; c.width = hdr[3]; c.off0 = hdr[4];
		c.k = f[0]; c.d = f[1]; c.right = f[2];
		if (c.H < 0 || (c.fmt != kRowsExplicit && c.fmt != kRowsAffine && c.fmt != kRowsConst)) { fprintf(stderr, "%s: tile %d malformed\n", in_path, i); return 2; }
		if (c.fmt == kRowsExplicit) {
			c.rows.resize((size_t) c.H);
			if (c.H && fread(c.rows.data(), sizeof(RowDesc2), (size_t) c.H, in) != (size_t) c.H) { fprintf(stderr, "%s: rows of tile %d truncated\n", in_path, i); return 2; }
		}
		out.push_back(plan_tile_brute(c.view(), c.W, c.H, max_mb));
	}
	fclose(in);
	FILE *o = fopen(out_path, "wb");
	if (!o) { perror(out_path); return 2; }
	static_assert(sizeof(TilePlan) == 32, "TilePlan is written as it is");
	if (n && fwrite(out.data(), sizeof(TilePlan), (size_t) n, o) != (size_t) n) { perror(out_path); return 2; }
	fclose(o);
	return 0;
}

int main(int argc, char **argv) {
	if (argc == 4 && strcmp(argv[1], "--plans") == 0) return plans_mode(argv[2], argv[3]);
	if (argc != 1) { fprintf(stderr, "usage: plan_logic_test [--plans IN OUT]\n"); return 2; }
	return self_test();
}
