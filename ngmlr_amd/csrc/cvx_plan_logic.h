/*
 * cvx_plan_logic.h -- the per-tile corridor analysis of plan_kernel (cvx_kernels.hip) as plain functions compiled
 * for the device and for the host, so that the CPU suite runs the very code the kernel runs
 * (tests/cpp/plan_logic_test.cpp), beside a brute-force restatement straight from the definitions.
 *
 * What a tile's plan says (TilePlan, cvx_types.h): the first and one-past-last anti-diagonal with a cell, the
 * cells of the corridor and those inside [0, W), whether the ring schedule applies (row starts increase, row ends
 * do not decrease), whether a gap run can pass SHRT_MAX, and `need`: the ring slots the fill needs -- for every
 * row y the rows from y up to the first row that starts at or after ge(y) + kSwitchMargin, inclusive.
 *
 * Two forms of the per-row work:
 *   plan_row_ondemand  every row the analysis looks at is evaluated where it is needed: row y, row y - 1 again
 *                      and about four probes of the search -- for a closed-form corridor a correctly rounded
 *                      binary32 divide each.  plan_kernel<64> (a wave per short tile) runs this.
 *   plan_row_staged    the spans of a strip of rows and of a stretch behind it are evaluated once, into a ring
 *                      of kPlanCap entries (LDS on the device, an array on the host), and everything is taken
 *                      from there: one evaluation per row.  Only a search that runs past the staged stretch
 *                      evaluates rows on demand.  plan_kernel<256> runs this.
 * Both run ONE search (plan_first_row_at), probe for probe, and a probe answers the same wherever the span comes
 * from -- so the two agree on every tile, also on one whose row starts are not monotone, where `need` is whatever
 * that search arrives at.
 */
#ifndef CVX_PLAN_LOGIC_H
#define CVX_PLAN_LOGIC_H

#include <stdint.h>

#include "cvx_types.h"

#if defined(__HIPCC__)
#define CVX_HD __host__ __device__ inline
#else
#define CVX_HD inline
#endif

namespace cvx {

/* rows of a strip, and the stretch behind the strip that is staged with it; the ring holds a strip, the stretch and the
 * row above the strip (a power of two: the ring index is a mask) */
static const int kPlanStrip = 1536;
static const int kPlanAhead = 511;
static const int kPlanCap = 2048;
static_assert(kPlanCap == kPlanStrip + kPlanAhead + 1 && (kPlanCap & (kPlanCap - 1)) == 0, "ring = strip + stretch behind it + the row above");

/* the rows of one tile wherever they live (the host's RowView) */
struct PlanRows {
	const RowDesc2 *rows;  /* kRowsDelta8 / kRowsExplicit: the tile's slice of the rows arena */
	int32_t fmt, width, off0;
	float k, d, right;
};

CVX_HD RowDesc2 plan_row_at(const PlanRows &p, const int y) {
	RowDesc2 r;
	if (p.fmt == kRowsAffine || p.fmt == kRowsConst) {
		r.x = p.fmt == kRowsConst ? p.off0 : affine_row_offset(y, p.d, p.k, p.right);
		r.y = p.width;
	} else {
		r = p.rows[y];
	}
	return r;
}
/* a row's length alone: no evaluation for a closed form */
CVX_HD int32_t plan_row_len(const PlanRows &p, const int y) {
	return (p.fmt == kRowsAffine || p.fmt == kRowsConst) ? p.width : p.rows[y].y;
}

/* gs(y): anti-diagonal of the first cell of row y; ge(y): one past the last.
 * Row y covers x in [max(0,off), min(off+len, W))  (src/ConvexAlignFast.cpp:948-950). */
CVX_HD void plan_row_span(const RowDesc2 ol, const int W, const int y, int &gs, int &ge) {
	long long lo = ol.x > 0 ? ol.x : 0;
	long long hi = (long long) ol.x + (long long) ol.y;
	if (hi > W) hi = W;
	if (hi < lo) hi = lo;
	gs = (int) (lo + y);
	ge = (int) (hi + y);
}

struct PlanAcc {           /* what the rows of a tile add up to; every member combines by sum, maximum, minimum or OR */
	unsigned long long cells, active;
	int need, flags, maxlen, rendmax, r0min;
};
CVX_HD PlanAcc plan_acc_init() {
	PlanAcc a;
	a.cells = 0; a.active = 0; a.need = 1; a.flags = 0; a.maxlen = 0; a.rendmax = -0x7fffffff; a.r0min = 0x7fffffff;
	return a;
}

/* first row y' > y that starts at or after lim (starts_before(yy): gs(yy) < lim; gs is increasing in a regular
 * corridor): gallop out from a guess -- row starts advance by about two anti-diagonals per row in a sloped corridor --
 * then bisect; a handful of probes instead of log2(H) */
template <typename Pred>
CVX_HD int plan_first_row_at(const int y, const int gs, const int lim, const int H, Pred starts_before) {
	int lo = y + 1, hi = H;                  /* rows < lo start before lim, rows >= hi do not */
	int g = y + 1 + ((lim - gs) >> 1);
	g = g < lo ? lo : g;
	if (g < hi) {
		if (starts_before(g)) {
			lo = g + 1;
			for (int step = 1; lo < hi; step <<= 1) {
				const int p = (lo + step - 1 < hi) ? lo + step - 1 : hi - 1;
				if (starts_before(p)) lo = p + 1; else { hi = p; break; }
			}
		} else {
			hi = g;
			for (int step = 1; lo < hi; step <<= 1) {
				const int p = (hi - step > lo) ? hi - step : lo;
				if (starts_before(p)) { lo = p + 1; break; } else hi = p;
			}
		}
	}
	while (lo < hi) {
		const int mid = (lo + hi) >> 1;
		if (starts_before(mid)) lo = mid + 1; else hi = mid;
	}
	return lo;
}

/* H > 32767 only.  How long can a gap run get in this corridor?  A deletion run stays inside one row (<= its length); an
 * insertion run stays inside one column, i.e. inside the consecutive rows that contain it: for the last column of row y
 * those are the rows up to the first one that starts at or behind hi(y) (row starts do not decrease in a regular
 * corridor).  Only when such a stretch exceeds SHRT_MAX can the reference's `short indelRun` wrap
 * (src/AlignmentMatrixFast.h:43) and the int16-emulating kernels are needed -- a 100 kb read on a 350-column corridor
 * never gets there, and the float-run kernels are three times as fast.  -> rows the last column of row y can run through */
CVX_HD int plan_insertion_extent(const PlanRows &p, const int W, const int H, const int y) {
	const RowDesc2 ol = plan_row_at(p, y);
	long long lo_y = ol.x > 0 ? ol.x : 0;
	long long hi_y = (long long) ol.x + (long long) ol.y;
	if (hi_y > W) hi_y = W;
	if (hi_y < lo_y) hi_y = lo_y;
	int a = y + 1, b = H;                    /* rows < a start before hi(y), rows >= b do not */
	while (a < b) {
		const int mid = (a + b) >> 1;
		const RowDesc2 om = plan_row_at(p, mid);
		const long long lo_m = om.x > 0 ? om.x : 0;
		if (lo_m < hi_y) a = mid + 1; else b = mid;
	}
	return a - y;
}

/* one row's share of the plan, given its span, the span of the row above and its length */
template <typename Pred>
CVX_HD void plan_row_common(PlanAcc &a, const PlanRows &p, const int W, const int H, const int y, const int len,
		const int gs, const int ge, const int pgs, const int pge, const int lim, Pred starts_before) {
	a.cells += (unsigned long long) (long long) len;
	a.active += (unsigned long long) (ge - gs);
	if (len > a.maxlen) a.maxlen = len;
	if (ge > a.rendmax) a.rendmax = ge;
	if (gs < a.r0min) a.r0min = gs;
	if (y > 0) {
		if (gs <= pgs) a.flags |= kPlanIrregular;  /* ring schedule needs increasing row starts */
		/* ... and rows that end in order: the fill hands slots over in row order (its staged row
		 * records are overwritten on that assumption).  True for every corridor the reference builds
		 * (one width, offsets that never decrease); a corridor whose rows shrink goes to the catch-all kernel. */
		if (ge < pge) a.flags |= kPlanIrregular;
	}
	const int n = plan_first_row_at(y, gs, lim, H, starts_before) - y + 1;
	if (n > a.need) a.need = n;
	if (H > 32767) {
		const int ext = plan_insertion_extent(p, W, H, y);
		if (ext > a.maxlen) a.maxlen = ext;      /* folded into the same maximum: either kind of run past 32767 needs the wrap kernels */
	}
}

CVX_HD void plan_row_ondemand(PlanAcc &a, const PlanRows &p, const int W, const int H, const int y) {
	const RowDesc2 ol = plan_row_at(p, y);
	int gs, ge, pgs = 0, pge = 0;
	plan_row_span(ol, W, y, gs, ge);
	if (y > 0) plan_row_span(plan_row_at(p, y - 1), W, y - 1, pgs, pge);
	const int lim = ge + kSwitchMargin;
	plan_row_common(a, p, W, H, y, ol.y, gs, ge, pgs, pge, lim, [&](const int yy) {
		int mgs, mge;
		plan_row_span(plan_row_at(p, yy), W, yy, mgs, mge);
		return mgs < lim;
	});
}

/* the ring: row r of the tile at entry r & (kPlanCap - 1) */
CVX_HD void plan_stage_row(const PlanRows &p, const int W, const int r, int *ring_gs, int *ring_ge) {
	int gs, ge;
	plan_row_span(plan_row_at(p, r), W, r, gs, ge);
	ring_gs[r & (kPlanCap - 1)] = gs;
	ring_ge[r & (kPlanCap - 1)] = ge;
}
/* rows [y - 1, staged) are in the ring (staged > y) */
CVX_HD void plan_row_staged(PlanAcc &a, const PlanRows &p, const int W, const int H, const int y, const int staged,
		const int *ring_gs, const int *ring_ge) {
	const int gs = ring_gs[y & (kPlanCap - 1)], ge = ring_ge[y & (kPlanCap - 1)];
	const int pgs = y > 0 ? ring_gs[(y - 1) & (kPlanCap - 1)] : 0, pge = y > 0 ? ring_ge[(y - 1) & (kPlanCap - 1)] : 0;
	const int lim = ge + kSwitchMargin;
	plan_row_common(a, p, W, H, y, plan_row_len(p, y), gs, ge, pgs, pge, lim, [&](const int yy) {
		if (yy < staged) return ring_gs[yy & (kPlanCap - 1)] < lim;
		int mgs, mge;                        /* a corridor so wide that the search leaves the staged stretch */
		plan_row_span(plan_row_at(p, yy), W, yy, mgs, mge);
		return mgs < lim;
	});
}
/* the strips of a tile: strip s = rows [s * kPlanStrip, ...); before its rows are worked on, the rows up to plan_strip_staged()
 * are in the ring -- those the strip before left there stay (the ring has room for the row above the strip, the strip and
 * the stretch behind it, so what this strip's staging overwrites lies two rows or more above it) */
CVX_HD int plan_strip_staged(const int Y, const int H) {
	const long long e = (long long) Y + kPlanStrip + kPlanAhead;
	return e < H ? (int) e : H;
}

/* the record, from what the rows added up to */
CVX_HD TilePlan plan_finish(const PlanAcc &a, const int H, const unsigned long long max_matrix_mb) {
	TilePlan p;
	p.cells = a.cells;
	p.active = a.active;
	p.need = a.need;
	int f = a.flags;
	int r0 = 0, rend = 0;
	if (H > 0) { r0 = a.r0min; rend = a.rendmax; }   /* first / one-past-last anti-diagonal with a cell */
	if (H <= 0 || a.active == 0) f |= kPlanEmpty;
	/* src/AlignmentMatrixFast.cpp:45: (ulong)(matrixSize / 1000.0f / 1000.0f) < maxMatrixSizeMB */
	const float mb = (float) a.cells / 1000.0f / 1000.0f;
	if (!((unsigned long long) mb < max_matrix_mb)) f |= kPlanTooLarge;
	/* longest possible deletion (row length) or insertion (column extent, rows above) run; the column bound needs
	 * row starts that do not decrease, so an irregular corridor that tall keeps the old rule */
	if (a.maxlen > 32767 || (H > 32767 && (f & kPlanIrregular))) f |= kPlanWrap16;
	p.r0 = r0;
	p.rend = rend;
	p.flags = f;
	return p;
}

#if !defined(__HIP_DEVICE_COMPILE__)
/* ---- the host's whole-tile forms (tests; nothing in the product plans on the host) */

/* what plan_kernel<256> computes: strip by strip through the ring, here a plain array */
inline TilePlan plan_tile_strips(const PlanRows &p, const int W, const int H, const unsigned long long max_matrix_mb) {
	static thread_local int ring_gs[kPlanCap], ring_ge[kPlanCap];
	PlanAcc a = plan_acc_init();
	int staged = 0;
	for (int Y = 0; Y < H; Y += kPlanStrip) {
		const int end = plan_strip_staged(Y, H);
		for (int r = staged; r < end; ++r) plan_stage_row(p, W, r, ring_gs, ring_ge);
		staged = end;
		const int yend = (long long) Y + kPlanStrip < H ? Y + kPlanStrip : H;
		for (int y = Y; y < yend; ++y) plan_row_staged(a, p, W, H, y, staged, ring_gs, ring_ge);
	}
	return plan_finish(a, H, max_matrix_mb);
}

/* what plan_kernel<64> computes */
inline TilePlan plan_tile_ondemand(const PlanRows &p, const int W, const int H, const unsigned long long max_matrix_mb) {
	PlanAcc a = plan_acc_init();
	for (int y = 0; y < H; ++y) plan_row_ondemand(a, p, W, H, y);
	return plan_finish(a, H, max_matrix_mb);
}

/* The yardstick: the definitions, by linear scans over the rows -- no guesses, no strips, no bisection.  `need` of a
 * corridor whose row starts are not increasing has no definition of its own (such a tile runs on the catch-all kernel,
 * which sizes its scratch by it): it is what the search above arrives at on rows evaluated where they are asked for. */
inline TilePlan plan_tile_brute(const PlanRows &p, const int W, const int H, const unsigned long long max_matrix_mb) {
	PlanAcc a = plan_acc_init();
	bool irregular = false;
	for (int y = 1; y < H; ++y) {
		int gs, ge, pgs, pge;
		plan_row_span(plan_row_at(p, y), W, y, gs, ge);
		plan_row_span(plan_row_at(p, y - 1), W, y - 1, pgs, pge);
		if (gs <= pgs || ge < pge) irregular = true;
	}
	if (irregular) a.flags |= kPlanIrregular;
	for (int y = 0; y < H; ++y) {
		const RowDesc2 ol = plan_row_at(p, y);
		int gs, ge;
		plan_row_span(ol, W, y, gs, ge);
		a.cells += (unsigned long long) (long long) ol.y;
		a.active += (unsigned long long) (ge - gs);
		if (ol.y > a.maxlen) a.maxlen = ol.y;
		if (ge > a.rendmax) a.rendmax = ge;
		if (gs < a.r0min) a.r0min = gs;
		const int lim = ge + kSwitchMargin;
		int first = H;
		if (!irregular) {
			for (int yy = y + 1; yy < H; ++yy) {
				int mgs, mge;
				plan_row_span(plan_row_at(p, yy), W, yy, mgs, mge);
				if (mgs >= lim) { first = yy; break; }
			}
		} else {
			first = plan_first_row_at(y, gs, lim, H, [&](const int yy) {
				int mgs, mge;
				plan_row_span(plan_row_at(p, yy), W, yy, mgs, mge);
				return mgs < lim;
			});
		}
		if (first - y + 1 > a.need) a.need = first - y + 1;
		if (H > 32767) {
			/* rows below y whose first column lies left of the end of row y, counted while they follow one another */
			long long hi_y = (long long) ol.x + (long long) ol.y;
			const long long lo_y = ol.x > 0 ? ol.x : 0;
			if (hi_y > W) hi_y = W;
			if (hi_y < lo_y) hi_y = lo_y;
			int ext;
			if (!irregular) {
				int yy = y + 1;
				while (yy < H) {
					const RowDesc2 om = plan_row_at(p, yy);
					if (!((om.x > 0 ? om.x : 0) < hi_y)) break;
					++yy;
				}
				ext = yy - y;
			} else {
				ext = plan_insertion_extent(p, W, H, y);      /* (no definition of its own either; the flag is set whatever it says) */
			}
			if (ext > a.maxlen) a.maxlen = ext;
		}
	}
	return plan_finish(a, H, max_matrix_mb);
}
#endif

}  // namespace cvx

#endif
