/*
 * cvx_kernels.hip -- hand-written gfx950 (CDNA4, wave64) kernels for ngmlr's
 * convex-gap banded Smith-Waterman.  gfx950 only: no other target, no dual paths.
 *
 *   plan_kernel       per-tile corridor analysis (AlignmentMatrixFast::prepare,
 *                     reference src/AlignmentMatrixFast.cpp:30-60, plus what the
 *                     anti-diagonal schedule needs: ring size, first/last diagonal)
 *   fill_ring_kernel  forward fill (fwdFillMatrixSSESimple == scalar recurrence of
 *                     reference src/ConvexAlignFast.cpp:606-774), anti-diagonal
 *                     wavefront, one wave per tile (per row block for chained tiles)
 *   backtrack_kernel  revBacktrack + validPath (src/ConvexAlignFast.cpp:335-432,
 *                     src/AlignmentMatrixFast.cpp:213-220)
 *   compact_ops_kernel  gathers the per-tile op regions into one dense arena
 *
 * Parallel scheme of the fill (see DESIGN.md for the derivation).  Cells on one
 * anti-diagonal r = x + y are independent: (x,y) needs left (x-1,y) and up (x,y-1)
 * from r-1 and diag (x-1,y-1) from r-2.  A wave keeps read ROWS in a ring of
 * N = 64*M slots, row y in slot y mod N, M consecutive slots per lane.  Per step
 * every slot advances its row by one column, so "left" is the slot's own previous
 * value (a register), "up" is the previous slot's value (a register for M-1 of the M
 * slots, one DPP wave_ror:1 for the lane boundary) and "diag" is the up value the
 * slot saw one step earlier.  Row state never touches LDS or HBM; the only HBM
 * traffic is one reference character per cell (L1/L2 resident) in, and the 2-bit
 * direction codes out (two bit-plane words per slot per 32 steps, 2N dwords).
 * The recurrence's priority chain runs on 64-bit lane masks in SGPRs (SALU), so the
 * VALU only sees the float adds/max/compares and a few selects per cell.
 *
 * Floating point: scores are IEEE binary32, every * and + rounded separately as in
 * the reference's scalar and SSE code (compile with -ffp-contract=off).
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cvx_types.h"
#include "cvx_launch.h"
#include "cvx_plan_logic.h"

namespace cvx {

#define CVX_DEV __device__ __forceinline__

/* lane i <- lane (i-1) mod 64 : DPP wave_ror:1 (GFX9 DPP_WF_RR1 = 0x13C) */
CVX_DEV int rot1_i(int v) {
	return __builtin_amdgcn_update_dpp(0, v, 0x13C, 0xf, 0xf, true);
}
CVX_DEV float rot1_f(float v) {
	return __int_as_float(rot1_i(__float_as_int(v)));
}

/* ------------------------------------------------------------------ plan */

/* The per-tile logic is cvx_plan_logic.h (compiled for the host too: tests/cpp/plan_logic_test.cpp); here the threads of a
 * tile share its rows out and combine what they add up to.
 *
 * TPT threads per tile, 256 / TPT tiles per workgroup: 256 for batches of long reads, 64 (a wave
 * per tile) for batches of short ones, where a 256-thread group per 150-row tile was mostly idle
 * threads and workgroup launches (short-read config: 1.7 of 8.9 ms per 100 000 tiles).
 *
 * TPT = 256 stages the row spans of a strip in LDS and evaluates every row once (plan_row_staged); TPT = 64 keeps the
 * on-demand form (plan_row_ondemand: about six evaluations per row): its tiles are a few hundred rows, four of them
 * share a workgroup, and a ring per tile would cost the kernel its occupancy for rows that are few anyway. */
template <int TPT>
__global__ void __launch_bounds__(256)
plan_kernel(const int2 *rows, const RowSrc *rsrc, const TileIn *tin, TilePlan *plan, int n_tiles, unsigned long long max_matrix_mb) {
	constexpr int TPB = 256 / TPT;                 /* tiles per block */
	const int sub = threadIdx.x / TPT;             /* tile slot inside the block */
	const int ltid = threadIdx.x % TPT;
	const int t = blockIdx.x * TPB + sub;
	const bool live = t < n_tiles;
	const TileIn ti = tin[live ? t : 0];
	/* rows of a closed-form corridor are evaluated in registers: the analysis of such a tile reads nothing
	 * but its 32-byte description -- it used to read 8 H bytes a handful of times (3.5 ms per 49 152 PacBio tiles, and
	 * most of a fill's duration when it ran beside one) */
	const RowSrc rs = rsrc[live ? t : 0];
	PlanRows pr;
	pr.rows = reinterpret_cast<const RowDesc2 *>(rows) + ti.row_off;
	pr.fmt = rs.fmt; pr.width = rs.width; pr.off0 = rs.off0;
	pr.k = rs.k; pr.d = rs.d; pr.right = rs.right;
	const int H = live ? ti.H : 0, W = ti.W;

	__shared__ unsigned long long s_cells[TPB], s_active[TPB];
	__shared__ int s_need[TPB], s_flags[TPB], s_maxlen[TPB], s_rend[TPB], s_r0[TPB];
	if (ltid == 0) { s_cells[sub] = 0; s_active[sub] = 0; s_need[sub] = 1; s_flags[sub] = 0; s_maxlen[sub] = 0; s_rend[sub] = -0x7fffffff; s_r0[sub] = 0x7fffffff; }
	__syncthreads();

	PlanAcc acc = plan_acc_init();
	if constexpr (TPT == 256) {
		/* (one tile per workgroup: H is uniform, every thread meets every barrier) */
		__shared__ int s_gs[kPlanCap], s_ge[kPlanCap];
		int staged = 0;
		for (int Y = 0; Y < H; Y += kPlanStrip) {
			const int end = plan_strip_staged(Y, H);
			__syncthreads();                       /* the strip before has been read */
			for (int r = staged + ltid; r < end; r += TPT) plan_stage_row(pr, W, r, s_gs, s_ge);
			staged = end;
			__syncthreads();
			const int yend = min(H, Y + kPlanStrip);
			for (int y = Y + ltid; y < yend; y += TPT) plan_row_staged(acc, pr, W, H, y, staged, s_gs, s_ge);
		}
	} else {
		for (int y = ltid; y < H; y += TPT) plan_row_ondemand(acc, pr, W, H, y);
	}
	if (H > 0) {
		atomicAdd(&s_cells[sub], acc.cells);
		atomicAdd(&s_active[sub], acc.active);
		atomicMax(&s_need[sub], acc.need);
		atomicOr(&s_flags[sub], acc.flags);
		atomicMax(&s_maxlen[sub], acc.maxlen);
		atomicMax(&s_rend[sub], acc.rendmax);
		atomicMin(&s_r0[sub], acc.r0min);
	}
	__syncthreads();

	if (ltid == 0 && live) {
		PlanAcc all;
		all.cells = s_cells[sub]; all.active = s_active[sub]; all.need = s_need[sub]; all.flags = s_flags[sub];
		all.maxlen = s_maxlen[sub]; all.rendmax = s_rend[sub]; all.r0min = s_r0[sub];
		plan[t] = plan_finish(all, H, max_matrix_mb);
	}
}

/* ------------------------------------------------------------------ rows */

/* Rebuilds the (offset, length) rows arena from what travelled over PCIe (RowSrc, cvx_types.h): one
 * signed step byte per row -- a running sum per tile: wave scans plus a carry, 256 rows per pass -- or
 * the rows verbatim for the tiles that do not fit that form.  The result is exactly the caller's
 * CorridorLine[] minus offsetInMatrix; everything downstream reads this arena as before. */
__global__ void __launch_bounds__(64)
expand_rows_kernel(const RowSrc *rsrc, const TileIn *tin, const uint8_t *delta, const int2 *rowsx, int2 *rows, int n_tiles, int closed_forms) {
	/* one wave per tile, 64 rows per pass, the running offset in a register: no LDS, no barrier -- the
	 * kernel runs on the upload stream beside the previous batch's fill, where a workgroup barrier per
	 * 256 rows cost it tens of ms (measured: 46 ms average in the pipelined bench, 1.6 ms alone) */
	const int t = blockIdx.x;
	if (t >= n_tiles) return;
	const int lane = threadIdx.x;
	const RowSrc rs = rsrc[t];
	const TileIn ti = tin[t];
	const int H = ti.H;
	int2 *out = rows + ti.row_off;
	if (rs.fmt == kRowsExplicit) {
		const int2 *src = rowsx + rs.src_off;
		for (int y = lane; y < H; y += 64) out[y] = src[y];
		return;
	}
	if ((rs.fmt == kRowsAffine || rs.fmt == kRowsConst) && !closed_forms) return;      /* evaluated in registers wherever a row is needed (RowView) */
	if (rs.fmt == kRowsAffine) {
		/* the reference's corridor builders in closed form (cvx_types.h affine_row_offset; src/AlignmentBuffer.cpp:107-127,
		 * 178-191, 68-82): binary32 subtract, correctly rounded divide, subtract, truncation -- row by row, no carried state */
		for (int y = lane; y < H; y += 64) out[y] = make_int2(affine_row_offset(y, rs.d, rs.k, rs.right), rs.width);
		return;
	}
	if (rs.fmt == kRowsConst) {
		for (int y = lane; y < H; y += 64) out[y] = make_int2(rs.off0, rs.width);
		return;
	}
	const int8_t *d = reinterpret_cast<const int8_t *>(delta + rs.src_off);
	int carry = rs.off0;
	for (int y0 = 0; y0 < H; y0 += 64) {
		const int y = y0 + lane;
		int v = (y < H && y > 0) ? (int) d[y] : 0;
#pragma unroll
		for (int k = 1; k < 64; k <<= 1) {
			const int u = __shfl_up(v, k, 64);
			if (lane >= k) v += u;
		}
		if (y < H) out[y] = make_int2(carry + v, rs.width);
		carry += __builtin_amdgcn_readlane(v, 63);
	}
}

/* ------------------------------------------------------------------ fill */

typedef unsigned long long u64;

/* per-lane predicate <-> wave-uniform 64-bit lane mask (SGPR pair) */
CVX_DEV u64 ballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }
/* A wave-uniform value that is needed in a rare path of a long loop (row staging, the direction flush): handed through an
 * "s" constraint at its use, so that it lives in a scalar register across the loop instead of in a vector register the
 * allocator then spills to scratch and reloads inside the loop (round 5: 26 spilled dwords, +16 GB of HBM traffic per launch) */
CVX_DEV int in_sgpr(int v) { v = __builtin_amdgcn_readfirstlane(v); asm volatile("" : "+s"(v)); return v; }
CVX_DEV float in_sgpr(float v) { return __int_as_float(in_sgpr(__float_as_int(v))); }
CVX_DEV unsigned in_sgpr(unsigned v) { return (unsigned) in_sgpr((int) v); }
CVX_DEV u64 in_sgpr(u64 u) { return ((u64) in_sgpr((unsigned) (u >> 32)) << 32) | (u64) in_sgpr((unsigned) u); }
template <typename T> CVX_DEV T *in_sgpr(T *p) {
	const u64 u = (u64) p;
	const unsigned lo = (unsigned) in_sgpr((int) (unsigned) u), hi = (unsigned) in_sgpr((int) (unsigned) (u >> 32));
	return (T *) (((u64) hi << 32) | (u64) lo);
}
CVX_DEV bool lanes(u64 m) { return __builtin_amdgcn_inverse_ballot_w64(m); }
/* A lane mask that inline assembly wrote to an SGPR pair: the compiler takes the outputs of an asm with a vector output for
 * per-lane values and would move the mask logic behind them to the VALU; readfirstlane of a scalar register is a copy it folds away */
CVX_DEV u64 asm_mask(u64 m) {
	return ((u64) (unsigned) __builtin_amdgcn_readfirstlane((int) (unsigned) (m >> 32)) << 32) | (u64) (unsigned) __builtin_amdgcn_readfirstlane((int) (unsigned) m);
}
/* mask of lane i <- mask of lane (i-1) mod 64 : the SALU twin of wave_ror:1 */
CVX_DEV u64 rot1_m(u64 m) { return (m << 1) | (m >> 63); }
/* acc = (acc << 1) | (lane's bit of m): one v_addc_co_u32 with the mask as carry-in.
 * m must come from SALU mask logic (it does: planes are s_or_b64 results). */
CVX_DEV unsigned shl1_in(unsigned acc, u64 m) {
	/* the (unused) carry-out goes to an SGPR pair of the compiler's choice, not to VCC: in that form the
	 * instruction issues beside a full-rate VALU op like any other half-rate one; with VCC as its
	 * destination it does not (profiles/r03_ubench_pipes.txt, kinds 15-18) */
	u64 carry_out;
	asm volatile("v_addc_co_u32_e64 %0, %1, %0, %0, %2" : "+v"(acc), "=s"(carry_out) : "s"(m));
	return acc;
}

/* ------------------------------------------------------------------ backtrack */

/* validPath, src/AlignmentMatrixFast.cpp:213-220: float arithmetic, int truncation,
 * no contraction.  A cell (x, row) is valid iff minC < x < maxC. */
CVX_DEV void valid_bounds(const int off, const int width, int &minC, int &maxC) {
	minC = (int) ((float) off + 0.1f * (float) width);
	maxC = (int) ((float) (minC + width) - 0.1f * (float) width);
}

/* direction code of bit `bit` of a plane pair: plane 0 = gap (I or D), plane 1 = the cell
 * consumes a read base on the way back (I or diagonal) */
CVX_DEV unsigned plane_code(const unsigned wx, const unsigned wy, const int bit) {
	const unsigned px = (wx >> bit) & 1u, py = (wy >> bit) & 1u;
	return px ? (py ? 1u : 2u) : (py ? 3u : 0u);
}

/*
 * revBacktrack (src/ConvexAlignFast.cpp:335-432) by ONE wave, run-skipping.  The path is
 * a chain of runs (diagonal runs broken by short gaps); instead of one dependent load per
 * cell, the 64 lanes probe the next 64 cells along the current direction at once (lane i
 * looks at the i-th cell back), a ballot finds how far the run goes, and the walk jumps to
 * its end.  Every probe is four coalesced loads (corridor rows, plane words, both sequences).
 * The gap that ends a diagonal run is then resolved from the SAME probe whenever the words
 * already in registers cover it (a deletion run lies in one lane's word, an insertion run in
 * the words of the following lanes), so a 10-kb PacBio tile costs ~1 500 probes instead of
 * ~20 000 dependent steps.  The walk state is wave-uniform; lane 0 writes the run-length ops.
 * `o` carries the argmax in (score, best_x, best_y) and returns the FwdResults.
 */
template <bool CHAINED>
CVX_DEV void backtrack_walk(const int lane, const int H, const int N, const int r0, const int ops_cap,
		const RowView &rows, const uint2 *dirs, const ChainBlk *blk, const uint8_t *ref, const uint8_t *qry, int *ops, TileOut &o) {
	/* make the walk's state provably wave-uniform so that it runs on scalar branches */
	const int best_x = __builtin_amdgcn_readfirstlane(o.best_x);
	const int best_y = __builtin_amdgcn_readfirstlane(o.best_y);
	/* src/ConvexAlignFast.cpp:338 */
	if (best_y <= 0) { o.status = 1; return; }

	const int qend = (H - best_y) - 1;
	int idx = ops_cap - 1;
	int elem = 4;          /* CIGAR_S: the trailing clip is tracked but not stored */
	int elem_len = qend;
	int consumed = qend;
	int x = best_x, y = best_y;
	int s = y % N;         /* ring slot of row y */
	int status = 0;
	unsigned want = 3u;    /* direction of the run being followed (first probe: a guess) */

	/* revBacktrack's run-length bookkeeping (src/ConvexAlignFast.cpp:395-403) */
	auto emit = [&](int cur, int n) {
		if (n <= 0) return;
		if (cur == elem) {
			elem_len += n;
		} else {
			if (elem != 4) { if (lane == 0) ops[idx] = (elem_len << 4) | elem; idx -= 1; }
			elem = cur;
			elem_len = n;
		}
	};

	/* every probe either consumes a cell or fixes the direction, so x + y + 2 probes always
	 * suffice; the cap turns corrupted direction data into an invalid tile, never a hang */
	int budget = 2 * (best_x + best_y) + 8;
	for (;;) {
		if (--budget < 0) { status = 3; break; }
		const int dx = (want != 1u) ? 1 : 0, dy = (want != 2u) ? 1 : 0;
		const int cx = x - lane * dx, cy = y - lane * dy;
		const bool inside = (cx >= 0 && cy >= 0);
		const int lx = cx > 0 ? cx : 0, ly = cy > 0 ? cy : 0;
		int sl = s - lane * dy;
		if (sl < 0) sl += N;
		const int tt = cx + cy - r0;
		const int ttc = tt > 0 ? tt : 0;
		const RowDesc2 ol = row_at(rows, ly);
		uint2 w;
		if (CHAINED) {
			/* row block of the probed cell -> its own region of direction words (N is a power of two here) */
			const int gb = ly / N;
			const ChainBlk cb = blk[gb];
			int wr = (ttc >> 5) - cb.tblk0;
			wr = wr < 0 ? 0 : (wr >= cb.nblk32 ? cb.nblk32 - 1 : wr);      /* cells outside their row are masked below */
			w = dirs[cb.dir_off + (size_t) wr * N + (size_t) (ly - gb * N)];
		} else {
			w = dirs[(size_t) (ttc >> 5) * N + sl];
		}
		const int rc = ref[lx], qc = qry[ly];
		/* used by every probe on purpose: keeps all four loads in one round trip */
		const u64 eqm = ballot(rc == qc);
		/* getDirection, src/AlignmentMatrixFast.cpp:185-195: outside -> STOP */
		const bool in_row = inside && tt >= 0 && cx >= ol.x && cx < ol.x + ol.y;
		unsigned code = plane_code(w.x, w.y, 31 - (ttc & 31));
		if (!in_row) code = 0u;
		int minC, maxC;
		valid_bounds(ol.x, ol.y, minC, maxC);

		const u64 run = ballot(code == want);
		const int L = (~run == 0ull) ? 64 : __builtin_ctzll(~run);   /* cells of this run */
		const u64 low = (L == 64) ? ~0ull : ((1ull << L) - 1ull);
		/* every visited cell must pass validPath before the move (:368-373) */
		const u64 vp = ballot(cx > minC && cx < maxC);
		if ((~vp & low) != 0ull) { status = 2; break; }

		if (want == 3u) {
			int pos = 0;
			while (pos < L) {
				const int isq = (int) ((eqm >> pos) & 1ull);
				const u64 m = (isq ? ~eqm : eqm) >> pos;
				int rl = (m == 0ull) ? 64 - pos : __builtin_ctzll(m);
				if (rl > L - pos) rl = L - pos;
				emit(isq ? 7 : 8, rl);
				pos += rl;
			}
			x -= L; y -= L; consumed += L;
		} else if (want == 1u) {
			emit(1, L);
			y -= L; consumed += L;
		} else {
			emit(2, L);
			x -= L;
		}
		if (want != 2u) { s -= L; if (s < 0) s += N; }
		if (L == 64) continue;
		const unsigned nxt = (unsigned) __builtin_amdgcn_readlane((int) code, L);
		if (nxt == 0u) break;     /* CIGAR_STOP (or outside the matrix) */
		if (want != 3u) { want = nxt; continue; }

		/* A diagonal run ended in a gap at (x, y) = lane L's cell.  Follow the gap run inside the
		 * words this probe already holds; whatever they do not cover goes to the next probe. */
		const int tp = x + y - r0;                       /* step index of (x, y), >= 0 inside a row */
		if (nxt == 2u) {
			/* deletion run: same row, earlier steps = higher bits of lane L's word */
			const unsigned wx = (unsigned) __builtin_amdgcn_readlane((int) w.x, L);
			const unsigned wy = (unsigned) __builtin_amdgcn_readlane((int) w.y, L);
			const int row_lo = max(__builtin_amdgcn_readlane(ol.x, L), 0);
			const int b0 = 31 - (tp & 31);
			const unsigned dm = (wx & ~wy) >> b0;        /* bit k: cell (x - k, y) is D; bit 0 is set */
			int Ld = (~dm == 0u) ? 32 : __builtin_ctz(~dm);   /* <= 32 - b0: the shift filled in zeros */
			const int in_word = 32 - b0;
			const int in_rowc = x - row_lo + 1;          /* cells down to the start of the row */
			if (Ld > in_rowc) Ld = in_rowc;
			const int rminC = __builtin_amdgcn_readlane(minC, L), rmaxC = __builtin_amdgcn_readlane(maxC, L);
			if (!(x - (Ld - 1) > rminC && x < rmaxC)) { status = 2; break; }
			emit(2, Ld);
			x -= Ld;
			if (Ld == in_rowc) break;                    /* next cell is left of the row: STOP */
			if (Ld == in_word) { want = 2u; continue; }  /* the run may go on in the previous word */
			const unsigned c2 = plane_code(wx, wy, b0 + Ld);
			if (c2 == 0u) break;
			want = c2;
		} else {
			/* insertion run: same column, cell k is in lane L+k's row and slot; it is step tp - k,
			 * which that lane's word covers unless a 32-step boundary lies in between */
			const int k = lane - L;
			const int tn = tp - k;
			const bool have = (k >= 0) && (cy >= 0) && (tn >= 0) && ((tn >> 5) == (ttc >> 5));
			const bool col_in = (x >= ol.x) && (x < ol.x + ol.y);
			unsigned c2 = plane_code(w.x, w.y, 31 - (tn & 31));
			if (!col_in) c2 = 0u;
			const u64 im = ballot(have && c2 == 1u) >> L;       /* bit k: cell (x, y - k) is I; bit 0 is set */
			const int Li = (~im == 0ull) ? 64 : __builtin_ctzll(~im);   /* <= 64 - L */
			const u64 ilow = (Li == 64) ? ~0ull : ((1ull << Li) - 1ull);
			const u64 vpi = ballot(x > minC && x < maxC) >> L;
			if ((~vpi & ilow) != 0ull) { status = 2; break; }
			emit(1, Li);
			y -= Li; consumed += Li;
			s -= Li; if (s < 0) s += N;
			const int e = L + Li;
			want = 1u;                                   /* default: let the next probe look again */
			if (e < 64 && ((ballot(have) >> e) & 1ull) != 0ull) {
				const unsigned c3 = (unsigned) __builtin_amdgcn_readlane((int) c2, e);
				if (c3 == 0u) break;
				want = c3;
			}
		}
	}
	if (status == 0) {
		if (elem != 4) { if (lane == 0) ops[idx] = (elem_len << 4) | elem; idx -= 1; }
		consumed += (y + 1);
		o.ref_position = x + 1;
		o.qstart = y + 1;
		o.qend = qend;
		o.ops_first = idx + 1;
		o.n_ops = ops_cap - 1 - idx;
		if (H != consumed) status = 3;
	}
	o.status = status;
}

/* first cell of the tile in (y, x) order: *fy = -1 when no row has a cell inside [0, W).
 * Rare path (a tile without any positive score), run by backtrack_kernel. */
CVX_DEV void first_cell(const RowView &rows, int H, int W, int lane, int *fy, int *fx) {
	*fy = -1;
	*fx = 0;
	for (int y0 = 0; y0 < H; y0 += 64) {
		const int yy = y0 + lane;
		bool has = false;
		int lo_i = 0;
		if (yy < H) {
			const RowDesc2 ol = row_at(rows, yy);
			long long lo = ol.x > 0 ? ol.x : 0;
			long long hi = (long long) ol.x + (long long) ol.y;
			if (hi > W) hi = W;
			has = hi > lo;
			lo_i = (int) lo;
		}
		const unsigned long long m = __builtin_amdgcn_ballot_w64(has);
		if (m != 0ull) {
			const int l = __builtin_ctzll(m);
			*fy = y0 + l;
			*fx = __builtin_amdgcn_readlane(lo_i, l);
			return;
		}
	}
}


template <bool WRAP> struct RunT { typedef float type; };
template <> struct RunT<true> { typedef int type; };
template <bool B> struct BoolTag { static constexpr bool value = B; };

/* Occupancy target, waves per SIMD as (min, max) of amdgpu_waves_per_eu.  The M = 3 kernels (corridors of 310-370 columns, i.e.
 * almost every PacBio/ONT tile) ask for exactly six (80 VGPRs, the few spilled values are tile constants outside the step loop;
 * ~14 % faster than at the five the allocator picks by itself), and for seven in the FAST form (TAB without a gang,
 * cvx_fill_ring.inc: 72 VGPRs, 4 KB of LDS per wave -- the PacBio launch).  The other classes keep the default. */
constexpr int fill_waves_min(const int m, const bool fast) { return m == 3 ? (fast ? 7 : 6) : 1; }
constexpr int fill_waves_max(const int m, const bool fast) { return m == 3 ? (fast ? 7 : 6) : 8; }
#define CVX_FILL_OCC(M, FAST) __attribute__((amdgpu_waves_per_eu(fill_waves_min(M, FAST), fill_waves_max(M, FAST))))

/* gang: s_sleep argument of a wave that waits for its neighbour's record (x 64 clocks) */
constexpr int kGangWaitSleep = 1;

/* What a cell that extends a gap offers: src/ConvexAlignFast.cpp:669-675, E = (score == 0) ? 0 : score + pen with
 * pen = min(gap_ext_min, gap_ext + run * decay).  score >= 0 and pen < 0, so this is max(score + pen, score * -2^100):
 * -0 for score 0 (compares equal to the reference's +0 and never reaches an output), score + pen otherwise.  One
 * function for the cell update and for the consumer of a chained block's boundary records, which rebuilds the up
 * candidate from (score, run) with exactly these operations. */
CVX_DEV float gap_extend_value(const float sc, const float runf, const float gem, const float gext, const float decay) {
	const float pen = fminf(gem, gext + runf * decay);
	return fmaxf(sc + pen, sc * -0x1p100f);
}

enum FillMode { kFillTwoPhase = 0, kFillExact = 1, kFillChain = 2 };

/*
 * One wave per tile: block b takes tile list[b].  The list is in LPT order and the hardware
 * dispatches workgroups in index order as wave slots free up, which is the work queue a
 * persistent kernel would build by hand -- without the atomic cursor and without a tile loop
 * around the step loop.
 *
 * Best-cell tracking (src/ConvexAlignFast.cpp:758-763: first strict maximum in (y, x) order)
 * is two-phase.  Exact (score, step, row) tracking costs three half-rate VALU ops per cell; the
 * best cell of an alignment that reaches the end of the read lies in the last few anti-
 * diagonals, so the kFillTwoPhase instantiation only keeps a per-lane running maximum
 * (2 ops per M cells) up to the last `late` groups and tracks exactly from there on.  The
 * late result is the tile's answer iff it strictly beats every earlier score; otherwise the
 * tile is flagged (TileOut::pad = kPadRedo) and the kFillExact instantiation, launched right
 * behind on the same stream over the same list, redoes just the flagged tiles with exact
 * tracking from the first step.
 *
 * kFillChain: corridors with more live rows than the widest ring (need > 256: the retry loop's
 * widened corridors up to 8192 columns, full-matrix inversion tiles) are cut into blocks of N
 * consecutive read rows; block g is an ordinary ring tile whose first row takes its "up" inputs
 * from the boundary stream that block g-1 writes while it computes its last row.  Blocks of one
 * tile run concurrently on different CUs, each a few hundred steps behind its predecessor
 * (about need / N of them at a time), so a wide tile is spread over many CUs instead of living
 * in one workgroup.  A wave takes the next task from a ticket counter (tasks are listed in
 * dependency order, so the producer of anything a wave waits for is always running or done);
 * the boundary is a stream of self-validating 8-byte records (BoundaryRec: score, run, insertion bit,
 * launch epoch) written with device-scope atomic stores as the last row advances and read kChainChunk
 * steps ahead of their use -- no counter, no release fence in the producer, no round trip to memory on
 * the consumer's critical path while the producer is ahead (it starts 2 N anti-diagonals earlier).
 */
#define CVX_FILL_KERNEL fill_ring_kernel
#define CVX_FILL_TWIN false
#include "cvx_fill_ring.inc"
#undef CVX_FILL_KERNEL
#undef CVX_FILL_TWIN
/* the scalar twin's forms (every one-wave form; gangs are not built for it: pick_fill) */
#define CVX_FILL_KERNEL fill_ring_twin_kernel
#define CVX_FILL_TWIN true
#include "cvx_fill_ring.inc"
#undef CVX_FILL_KERNEL
#undef CVX_FILL_TWIN

/* A tile record read by a whole wave: lane i fetches dword i, fields come back as SGPRs
 * through v_readlane: three VGPRs instead of one per field. */
CVX_DEV int rec_load(const void *rec, const int n_dwords, const int lane) {
	return lane < n_dwords ? reinterpret_cast<const int *>(rec)[lane] : 0;
}
CVX_DEV int fld(const int w, const int k) { return __builtin_amdgcn_readlane(w, k); }
CVX_DEV unsigned long long fld64(const int w, const int k) {
	return ((unsigned long long) (unsigned) fld(w, k + 1) << 32) | (unsigned) fld(w, k);
}

/* backtrack of one tile by one wave (nothing to do for skipped, invalid or already walked tiles) */
CVX_DEV void walk_tile(const BacktrackArgs &a, const int t, const int lane) {
	static_assert(sizeof(TileRun) == 48 && sizeof(TileIn) == 32 && sizeof(TileOut) == 40, "record layout");
	const int wr = rec_load(a.trun + t, 12, lane);   /* dir_off 0-1, ops_off 2-3, ring 4, ops_cap 5, r0 6, nsteps 7, skip 8, mnw 9, chain_blk0 10 */
	const int wo = rec_load(a.tout + t, 10, lane);   /* score 0, status 1, best_x 2, best_y 3, ..., pad 9 */
	if (fld(wr, 8) != 0) return;
	TileOut o;
	o.score = __int_as_float(fld(wo, 0));
	o.status = fld(wo, 1);
	o.best_x = fld(wo, 2); o.best_y = fld(wo, 3);
	o.ref_position = 0; o.qstart = 0; o.qend = 0; o.n_ops = 0; o.ops_first = 0;
	o.pad = fld(wo, 9);
	if (o.status != 0 || o.pad != 0) return;
	const int wi = rec_load(a.tin + t, 8, lane);     /* ref_off 0, qry_off 1, W 2, H 3, row_off 4-5 */
	const int H = fld(wi, 3), W = fld(wi, 2);
	const RowView rows = row_view(a.rsrc[t], a.rows, fld64(wi, 4));
	if (!(o.score > 0.0f)) {
		/* no positive score: the reference's best cell is the first cell in (y, x) order with
		 * score 0 (curr_max starts at -1, src/ConvexAlignFast.cpp:758-763) */
		int fy, fx;
		first_cell(rows, H, W, lane, &fy, &fx);
		if (fy < 0) {
			o.score = -1.0f; o.status = 5; o.pad = 1;
			if (lane == 0) a.tout[t] = o;
			return;
		}
		o.score = 0.0f; o.best_x = fx; o.best_y = fy;
	}
	const int cb0 = fld(wr, 10);
	if (cb0 >= 0)
		backtrack_walk<true>(lane, H, fld(wr, 4), fld(wr, 6), fld(wr, 5), rows,
				reinterpret_cast<const uint2 *>(a.dirs), a.chain_blk + cb0,
				a.seq + (unsigned) fld(wi, 0), a.seq + (unsigned) fld(wi, 1),
				a.ops + fld64(wr, 2), o);
	else
		backtrack_walk<false>(lane, H, fld(wr, 4), fld(wr, 6), fld(wr, 5), rows,
				reinterpret_cast<const uint2 *>(a.dirs + fld64(wr, 0)), nullptr,
				a.seq + (unsigned) fld(wi, 0), a.seq + (unsigned) fld(wi, 1),
				a.ops + fld64(wr, 2), o);
	o.pad = 1;
	if (lane == 0) a.tout[t] = o;
}

/* ------------------------------------------------------------------ backtrack, G lanes per tile */

/*
 * The same walk as backtrack_walk with G (= 16) lanes per tile and four tiles per wave.  The
 * one-wave-per-tile walk keeps its state wave-uniform and therefore lives on the scalar unit: ~140
 * SALU instructions per probe, and one scalar issue slot per SIMD every ~4.3 cycles makes that the
 * bound (SQ counters: the scalar unit 78 % busy, VALU 30 %).  Diagonal runs between two gaps are
 * ~7 cells long at 15 % error, so 64 probing lanes are mostly idle anyway.  Here the walk state is
 * group-uniform in VGPRs, predicates replace the scalar branches, four tiles share every
 * instruction, and the EQ / X sub-runs of a diagonal run are written by their own lanes instead of a
 * scalar loop.  Probe geometry, run skipping, validPath and the op encoding are those of
 * backtrack_walk (reference src/ConvexAlignFast.cpp:335-432, src/AlignmentMatrixFast.cpp:213-220).
 */
template <int G>
struct Group {
	int gl;        /* lane inside the group */
	int base;      /* first lane of the group */
	CVX_DEV unsigned ballot(bool p) const {
		const u64 b = __builtin_amdgcn_ballot_w64(p);
		return (unsigned) (b >> base) & (G == 32 ? 0xffffffffu : ((1u << (G & 31)) - 1u));
	}
	CVX_DEV int bcast(int v, int l) const { return __shfl(v, base + l, 64); }
};

template <int G>
CVX_DEV void backtrack_walk_grp(const Group<G> g, const bool has_tile, const bool chained, const int H, const int N, const int r0, const int ops_cap,
		const RowView &rows, const uint2 *dirs, const ChainBlk *blk, const uint8_t *ref, const uint8_t *qry, int *ops, TileOut &o) {
	/* `chained` is a property of the group's tile (a wave may carry both kinds): dirs is the tile's own
	 * region for whole tiles and the arena for chained ones, whose blocks carry their offsets */
	const int gl = g.gl;
	const int best_x = o.best_x, best_y = o.best_y;
	bool act = has_tile;
	if (has_tile && best_y <= 0) { o.status = 1; act = false; }      /* src/ConvexAlignFast.cpp:338 */
	const bool walked = act;

	const int qend = (H - best_y) - 1;
	int idx = ops_cap - 1;
	int elem = 4;          /* CIGAR_S: the trailing clip is tracked but not stored */
	int elem_len = qend;
	int consumed = qend;
	int x = best_x, y = best_y;
	int s = act ? y % N : 0;
	int status = 0;
	unsigned want = 3u;
	int budget = 2 * (best_x + best_y) + 8;

	auto emit = [&](int cur, int n) {      /* revBacktrack's run-length bookkeeping (:395-403) */
		if (n <= 0) return;
		if (cur == elem) {
			elem_len += n;
		} else {
			if (elem != 4) { if (gl == 0) ops[idx] = (elem_len << 4) | elem; idx -= 1; }
			elem = cur;
			elem_len = n;
		}
	};
	int c_gb = -1;             /* chained tiles: block whose record c_cb holds (per lane) */
	ChainBlk c_cb;
	c_cb.dir_off = 0; c_cb.tblk0 = 0; c_cb.nblk32 = 1;

	while (__builtin_amdgcn_ballot_w64(act) != 0ull) {
		if (act) {
			bool go_on = true;
			if (--budget < 0) { status = 3; go_on = false; }
			else {
				const int dx = (want != 1u) ? 1 : 0, dy = (want != 2u) ? 1 : 0;
				const int cx = x - gl * dx, cy = y - gl * dy;
				const bool inside = (cx >= 0 && cy >= 0);
				const int lx = cx > 0 ? cx : 0, ly = cy > 0 ? cy : 0;
				int sl = s - gl * dy;
				if (sl < 0) sl += N;
				const int tt = cx + cy - r0;
				const int ttc = tt > 0 ? tt : 0;
				const RowDesc2 ol = row_at(rows, ly);
				size_t widx = (size_t) (ttc >> 5) * N + sl;
				if (chained) {
					/* the block record of this lane's row: kept from the previous probe while the row stays in
					 * the same 64-row block, so that most probes cost one memory round trip, not two */
					const int gb = ly / N;
					if (gb != c_gb) { c_cb = blk[gb]; c_gb = gb; }
					int wr = (ttc >> 5) - c_cb.tblk0;
					wr = wr < 0 ? 0 : (wr >= c_cb.nblk32 ? c_cb.nblk32 - 1 : wr);
					widx = c_cb.dir_off + (size_t) wr * N + (size_t) (ly - gb * N);
				}
				const uint2 w = dirs[widx];
				const int rc = ref[lx], qc = qry[ly];
				const unsigned eqm = g.ballot(rc == qc);
				const bool in_row = inside && tt >= 0 && cx >= ol.x && cx < ol.x + ol.y;    /* getDirection: outside -> STOP */
				unsigned code = plane_code(w.x, w.y, 31 - (ttc & 31));
				if (!in_row) code = 0u;
				int minC, maxC;
				valid_bounds(ol.x, ol.y, minC, maxC);

				const unsigned full = (G == 32) ? 0xffffffffu : ((1u << (G & 31)) - 1u);
				const unsigned run = g.ballot(code == want);
				const int L = (run == full) ? G : __builtin_ctz(~run);
				const unsigned low = (L == G) ? full : ((1u << L) - 1u);
				const unsigned vp = g.ballot(cx > minC && cx < maxC);      /* validPath before every move (:368-373) */
				if ((~vp & low) != 0u) { status = 2; go_on = false; }
				else {
					if (want == 3u) {
						if (L > 0) {
							/* EQ / X sub-runs of the diagonal run, lane-parallel: sub-run j (cells from the
							 * current one backwards) goes to ops[idx - w0 - j]; the last one stays pending */
							const unsigned e = eqm & low;
							const unsigned starts = (((e ^ (e << 1)) & low) & ~1u) | 1u;
							const int k = __builtin_popcount(starts);
							const int op0 = (e & 1u) ? 7 : 8;
							if (k == 1) {
								emit(op0, L);
							} else {
								const unsigned after0 = starts & ~1u;
								int len0 = __builtin_ctz(after0);
								int w0 = 0;
								if (op0 == elem) len0 += elem_len;
								else if (elem != 4) { if (gl == 0) ops[idx] = (elem_len << 4) | elem; w0 = 1; }
								const bool is_start = gl < L && ((starts >> gl) & 1u) != 0u;
								const int j = __builtin_popcount(starts & ((1u << gl) - 1u));
								const unsigned rest = (starts >> gl) >> 1;
								int mylen = rest ? __builtin_ctz(rest) + 1 : L - gl;
								if (gl == 0) mylen = len0;
								const int myop = ((e >> gl) & 1u) ? 7 : 8;
								if (is_start && j < k - 1) ops[idx - w0 - j] = (mylen << 4) | myop;
								idx -= w0 + (k - 1);
								const int lastpos = 31 - __builtin_clz(starts);
								elem = ((e >> lastpos) & 1u) ? 7 : 8;
								elem_len = L - lastpos;
							}
						}
						x -= L; y -= L; consumed += L;
					} else if (want == 1u) {
						emit(1, L);
						y -= L; consumed += L;
					} else {
						emit(2, L);
						x -= L;
					}
					if (want != 2u) { s -= L; if (s < 0) s += N; }
					if (L < G) {
						const unsigned nxt = (unsigned) g.bcast((int) code, L);
						if (nxt == 0u) go_on = false;                       /* CIGAR_STOP (or outside the matrix) */
						else if (want != 3u) want = nxt;
						else {
							/* a diagonal run ended in a gap at (x, y) = lane L's cell: follow the gap run inside
							 * the words this probe already holds */
							const int tp = x + y - r0;
							if (nxt == 2u) {
								const unsigned wx = (unsigned) g.bcast((int) w.x, L);
								const unsigned wy = (unsigned) g.bcast((int) w.y, L);
								const int row_lo = max(g.bcast(ol.x, L), 0);
								const int b0 = 31 - (tp & 31);
								const unsigned dm = (wx & ~wy) >> b0;
								int Ld = (~dm == 0u) ? 32 : __builtin_ctz(~dm);
								const int in_word = 32 - b0;
								const int in_rowc = x - row_lo + 1;
								if (Ld > in_rowc) Ld = in_rowc;
								const int rminC = g.bcast(minC, L), rmaxC = g.bcast(maxC, L);
								if (!(x - (Ld - 1) > rminC && x < rmaxC)) { status = 2; go_on = false; }
								else {
									emit(2, Ld);
									x -= Ld;
									if (Ld == in_rowc) go_on = false;            /* next cell is left of the row: STOP */
									else if (Ld == in_word) want = 2u;           /* the run may go on in the previous word */
									else {
										const unsigned c2 = plane_code(wx, wy, b0 + Ld);
										if (c2 == 0u) go_on = false; else want = c2;
									}
								}
							} else {
								const int k = gl - L;
								const int tn = tp - k;
								const bool have = (k >= 0) && (cy >= 0) && (tn >= 0) && ((tn >> 5) == (ttc >> 5));
								const bool col_in = (x >= ol.x) && (x < ol.x + ol.y);
								unsigned c2 = plane_code(w.x, w.y, 31 - (tn & 31));
								if (!col_in) c2 = 0u;
								const unsigned im = g.ballot(have && c2 == 1u) >> L;      /* bit k: cell (x, y - k) is I; bit 0 is set */
								const int Li = (~im == 0u) ? 32 : __builtin_ctz(~im);       /* <= G - L */
								const unsigned ilow = (Li >= 32) ? 0xffffffffu : ((1u << Li) - 1u);
								const unsigned vpi = g.ballot(x > minC && x < maxC) >> L;
								if ((~vpi & ilow) != 0u) { status = 2; go_on = false; }
								else {
									emit(1, Li);
									y -= Li; consumed += Li;
									s -= Li; if (s < 0) s += N;
									const int en = L + Li;
									want = 1u;                                   /* default: let the next probe look again */
									const unsigned hv = g.ballot(have);
									const int c3i = g.bcast((int) c2, en < G ? en : 0);
									if (en < G && ((hv >> en) & 1u) != 0u) {
										if (c3i == 0) go_on = false; else want = (unsigned) c3i;
									}
								}
							}
						}
					}
				}
			}
			if (!go_on) act = false;
		}
	}
	if (walked) {
		if (status == 0) {
			if (elem != 4) { if (gl == 0) ops[idx] = (elem_len << 4) | elem; idx -= 1; }
			consumed += (y + 1);
			o.ref_position = x + 1;
			o.qstart = y + 1;
			o.qend = qend;
			o.ops_first = idx + 1;
			o.n_ops = ops_cap - 1 - idx;
			if (H != consumed) status = 3;
		}
		o.status = status;
	}
}

/* G lanes per tile: block b walks tiles order[b * (64 / G) ...] (largest first: the four tiles of a
 * wave have paths of similar length) */
template <int G>
__global__ void __launch_bounds__(64)
backtrack_grp_kernel(const BacktrackArgs a, const int32_t *order, const int n_order) {
	const int lane = threadIdx.x;
	Group<G> g;
	g.gl = lane & (G - 1);
	g.base = lane & ~(G - 1);
	const int q = blockIdx.x * (64 / G) + lane / G;
	bool has = q < n_order;
	const int t = has ? order[q] : 0;
	TileOut o;
	o.score = -1.0f; o.status = 0; o.best_x = 0; o.best_y = 0;
	o.ref_position = 0; o.qstart = 0; o.qend = 0; o.n_ops = 0; o.ops_first = 0; o.pad = 0;
	TileRun tr;
	TileIn ti;
	tr.skip = 1; tr.ring = 64; tr.r0 = 0; tr.ops_cap = 8; tr.dir_off = 0; tr.ops_off = 0; tr.chain_blk0 = -1;
	ti.H = 0; ti.W = 0; ti.row_off = 0; ti.ref_off = 0; ti.qry_off = 0;
	if (has) {
		tr = a.trun[t];
		o = a.tout[t];
		ti = a.tin[t];
		if (tr.skip != 0 || o.status != 0 || o.pad != 0) has = false;
	}
	const int H = ti.H, W = ti.W;
	/* (a group's tile may be of either kind: per-lane fmt; a batch is all of one kind in practice and the branch in row_at uniform) */
	const RowView rows = row_view(a.rsrc[t], a.rows, ti.row_off);
	bool dead = false;       /* no cell at all: status 5 */
	if (__builtin_amdgcn_ballot_w64(has && !(o.score > 0.0f)) != 0ull) {
		/* no positive score: the reference's best cell is the first cell in (y, x) order with score 0
		 * (curr_max starts at -1, src/ConvexAlignFast.cpp:758-763) */
		if (has && !(o.score > 0.0f)) {
			int fy = -1, fx = 0;
			bool searching = true;
			for (int y0 = 0; __builtin_amdgcn_ballot_w64(searching && y0 < H) != 0ull; y0 += G) {
				if (searching && y0 < H) {
					const int yy = y0 + g.gl;
					bool hc = false;
					int lo_i = 0;
					if (yy < H) {
						const RowDesc2 ol = row_at(rows, yy);
						long long lo = ol.x > 0 ? ol.x : 0;
						long long hi = (long long) ol.x + (long long) ol.y;
						if (hi > W) hi = W;
						hc = hi > lo;
						lo_i = (int) lo;
					}
					const unsigned m = g.ballot(hc);
					const int l = m ? __builtin_ctz(m) : 0;
					const int fxl = g.bcast(lo_i, l);
					if (m != 0u) { fy = y0 + l; fx = fxl; searching = false; }
				}
			}
			if (fy < 0) { dead = true; has = false; }
			else { o.score = 0.0f; o.best_x = fx; o.best_y = fy; }
		}
	}
	const bool chained = tr.chain_blk0 >= 0;
	int *ops = a.ops + tr.ops_off;
	const uint8_t *ref = a.seq + ti.ref_off, *qry = a.seq + ti.qry_off;
	const uint2 *dirs = reinterpret_cast<const uint2 *>(chained ? a.dirs : a.dirs + tr.dir_off);
	backtrack_walk_grp<G>(g, has, chained, H, tr.ring, tr.r0, tr.ops_cap, rows, dirs,
			a.chain_blk + (chained ? tr.chain_blk0 : 0), ref, qry, ops, o);
	if (dead) { o.score = -1.0f; o.status = 5; }
	if ((has || dead) && g.gl == 0) { o.pad = 1; a.tout[t] = o; }
}

/* one wave per tile, after every fill launch of the batch has finished.  (Walkers running
 * BESIDE the fill, in the two wave slots per SIMD it leaves free, were tried: the fill slowed
 * down by as much as the backtrack took -- both phases are bound by instruction issue,
 * DESIGN.md 5.) */
__global__ void __launch_bounds__(64)
backtrack_kernel(const BacktrackArgs a, const int32_t *order, const int n_order) {
	/* block b walks tile order[b] (longest read first; a class's own tiles when a batch walks class by class), or tile b */
	if ((int) blockIdx.x >= n_order) return;
	const int t = order ? order[blockIdx.x] : (int) blockIdx.x;
	walk_tile(a, t, threadIdx.x);
}

/*
 * finalize -- what the host used to do between backtrack and compaction, on the device: exclusive prefix
 * sum of the op counts of the valid tiles (= each tile's slice of the dense ops arena), the caller-facing
 * result records (cvx_result layout) and the batch summary.  Three small launches over blocks of
 * kFinalizeTile tiles, one tile per thread (one workgroup walking 192 tiles per thread took 0.42 ms of the
 * serial stretch between walk and compaction, all of it load latency):
 *
 *   finalize_sum_kernel    per block: ops and number of the valid tiles             -> part[b], part[nblk + b]
 *   finalize_scan_kernel   one workgroup: exclusive scan of part[0 .. nblk) in place, the batch summary,
 *                          and the batch's counters zeroed (it is their last reader)
 *   finalize_write_kernel  per block: part[b] + the scan inside the block           -> res[t], dst_off[t]
 *
 * Every workgroup has 256 threads = one wave per SIMD: a workgroup that finds room on a CU the next
 * batch's fill already occupies (a 1024-thread group waited ~50 ms for sixteen free wave slots on one CU).
 */
/* inclusive scan of v over the 256 threads of a workgroup (s_wave: four slots of LDS); total = the sum of all */
CVX_DEV unsigned long long finalize_block_scan(unsigned long long v, unsigned long long *s_wave, unsigned long long &total) {
	const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
#pragma unroll
	for (int k = 1; k < 64; k <<= 1) {
		const unsigned long long u = __shfl_up(v, k, 64);
		if (lane >= k) v += u;
	}
	__syncthreads();              /* (s_wave may still be read from the scan before) */
	if (lane == 63) s_wave[w] = v;
	__syncthreads();
	unsigned long long before = 0, all = 0;
#pragma unroll
	for (int i = 0; i < kFinalizeTile / 64; ++i) {
		const unsigned long long x = s_wave[i];
		if (i < w) before += x;
		all += x;
	}
	total = all;
	return v + before;
}

__global__ void __launch_bounds__(kFinalizeTile)
finalize_sum_kernel(const TileOut *tout, unsigned long long *part, int n_tiles, int nblk) {
	__shared__ unsigned long long s_wave[kFinalizeTile / 64];
	const int t = blockIdx.x * kFinalizeTile + threadIdx.x;
	unsigned long long ops = 0, valid = 0;
	if (t < n_tiles) {
		const int status = tout[t].status, n_ops = tout[t].n_ops;
		if (status == 0) { valid = 1; if (n_ops > 0) ops = (unsigned long long) n_ops; }
	}
	/* ops < 2^31 per tile and 256 tiles: both sums in one word, the count above bit 40 */
	unsigned long long total;
	finalize_block_scan(ops | (valid << 40), s_wave, total);
	if (threadIdx.x == 0) {
		part[blockIdx.x] = total & ((1ull << 40) - 1);
		part[nblk + blockIdx.x] = total >> 40;
	}
}

__global__ void __launch_bounds__(kFinalizeTile)
finalize_scan_kernel(unsigned long long *part, int nblk, BatchSummary *sum, int32_t *counters, unsigned long long dense_cap) {
	__shared__ unsigned long long s_wave[kFinalizeTile / 64];
	const int tid = threadIdx.x;
	unsigned long long carry = 0, valid = 0;
	for (int b0 = 0; b0 < nblk; b0 += kFinalizeTile) {
		const int b = b0 + tid;
		const unsigned long long mine = b < nblk ? part[b] : 0ull;
		unsigned long long total;
		const unsigned long long incl = finalize_block_scan(mine, s_wave, total);
		if (b < nblk) part[b] = carry + incl - mine;
		carry += total;
		finalize_block_scan(b < nblk ? part[nblk + b] : 0ull, s_wave, total);
		valid += total;
	}
	if (tid == 0) {
		BatchSummary s;
		s.ops_total = carry;
		s.dense_cap = dense_cap;
		s.n_valid = (int32_t) valid;
		s.n_redone = counters ? counters[0] : 0;
		s.chain_task_ticks = counters ? reinterpret_cast<const unsigned long long *>(counters + kCtrChainTicks)[0] : 0ull;
		s.chain_poll_ticks = counters ? reinterpret_cast<const unsigned long long *>(counters + kCtrChainTicks)[1] : 0ull;
		*sum = s;
	}
	/* last reader of the batch's counters (redo statistics, chain tickets): leave them zeroed for the
	 * batch's next run (after the summary above has read the redo count) */
	__syncthreads();
	if (counters && tid < 64) counters[tid] = 0;
}

__global__ void __launch_bounds__(kFinalizeTile)
finalize_write_kernel(const TileOut *tout, const TilePlan *plan, const unsigned long long *part, uint64_t *dst_off, ResultRec *res, int n_tiles) {
	__shared__ unsigned long long s_wave[kFinalizeTile / 64];
	const int t = blockIdx.x * kFinalizeTile + threadIdx.x;
	const bool live = t < n_tiles;
	TileOut o;
	unsigned long long ops = 0;
	if (live) {
		o = tout[t];
		if (o.status == 0 && o.n_ops > 0) ops = (unsigned long long) o.n_ops;
	}
	unsigned long long total;
	const unsigned long long off = part[blockIdx.x] + finalize_block_scan(ops, s_wave, total) - ops;
	if (!live) return;
	ResultRec r;
	r.score = o.score;
	r.status = o.status;
	r.best_x = o.best_x; r.best_y = o.best_y;
	r.ref_position = o.ref_position; r.qstart = o.qstart; r.qend = o.qend;
	r.n_ops = (o.status == 0) ? o.n_ops : 0;
	r.ops_begin = off;
	r.cells = plan[t].cells;
	res[t] = r;
	dst_off[t] = off;
}

/* dense[dst_off[t] .. +n_ops) = region of tile t (tiles that do not fit the arena are skipped:
 * the host sees ops_total > dense_cap in the summary, grows the arena and compacts again) */
__global__ void __launch_bounds__(256)
compact_ops_kernel(const int32_t *regions, const TileRun *trun, const TileOut *tout,
		const uint64_t *dst_off, uint32_t *dense, int n_tiles, unsigned long long dense_cap) {
	const int t = blockIdx.x;
	if (t >= n_tiles) return;
	const TileOut o = tout[t];
	if (o.status != 0 || o.n_ops <= 0) return;
	const unsigned long long d0 = dst_off[t];
	if (d0 + (unsigned long long) o.n_ops > dense_cap) return;
	const int32_t *src = regions + trun[t].ops_off + o.ops_first;
	uint32_t *dst = dense + d0;
	for (int i = threadIdx.x; i < o.n_ops; i += blockDim.x) dst[i] = (uint32_t) src[i];
}

/* ------------------------------------------------------------------ launchers */

/* best cell of a chained tile = first strict maximum over its row blocks in block order (blocks
 * are in row order and each block's own best is already its first strict maximum in (y, x) order) */
__global__ void __launch_bounds__(64)
chain_reduce_kernel(const int32_t *tiles, int n_tiles, const TileRun *trun, const ChainOut *cout, TileOut *tout) {
	const int q = blockIdx.x;
	if (q >= n_tiles) return;
	const int t = tiles[q];
	const TileRun tr = trun[t];
	const int lane = threadIdx.x;
	float b = -1.0f;
	int by = 0x7fffffff, bx = 0x7fffffff, failed = 0;
	for (int g = lane; g < tr.chain_nblk; g += 64) {
		const ChainOut c = cout[tr.chain_blk0 + g];
		failed |= c.failed;
		if (c.score > b) { b = c.score; by = c.best_y; bx = c.best_x; }      /* g ascending: earlier blocks win ties */
	}
#pragma unroll
	for (int off = 32; off >= 1; off >>= 1) {
		const float ob = __shfl_xor(b, off, 64);
		const int oy = __shfl_xor(by, off, 64);
		const int ox = __shfl_xor(bx, off, 64);
		failed |= __shfl_xor(failed, off, 64);
		if (ob > b || (ob == b && (oy < by || (oy == by && ox < bx)))) { b = ob; by = oy; bx = ox; }
	}
	if (lane == 0) {
		TileOut o;
		o.score = b;
		o.status = failed ? -1 : 0;          /* CVX_TILE_UNSUPPORTED: loud, never silent */
		o.best_x = (b > -1.0f) ? bx : 0;
		o.best_y = (b > -1.0f) ? by : 0;
		o.ref_position = 0; o.qstart = 0; o.qend = 0; o.n_ops = 0; o.ops_first = 0;
		o.pad = 0;
		tout[t] = o;
	}
}

/* Which instantiation serves (m, gang, wrap, mode, penalty table, twin): the one place that says so -- launch_fill launches what
 * pick_fill returns, fill_two_phase_waves_per_simd asks the runtime about it -- and the only place that instantiates a fill
 * kernel: what is reachable here is what the code object holds, in the order in which it is first named here. */
typedef void (*FillKernel)(const FillArgs);

template <bool TWIN, int M, bool WRAP, int MODE, bool TAB = false>
static FillKernel wave_fill_kernel() {
	if constexpr (TWIN) return fill_ring_twin_kernel<M, WRAP, MODE, TAB>;
	else return fill_ring_kernel<M, WRAP, MODE, TAB>;
}

/* one wave per tile (per task for chained tiles): chain for the rings that are a power of two, the exact pass, and two-phase with
 * the penalty table when the scoring allows it and the runs are floats, else arithmetic */
template <bool TWIN, int M, bool WRAP>
static FillKernel pick_wave_fill(int mode, bool pen_table) {
	if (mode == kFillChain) {
		if constexpr (M == 3) return nullptr;
		else return wave_fill_kernel<TWIN, M, WRAP, kFillChain>();
	}
	if (mode == kFillExact) return wave_fill_kernel<TWIN, M, WRAP, kFillExact>();
	if (!WRAP && pen_table) return wave_fill_kernel<TWIN, M, false, kFillTwoPhase, true>();
	return wave_fill_kernel<TWIN, M, WRAP, kFillTwoPhase>();
}

template <int M>
static FillKernel pick_wave_fill(bool wrap, int mode, bool pen_table, bool twin) {
	if (wrap) return twin ? pick_wave_fill<true, M, true>(mode, pen_table) : pick_wave_fill<false, M, true>(mode, pen_table);
	return twin ? pick_wave_fill<true, M, false>(mode, pen_table) : pick_wave_fill<false, M, false>(mode, pen_table);
}

/* gangs: G waves per tile on one ring of 64 * 3 * G slots, float runs, whole tiles, not for the twin */
template <int G>
static FillKernel pick_gang_fill(int mode, bool pen_table) {
	if (mode == kFillExact) return fill_ring_kernel<3, false, kFillExact, false, G>;
	if (pen_table) return fill_ring_kernel<3, false, kFillTwoPhase, true, G>;
	return fill_ring_kernel<3, false, kFillTwoPhase, false, G>;
}

struct FillPick {
	FillKernel kernel;      /* nullptr: a combination that is not built */
	int threads;            /* of a workgroup */
};

static FillPick pick_fill(int m, int gang, bool wrap, int mode, bool pen_table, bool twin) {
	FillPick p = { nullptr, 64 };
	if (gang > 1) {
		p.threads = 64 * gang;
		if (m != 3 || wrap || mode == kFillChain || twin) return p;
		p.kernel = gang == 2 ? pick_gang_fill<2>(mode, pen_table) : gang == 3 ? pick_gang_fill<3>(mode, pen_table) : nullptr;
		return p;
	}
	switch (m) {
	case 1: p.kernel = pick_wave_fill<1>(wrap, mode, pen_table, twin); break;
	case 2: p.kernel = pick_wave_fill<2>(wrap, mode, pen_table, twin); break;
	case 3: p.kernel = pick_wave_fill<3>(wrap, mode, pen_table, twin); break;
	case 4: p.kernel = pick_wave_fill<4>(wrap, mode, pen_table, twin); break;
	}
	return p;
}

hipError_t launch_fill(int m, int gang, bool wrap, int mode, const FillArgs &a, size_t pad_lds, hipStream_t st) {
	if (a.list_n <= 0) return hipSuccess;
	const FillPick p = pick_fill(m, gang, wrap, mode, a.pen_table != 0, a.twin != 0);
	if (p.kernel == nullptr) return hipErrorInvalidValue;
	/* pad_lds: unused dynamic LDS that caps how many waiting tasks of a chain launch are resident */
	hipLaunchKernelGGL(p.kernel, dim3(a.list_n), dim3(p.threads), mode == kFillChain ? pad_lds : 0, st, a);
	return hipGetLastError();
}

int fill_two_phase_waves_per_simd(int m, bool wrap, bool pen_table, bool twin) {
	const FillPick p = pick_fill(m, 1, wrap, kFillTwoPhase, pen_table, twin);
	int blocks = 0;      /* workgroups of one wave on a CU = its four SIMDs */
	if (p.kernel == nullptr) return -1;
	if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, p.kernel, p.threads, 0) != hipSuccess) { (void) hipGetLastError(); return -1; }
	return blocks > 0 ? blocks / 4 : -1;
}

hipError_t launch_chain_reduce(const int32_t *tiles, int n_tiles, const TileRun *trun, const ChainOut *cout, TileOut *tout, hipStream_t st) {
	if (n_tiles <= 0) return hipSuccess;
	hipLaunchKernelGGL(chain_reduce_kernel, dim3(n_tiles), dim3(64), 0, st, tiles, n_tiles, trun, cout, tout);
	return hipGetLastError();
}

hipError_t launch_expand_rows(const RowSrc *rsrc, const TileIn *tin, const uint8_t *delta, const RowDesc *rowsx, RowDesc *rows,
		int n_tiles, bool closed_forms, hipStream_t st) {
	if (n_tiles <= 0) return hipSuccess;
	hipLaunchKernelGGL(expand_rows_kernel, dim3(n_tiles), dim3(64), 0, st, rsrc, tin, delta,
			reinterpret_cast<const int2 *>(rowsx), reinterpret_cast<int2 *>(rows), n_tiles, closed_forms ? 1 : 0);
	return hipGetLastError();
}

hipError_t launch_plan(const RowDesc *rows, const RowSrc *rsrc, const TileIn *tin, TilePlan *plan, int n_tiles, uint64_t rows_per_tile,
		unsigned long long max_matrix_mb, hipStream_t st) {
	if (n_tiles <= 0) return hipSuccess;
	if (rows_per_tile >= 1024)
		hipLaunchKernelGGL(plan_kernel<256>, dim3(n_tiles), dim3(256), 0, st,
				reinterpret_cast<const int2 *>(rows), rsrc, tin, plan, n_tiles, max_matrix_mb);
	else
		hipLaunchKernelGGL(plan_kernel<64>, dim3((n_tiles + 3) / 4), dim3(256), 0, st,
				reinterpret_cast<const int2 *>(rows), rsrc, tin, plan, n_tiles, max_matrix_mb);
	return hipGetLastError();
}

/* G lanes per tile, 64 / G tiles per wave */
template <int G>
static void launch_backtrack_grp(const BacktrackArgs &a, const int32_t *order, int n_order, hipStream_t st) {
	hipLaunchKernelGGL(backtrack_grp_kernel<G>, dim3((n_order + 64 / G - 1) / (64 / G)), dim3(64), 0, st, a, order, n_order);
}

hipError_t launch_backtrack(const BacktrackArgs &a, const int32_t *order, int n_order, int group, hipStream_t st) {
	if (a.n_tiles <= 0) return hipSuccess;
	const int nb = order != nullptr ? n_order : a.n_tiles;
	if (nb <= 0) return hipSuccess;
	switch (order != nullptr ? group : 0) {      /* (the code object holds the kernels in the order of the cases) */
	case 16: launch_backtrack_grp<16>(a, order, n_order, st); break;
	case 4: launch_backtrack_grp<4>(a, order, n_order, st); break;       /* (CVX_TUNE_BT_GROUP=4 only) */
	case 8: launch_backtrack_grp<8>(a, order, n_order, st); break;
	case 32: launch_backtrack_grp<32>(a, order, n_order, st); break;
	default: hipLaunchKernelGGL(backtrack_kernel, dim3(nb), dim3(64), 0, st, a, order, nb);   /* one wave per tile */
	}
	return hipGetLastError();
}

hipError_t launch_finalize(const TileOut *tout, const TilePlan *plan, uint64_t *dst_off, uint64_t *part, ResultRec *res,
		BatchSummary *sum, int32_t *counters, int n_tiles, uint64_t dense_cap, hipStream_t st) {
	/* part: 2 * finalize_blocks(n_tiles) words of scratch; an empty batch still gets its summary and its counters zeroed */
	const int nblk = finalize_blocks(n_tiles);
	unsigned long long *p = reinterpret_cast<unsigned long long *>(part);
	if (nblk > 0) hipLaunchKernelGGL(finalize_sum_kernel, dim3(nblk), dim3(kFinalizeTile), 0, st, tout, p, n_tiles, nblk);
	hipLaunchKernelGGL(finalize_scan_kernel, dim3(1), dim3(kFinalizeTile), 0, st, p, nblk, sum, counters, (unsigned long long) dense_cap);
	if (nblk > 0) hipLaunchKernelGGL(finalize_write_kernel, dim3(nblk), dim3(kFinalizeTile), 0, st, tout, plan, p, dst_off, res, n_tiles);
	return hipGetLastError();
}

hipError_t launch_compact(const int32_t *regions, const TileRun *trun, const TileOut *tout,
		const uint64_t *dst_off, uint32_t *dense, int n_tiles, uint64_t dense_cap, hipStream_t st) {
	if (n_tiles <= 0) return hipSuccess;
	hipLaunchKernelGGL(compact_ops_kernel, dim3(n_tiles), dim3(256), 0, st, regions, trun, tout, dst_off, dense, n_tiles,
			(unsigned long long) dense_cap);
	return hipGetLastError();
}

}  // namespace cvx
