/*
 * cvx_fill_ring.inc -- the ring fill kernel's text, included by cvx_kernels.hip once per form:
 *
 *   CVX_FILL_KERNEL = fill_ring_kernel,      CVX_FILL_TWIN = false   the reference's ConvexAlignFast (every default handle)
 *   CVX_FILL_KERNEL = fill_ring_twin_kernel, CVX_FILL_TWIN = true    its scalar twin Convex::ConvexAlign (ngmlr --nosse,
 *                                                                    CVX_CREATE_SCALAR_TWIN)
 *
 * The twin runs the same recurrence except that a mismatch against an 'x' of the reference window -- the padding of a window
 * that reaches past its contig, src/SequenceProvider.cpp:610-613 -- costs ScoreParams::misx = mismatch * 100
 * (src/ConvexAlign.cpp:511-513).  That is one compare and one select more per cell, in a loop whose floor is the pipe those
 * two run on (DESIGN.md 5), hence a compile-time switch; and it is a second kernel name instead of a sixth template
 * parameter so that the default forms keep their names and, instruction for instruction, their code.
 *
 * The forms of one kernel (which of them are built, and which serves a launch: pick_fill, cvx_kernels.hip):
 *
 *   MODE   kFillTwoPhase / kFillExact (whole tiles: best-cell tracking late only / from the first step), kFillChain (row blocks)
 *   WRAP   gap runs as the reference's int16 instead of floats
 *   G > 1  a gang of G waves on one ring (M = 3, whole tiles, float runs)
 *   TAB    the convex penalty from a table in LDS instead of multiply, add, min (two-phase, float runs); a cell's offers to its
 *          neighbours are then worked out one step after the cell, when the penalty has come back.  Two forms of it:
 *            a gang    a table of penalties, the run register its byte address, clamped once per 32 steps
 *            FAST      (no gang) {penalty, next address} pairs, the extension offer without a multiply, scores scaled by 2^-64
 *          and without TAB the arithmetic form: V[] and Hc[] hold the offers, computed with the cell.
 *
 * The text has no preprocessor conditional: every choice is a template parameter.  What was tried and left out is in
 * docs/history.md ("Retired build switches of the ring fill").
 */
template <int M, bool WRAP, int MODE, bool TAB = false, int G = 1>
__global__ void __launch_bounds__(64 * G) CVX_FILL_OCC(M, TAB && G == 1)
CVX_FILL_KERNEL(const FillArgs a) {
	constexpr bool TWIN = CVX_FILL_TWIN;
	/* G > 1: a GANG of G waves shares one ring of N = 64 M G slots -- wave w holds the slots [64 M w, 64 M (w + 1)), i.e.
	 * every G-th stretch of 64 M consecutive read rows.  Inside a wave nothing changes; the lane boundary between the last
	 * lane of wave w and the first lane of wave w + 1 (and from the last wave back to the first: the ring) goes through one
	 * self-validating 8-byte record per step in LDS instead of the DPP rotate.  The waves of a gang are never more than
	 * G - 1 steps apart (each needs its predecessor's record of the step before), so they run in lock step on their own
	 * SIMDs: a corridor with 257-576 live rows -- the retry loop's doubled corridors, src/AlignmentBuffer.cpp:291-294 -- is
	 * a whole tile on a ring again (M = 3 per wave: the cheapest cell update there is) instead of 64-row blocks chained
	 * through L2 at 1.6 x the instructions per cell. */
	constexpr int N = 64 * M * G;
	constexpr int NW = 64 * M;             /* slots of one wave */
	constexpr bool EXACT = (MODE != kFillTwoPhase);
	constexpr bool CHAIN = (MODE == kFillChain);
	constexpr bool GANG = G > 1;
	static_assert(!GANG || (!WRAP && !CHAIN), "gangs serve whole tiles with float runs");
	static_assert(!TAB || (!WRAP && MODE == kFillTwoPhase), "the penalty table serves the two-phase float-score instantiation only");
	/* gap run: float (exact small ints), int16-emulating int, or (TAB) the byte address of the run's entry in the penalty table */
	typedef typename RunT<WRAP || TAB>::type run_t;
	const int tid = threadIdx.x;           /* = ring slot / M of the thread's first slot */
	const int lane = GANG ? (tid & 63) : tid;
	const int wv = GANG ? __builtin_amdgcn_readfirstlane(tid >> 6) : 0;      /* wave inside the gang */
	/* FAST = TAB without a gang (the ring classes of every default handle): the penalty table holds {penalty, next run} pairs
	 * (s_pen2 below), the gap-extension offer has no multiply and the step loop runs on scaled scores */
	constexpr bool FAST = TAB && !GANG;
	/* SCALED = FAST, under the name that says why a value is multiplied: every score of the step loop is the unscaled form's times
	 * kScoreScale = 2^-64, so that the clamp bit of v_max3_f32 ([0, 1]) is the zero clamp of the cell maximum and nothing else:
	 * the largest score, 2^20 a row over 2^31 rows, scales to 2^-13.  The scoring values are scaled once, here (the table's
	 * penalties below, computed unscaled first); the host admits only scorings whose nonzero values have binary exponents in [-20, 20] (score_scale_exact, cvx_host_logic.h),
	 * every score is then a multiple of 2^-43 and its scaled value is zero or normal, and binary32 +, max, negation and
	 * compares commute with the scaling.  best[] and lbest are multiplied back before the argmax; kFillExact stays unscaled. */
	constexpr bool SCALED = FAST;
	const float go = SCALED ? a.sp.go * kScoreScale : a.sp.go;
	const float gext = a.sp.ge, gem = a.sp.gem, decay = a.sp.decay;
	/* keep match / mismatch in VGPRs: v_cndmask cannot take two SGPR values plus a mask */
	float vmat = SCALED ? a.sp.mat * kScoreScale : a.sp.mat, vmis = SCALED ? a.sp.mis * kScoreScale : a.sp.mis;
	asm volatile("" : "+v"(vmat), "+v"(vmis));

	/* The row a slot takes over next is a 16-byte record in LDS, written 16*M rows at a time by the whole
	 * wave long before the hand-over (stage_rows below): the hand-over itself is one ds_read_b128 and two
	 * adds for the few lanes whose row just ended, instead of two dependent trips to HBM (corridor row, then
	 * reference characters) and ~25 VALU instructions executed by the whole wave for one or two lanes --
	 * round 2's counters had the wave parked on s_waitcnt for a quarter of its time, most of it here.
	 * The row of a slot's best cell (changes only at a hand-over) lives in LDS too, to keep VGPRs for occupancy. */
	__shared__ int4 s_rec[CHAIN ? 1 : M * G][64];      /* (gang: wave w's records at [w * M + ...]) */
	__shared__ int s_besty[M][64 * G];
	/* gang: what the last slot of wave w offers the first slot of wave w + 1, one record per step in a ring of kGangDepth
	 * (BoundaryRec layout: score bits | run16 | insertion bit | 15-bit step tag), and the waves' partial results at the end */
	__shared__ u64 s_gx[GANG ? G : 1][GANG ? kGangDepth : 1];
	__shared__ float s_gred[GANG ? G : 1][4];
	__shared__ int s_gfail[GANG ? G : 1];
	__shared__ BoundaryVal s_bnd[CHAIN ? kChainChunk : 1];      /* the predecessor's boundary records of the current chunk of steps */
	/* TAB: the convex penalty min(gem, gext + run * decay) (src/ConvexAlignFast.cpp:672-674) takes 28 distinct values under
	 * every preset; entry `run` of this table holds it, computed once per wave with the very operations the arithmetic form
	 * uses (binary32 multiply, add, min, each rounded on its own).  The run register of a slot is then the entry's byte
	 * address and the cell update reads its penalty with one ds_read_b32 -- the LDS pipe is otherwise idle in the step
	 * loop -- instead of v_mul + v_add + v_min.  The penalty is constant from some run on (27 with the default scoring:
	 * gext + run * decay has reached gem); the host enables this form only when that run is below kPenClamp
	 * (FillArgs::pen_table), and the run registers are clamped to kPenClamp once per 32-step block, in the branch that
	 * flushes the direction words -- a run register only ever selects a penalty, so the clamp changes nothing, and it need
	 * only run often enough that the address stays inside the table: a register grows by one entry per step at most, so
	 * the table has kPenClamp + kPenClampSteps + 1 entries or more whatever the corridor (gap runs through zero-score
	 * cells are as long as a row is wide).  A gang's wave clamps what it takes from its neighbour's record as well (a
	 * scalar min): that register was offered one step before the neighbour's own clamp. */
	/* FAST: the table holds {pen, next} pairs,
	 * next(e) = kPenPairStride * min(e + 1, kPenClamp), and the run register of the new cell is the second dword of the same
	 * ds_read_b64 that fetches its penalty, consumed one step later like the penalty.  No add per cell, no periodic clamp, no
	 * slack entries: an address is always one of kPenPairStride * (1 ... kPenClamp).  The host's condition (penalty constant
	 * from run kPenClamp on) is what makes the saturating next exact.  The gang form keeps the table above, its clamp and the
	 * 16-bit run of its boundary record. */
	__shared__ float s_pen[TAB && !FAST ? kPenEntries : 1];
	__shared__ float2 s_pen2[FAST ? kPenPairs : 1];

	int t;                          /* tile */
	int task_id = 0, y0 = 0;        /* chain: task index, first read row of the block */
	u64 chain_t0 = 0ull, chain_polled = 0ull;      /* chain: s_memtime at the task's start; ticks spent polling for boundary records */
	ChainTask ct;
	if (CHAIN) {
		int tk = 0;
		if (lane == 0) tk = atomicAdd(a.chain_ticket, 1);
		task_id = __builtin_amdgcn_readfirstlane(tk);
		if (task_id >= a.list_n) return;
		ct = a.tasks[task_id];
		t = ct.tile;
		y0 = ct.y0;
		/* A chained tile is a dependency chain through all of its blocks and, beside thousands of whole tiles (ONT
		 * mix: 10 % retries at twice the width among 54 000 short tiles; C5: the corridors widened to 2 048 / 8 192
		 * columns), the long pole of the launch: its waves go first on their SIMDs and the whole-tile classes fill in
		 * (ONT, 60 000 tiles: 7 660-7 770 -> 8 320-8 450 Gbp/h; C5 mix, 2 048 tiles: 2 860-2 930 -> 3 140).  The host
		 * can switch it off (CVX_TUNE_CHAIN_PRIO=0). */
		if (a.chain_prio) __builtin_amdgcn_s_setprio(3);
		chain_t0 = __builtin_amdgcn_s_memtime();
	} else {
		t = a.list[blockIdx.x];
		/* the widest ring class of a batch of several (FillArgs::chain_prio, set by the host): its waves pay the most per step, its
		 * tiles are the launch's long pole beside the narrower classes' -- one notch above those */
		if (!GANG && a.chain_prio) { if (a.chain_prio >= 2) __builtin_amdgcn_s_setprio(2); else __builtin_amdgcn_s_setprio(1); }
		/* The list is longest-first and a tile is a serial chain of steps: in a batch of uneven tiles (ONT mix: median
		 * 1.3 kb, up to 20 kb) the launch lasts as long as its longest tiles take at a sixth of a SIMD.  The first
		 * sixteenth of the list runs at raised wave priority: those waves proceed at nearly a whole SIMD's pace, the short
		 * tiles fill in behind them.  (A batch of equal tiles -- the PacBio bench -- is unaffected.) */
		if (blockIdx.x < (unsigned) (a.list_n >> 4)) __builtin_amdgcn_s_setprio(2);
		/* a gang's tiles are the widest corridors of the batch -- the retry loop's second and third attempts, twice and three
		 * times the steps per row -- and, like the chained blocks, the long pole of a mixed launch: raised priority for all of them
		 * (FillArgs::chain_prio; CVX_TUNE_GANG_PRIO=0 switches it off) */
		if (GANG && a.chain_prio) __builtin_amdgcn_s_setprio(2);
		if (MODE == kFillExact) {
			if (a.tout[t].pad != kPadRedo) return;   /* block-uniform */
			if (tid == 0) atomicAdd(a.redo_count, 1);
		}
	}
	/* The tile's constants are wave-uniform, but the records they come from are fetched with vector loads (nothing tells the
	 * compiler the tables are not written meanwhile), and what is derived from them -- 64-bit addresses above all -- then sits in
	 * vector registers for the whole step loop, to be spilled and reloaded in its rare paths (round 5: 26 dwords, +16 GB of
	 * scratch traffic per launch).  Through readfirstlane once, here, they are scalar for good. */
	TileIn ti = a.tin[t];
	ti.ref_off = in_sgpr(ti.ref_off); ti.qry_off = in_sgpr(ti.qry_off); ti.W = in_sgpr(ti.W); ti.H = in_sgpr(ti.H);
	ti.row_off = in_sgpr((u64) ti.row_off);
	TileRun tr = a.trun[t];
	tr.dir_off = in_sgpr((u64) tr.dir_off); tr.r0 = in_sgpr(tr.r0); tr.nsteps = in_sgpr(tr.nsteps);
	RowView rv = row_view(a.rsrc[t], a.rows, ti.row_off, y0);      /* wave-uniform: closed forms are evaluated in make_rec */
	rv.rows = in_sgpr(rv.rows); rv.fmt = in_sgpr(rv.fmt); rv.width = in_sgpr(rv.width);
	rv.k = in_sgpr(rv.k); rv.d = in_sgpr(rv.d); rv.right = in_sgpr(rv.right);
	const uint8_t *seq = a.seq;
	const int H = CHAIN ? ct.rows : ti.H, W = ti.W;     /* rows of this task */
	const unsigned qry_off = ti.qry_off + (unsigned) y0;
	const int r0 = CHAIN ? ct.r0 : tr.r0;
	const int nsteps = CHAIN ? ct.nsteps : tr.nsteps;
	uint32_t *dirs = in_sgpr(a.dirs + (CHAIN ? ct.dir_off : tr.dir_off));
	/* per-slot state in VGPRs (static indexing only).  A slot that is not inside its
	 * row's range holds the reference's empty element (score 0, run 0, STOP:
	 * src/AlignmentMatrixFast.h:49-53), i.e. S = 0, runs = 0, V = Hc = gap_open;
	 * the update below produces exactly that for inactive lanes by itself. */
	float S[M];        /* score of the slot's latest cell                            */
	float Hc[M];       /* left candidate that cell offers to the next column (arithmetic forms: TAB has offers() instead) */
	float V[M];        /* up candidate it offers to the next row (likewise)          */
	float dg[M];       /* diagonal score for the slot's next cell                    */
	run_t drun[M];     /* deletion run of the latest cell: the run itself (0 unless D) in the int16   */
	run_t irun[M];     /* kernels, run + 1 in the float ones (read only through mD / mI); same for I  */
	int cnt[M];        /* next column index inside the row (negative: not started)   */
	int len[M];        /* row length after clipping to [0,W)                         */
	int qch[M];        /* read character of the row                                  */
	unsigned xa[M];    /* seq-arena offset of the next reference dword to prefetch   */
	unsigned cwn[M];   /* reference characters of the NEXT 4-step group              */
	float penp[M];     /* TAB: the penalty an extension of the slot's latest cell pays, on its way from LDS */
	float best[M];
	int best_r[M];
	float lbest = 0.0f;          /* early phase: running maximum of this lane's cells */
	unsigned accA[M], accB[M];   /* direction bit-planes of the current 32-step block */
	/* per-slot lane masks in SGPRs */
	u64 mD[M];         /* latest cell is a deletion (run > 0)  */
	u64 mI[M];         /* latest cell is an insertion          */

	/* Row record: what a slot needs to take row yy (block-local index) over at any later step rnext:
	 *   x = first anti-diagonal of the row (cnt = rnext - x is the column index inside the row, < 0 before it starts)
	 *   y = row length after clipping to [0, W)          z = read character of the row
	 *   w = arena offset of the reference character of anti-diagonal 0 in this row (= ref_off - row index);
	 *       also identifies the row: yy = ref_base - w.
	 * Rows at and beyond H (the ring outlives the tile) get a record that never starts. */
	const unsigned ref_base = ti.ref_off - (unsigned) y0;
	auto make_rec = [&](const int yy) {
		int4 rec;
		rec.w = (int) (ref_base - (unsigned) yy);
		if (yy < H) {
			const RowDesc2 ol = row_at(rv, yy);
			const long long Ws = (long long) W;
			long long lo = ol.x > 0 ? ol.x : 0;
			long long hi = (long long) ol.x + (long long) ol.y;
			if (hi > Ws) hi = Ws;
			if (hi < lo) hi = lo;
			rec.x = yy + y0 + (int) lo;
			rec.y = (int) (hi - lo);
			rec.z = seq[qry_off + (unsigned) yy];
		} else {
			rec.x = yy + y0 + (1 << 30);
			rec.y = 0;
			rec.z = 0;
		}
		return rec;
	};
	/* slot j takes the row of `rec` over; rnext = index of the next step.  Invariant between groups:
	 * xa[j] = rec.w + r + 4, the address of the characters of the group after next. */
	auto take_row = [&](const int j, const int4 rec, const int rnext, const bool fetch_now) {
		cnt[j] = rnext - rec.x;
		len[j] = rec.y;
		qch[j] = rec.z;
		xa[j] = (unsigned) rec.w + (unsigned) rnext + 4u;
		/* The characters of the group starting at rnext: whatever cwn[j] holds will do when the row starts
		 * no earlier than the group after (cells outside a row are forced to the empty element whatever
		 * they compare); the regular prefetch at the top of the next group then picks the row up.  Only a
		 * ring without slack hands a slot over less than a group before its row starts. */
		if (fetch_now || cnt[j] > -4) cwn[j] = *reinterpret_cast<const unsigned *>(seq + (xa[j] - 4u));
	};
	/* the wave writes the records of rows [Y, Y + 16 M) to their slots (sY = the first one's slot inside the wave, wave-uniform) */
	constexpr int kStage = 16 * M;
	auto stage_rows = [&](const int Y, const int sY) {
		if (lane < kStage) {
			const int4 rec = make_rec(Y + lane);
			const int sl = sY + lane;
			s_rec[CHAIN ? 0 : wv * M + sl % M][sl / M] = rec;
		}
		__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");      /* one wave: LDS write -> read order across lanes */
	};

	if (FAST) {
		if (lane < kPenPairs) {
			const int nx = lane + 1 < kPenClamp ? lane + 1 : kPenClamp;
			const float pen = fminf(gem, gext + (float) lane * decay);
			s_pen2[lane] = make_float2(SCALED ? pen * kScoreScale : pen, __int_as_float(kPenPairStride * nx));
		}
		__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
	} else if (TAB) {
		for (int i = lane; i < kPenEntries; i += 64) s_pen[i] = fminf(gem, gext + (float) i * decay);
		__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
	}
#pragma unroll
	for (int j = 0; j < M; ++j) {
		s_besty[j][tid] = 0;
		S[j] = 0.0f; Hc[j] = go; V[j] = go; dg[j] = 0.0f;
		drun[j] = 0; irun[j] = 0;
		best[j] = 0.0f; best_r[j] = 0;
		penp[j] = gem;
		accA[j] = accB[j] = 0u;
		mD[j] = 0; mI[j] = 0;
		cwn[j] = 0u;
		take_row(j, make_rec(tid * M + j), r0, true);
	}
	/* rows [N, 2N - 16 M) are staged up front; from then on the hand-over of every row that is a multiple
	 * of 16 M (slot 0 of lanes 0, 16, 32, 48) stages the 16 M rows that end one ring further on: their slots
	 * were all handed over before it (rows end in order), and the first of them is needed only when the row
	 * 16 M above the triggering one ends, N - 16 M row ends later.  (A gang's wave stages its own stretches of 64 M rows:
	 * three of the four chunks of its next stretch up front, then one chunk per trigger, a stretch every N rows.) */
	int stage_next = N + wv * NW, stage_slot = 0;
	auto stage_advance = [&]() {
		stage_next += kStage;
		stage_slot += kStage;
		if (stage_slot >= NW) { stage_slot = 0; stage_next += N - NW; }
	};
	if (!CHAIN) {
		for (int c = 0; c < NW / kStage - 1; ++c) { stage_rows(stage_next, stage_slot); stage_advance(); }
	}

	int gang_failed = 0;
	if (GANG) {
		/* no record is valid yet (tag 0x7fff is the one of step 32767, by when every entry has long been rewritten) */
		if (lane < kGangDepth) s_gx[wv][lane] = ~0ull;
		__syncthreads();
	}
	const int gang_pred = GANG ? (wv + G - 1) % G : 0;      /* the wave whose last slot holds the row above this wave's first */

	const int ngroups = (nsteps + 3) >> 2;
	int late = ngroups >> a.late_shift;
	if (late < a.late_min_groups) late = a.late_min_groups;
	const int gswitch = (EXACT || late >= ngroups) ? 0 : ngroups - late;   /* first exactly tracked group */
	int r = r0;

	/* chain: where this block's last row lives (it feeds the next block) and what has been published */
	const int out_slot = CHAIN ? (ct.rows - 1) : 0;
	const int out_lane = out_slot / M, out_j = out_slot % M;
	u64 *bnd_out = CHAIN ? reinterpret_cast<u64 *>(a.bnd + ct.bnd_out_off) : nullptr;
	u64 *bnd_in = CHAIN ? reinterpret_cast<u64 *>(a.bnd + ct.bnd_in_off) : nullptr;
	const unsigned epoch = a.bnd_epoch;
	int chain_failed = 0;
	BoundaryVal bcur;               /* boundary record of the next step */
	bcur.V = go; bcur.S = 0.0f; bcur.run = 0u; bcur.is_ins = 0u;
	u64 bpre = 0ull;                /* this lane's record of the NEXT chunk, requested one chunk early (epoch 0: not valid) */

	/* one 4-step group; TRACK: exact best-cell tracking (else only the lane maximum) */
	auto group = [&](auto track_tag, const int g) {
		constexpr bool TRACK = decltype(track_tag)::value;
		if (CHAIN && (g & (kChainChunk / 4 - 1)) == 0) {
			/* boundary records of the next kChainChunk steps: record i belongs to column lo + i of the row above this
			 * block.  Lane l < kChainChunk owns the record of step r + l; it asked for it one chunk ago. */
			const int x = (r - y0) + lane;                     /* column of the first row's cell at step r + lane */
			const int idx = x - ct.bnd_lo;
			const bool mine = ct.prev >= 0 && lane < kChainChunk && idx >= 0 && idx < ct.bnd_len;
			u64 q = bpre;
			bool ok = !mine || (unsigned) (q >> 49) == epoch;
			int spins = 0;
			const bool must_poll = !chain_failed && ballot(!ok) != 0ull;
			const u64 poll_t0 = must_poll ? __builtin_amdgcn_s_memtime() : 0ull;      /* (statistics: cvx_timing.chain_poll_ticks) */
			while (!chain_failed && ballot(!ok) != 0ull) {     /* (wave-uniform) the producer has not got there yet */
				if (!ok) {
					q = __hip_atomic_load(bnd_in + idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
					ok = (unsigned) (q >> 49) == epoch;
				}
				if (ballot(!ok) == 0ull) break;
				if (++spins > (1 << 21)) { chain_failed = 1; break; }     /* seconds: never hang the device */
				/* back off: a task that was dispatched long before its turn must not flood the fabric with polls */
				if (spins < 8) __builtin_amdgcn_s_sleep(2);
				else if (spins < 64) __builtin_amdgcn_s_sleep(32);
				else __builtin_amdgcn_s_sleep(127);
			}
			if (must_poll) chain_polled += __builtin_amdgcn_s_memtime() - poll_t0;
			BoundaryVal br;
			br.V = go; br.S = 0.0f; br.run = 0u; br.is_ins = 0u;     /* outside the row above: the empty element */
			if (mine && ok) {
				const unsigned meta = (unsigned) (q >> 32);
				const float sc = __uint_as_float((unsigned) q);
				const unsigned run16 = meta & 0xffffu;
				const bool ins = (meta >> 16) & 1u;
				/* the run register as the producer's slot held it, and the run its gap penalty was computed from */
				const float runf = WRAP ? (float) (int) (short) run16 : (float) run16 - 1.0f;
				br.S = sc;
				br.run = WRAP ? (unsigned) (int) (short) run16 : __float_as_uint((float) run16);
				br.is_ins = ins ? 1u : 0u;
				br.V = ins ? gap_extend_value(sc, runf, gem, gext, decay) : sc + go;
			}
			if (lane < kChainChunk) s_bnd[lane] = br;
			__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");      /* one wave: LDS write -> read order */
			bcur = s_bnd[0];
			/* ask for the next chunk's records now: they are on their way while this chunk computes */
			const int idxn = idx + kChainChunk;
			bpre = 0ull;
			if (ct.prev >= 0 && lane < kChainChunk && idxn >= 0 && idxn < ct.bnd_len)
				bpre = __hip_atomic_load(bnd_in + idxn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		}
		/* this group's reference characters were fetched one group ago */
		unsigned cw[M];
		const float misx = TWIN ? (SCALED ? a.sp.misx * kScoreScale : a.sp.misx) : 0.0f;      /* (handed to phase1 as an argument: one more capture and hipcc no longer unrolls the step loop) */
#pragma unroll
		for (int j = 0; j < M; ++j) {
			cw[j] = cwn[j];
			cwn[j] = *reinterpret_cast<const unsigned *>(seq + xa[j]);
			xa[j] += 4u;
		}
		/* flush the previous 32-step block of direction words HERE, right after the
		 * wait for this group's characters: gfx9 counts loads and stores in one vmcnt,
		 * so a store issued just before that wait would be waited for in full */
		if (g != 0 && (g & 7) == 0) {
			/* scalar base of the block + a 32-bit lane offset (a per-lane 64-bit pointer kept across the loop was spilled) */
			uint32_t *d = dirs + (size_t) ((g >> 3) - 1) * (N * 2);
			const unsigned dl = (unsigned) tid * (M * 2);
#pragma unroll
			for (int j = 0; j < M; ++j) { d[dl + 2 * j] = accA[j]; d[dl + 2 * j + 1] = accB[j]; }
			if (TAB && !FAST) {
				/* the clamp of the run registers, once per kPenClampSteps steps (one register per slot: the deletion and the
				 * insertion run of a cell share it in this form) */
				static_assert(kPenClampSteps == 32, "the run registers are clamped where the direction words are flushed");
#pragma unroll
				for (int j = 0; j < M; ++j) { const int c = min((int) drun[j], 4 * kPenClamp); drun[j] = (run_t) c; irun[j] = (run_t) c; }
			}
		}

#pragma unroll
		for (int i = 0; i < 4; ++i) {
			/* lane boundary: previous lane's last slot, values of step r-1 */
			/* (TAB: what a slot's latest cell offers -- E to an extension, O to an opening -- is worked out here, one
			 * step after the cell, from its score, the penalty that has come back from LDS meanwhile and its two masks) */
			float p_E[M], p_O[M];
			auto offers = [&](const int j) {
				/* FAST: -S for the product.  Either is +-0 exactly when S is zero and negative otherwise, and an offer is only read
				 * through the maximum with zero and the equality with that maximum */
				p_E[j] = FAST ? fmaxf(S[j] + penp[j], -S[j]) : fmaxf(S[j] + penp[j], S[j] * -0x1p100f);
				p_O[j] = S[j] + go;
			};
			if (TAB) offers(M - 1);
			float uV0 = TAB ? rot1_f(lanes(mI[M - 1]) ? p_E[M - 1] : p_O[M - 1]) : rot1_f(V[M - 1]);
			float uS0 = rot1_f(S[M - 1]);
			run_t uI0;
			if (WRAP || TAB) uI0 = (run_t) rot1_i((int) irun[M - 1]);
			else uI0 = (run_t) rot1_f((float) irun[M - 1]);
			u64 mIu0 = rot1_m(mI[M - 1]);
			u64 gq = 0ull;
			if (GANG && r != r0) gq = __hip_atomic_load(&s_gx[gang_pred][(r - r0 - 1) & (kGangDepth - 1)], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
			/* gang: the first slot of the wave has the last slot of the wave before it above it.  The record of the step before
			 * was asked for at the top of this step and is looked at only here, in front of slot 0, the last slot of the step --
			 * the waves of a gang run in lock step, it has been there for most of a step (a spin otherwise, bounded) */
			auto gang_take = [&]() {
				float sc = 0.0f, vv = go;
				unsigned run16 = 0u, ins = 0u;
				if (r != r0) {
					const unsigned want_tag = (unsigned) (r - r0 - 1) & 0x7fffu;
					int spins = 0;
					while (!gang_failed && (((unsigned) __builtin_amdgcn_readfirstlane((int) (gq >> 32))) >> 17) != want_tag) {
						if (++spins > (1 << 22)) { gang_failed = 1; break; }      /* never hang the device */
						__builtin_amdgcn_s_sleep(kGangWaitSleep);
						gq = __hip_atomic_load(&s_gx[gang_pred][(r - r0 - 1) & (kGangDepth - 1)], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
					}
					const unsigned meta = (unsigned) __builtin_amdgcn_readfirstlane((int) (gq >> 32));
					sc = __uint_as_float((unsigned) __builtin_amdgcn_readfirstlane((int) gq));
					run16 = meta & 0xffffu;
					ins = (meta >> 16) & 1u;
					/* the up candidate is a function of (score, run, insertion): rebuilt with the cell update's own operations */
					vv = ins ? gap_extend_value(sc, (float) run16 - 1.0f, gem, gext, decay) : sc + go;
				}
				if (lane == 0) {
					uV0 = vv;
					uS0 = sc;
					/* (TAB: the neighbour's register of the step before, which may be the last step before its clamp; clamped here
					 * it obeys this wave's bound -- kPenClamp plus the steps since this wave's own clamp -- like every other one) */
					uI0 = TAB ? (run_t) (int) ((run16 < (unsigned) kPenClamp ? run16 : (unsigned) kPenClamp) << 2) : (run_t) (float) run16;
				}
				mIu0 = (mIu0 & ~1ull) | (u64) ins;
			};
			/* ... and offers its own last slot's new cell to the wave after it: lane 63, right after that slot (the first of the step) */
			auto gang_give = [&]() {
				const unsigned run16 = TAB ? (((unsigned) (int) irun[M - 1]) >> 2) & 0xffffu : ((unsigned) (int) (float) irun[M - 1]) & 0xffffu;
				const unsigned meta = run16 | (unsigned) (((mI[M - 1] >> 63) & 1ull) << 16) | (((unsigned) (r - r0) & 0x7fffu) << 17);
				if (lane == 63)
					__hip_atomic_store(&s_gx[wv][(r - r0) & (kGangDepth - 1)], ((u64) meta << 32) | (u64) __float_as_uint(S[M - 1]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
			};
			if (CHAIN) {
				/* the block's first row (lane 0, slot 0) has the previous block's last row above it */
				/* (the record was fetched from LDS one step ago: its latency is off the step's critical path) */
				const BoundaryVal br = bcur;
				bcur = s_bnd[((r - r0) + 1) & (kChainChunk - 1)];
				if (lane == 0) {
					uV0 = br.V;
					uS0 = br.S;
					uI0 = WRAP ? (run_t) (int) br.run : (run_t) __uint_as_float(br.run);
				}
				const int bit = __builtin_amdgcn_readfirstlane((int) br.is_ins);
				mIu0 = (mIu0 & ~1ull) | (u64) (bit & 1);
			}

			/* The cell update in three phases per slot: (1) candidates, maximum and the equality /
			 * activity lane masks; (2) the priority chain on the masks (SALU); (3) the new slot state.
			 * Slot j reads slot j-1's values of the previous step: phase 3 runs in descending j. */
			float p_lc[M], p_dc[M], p_uc[M], p_mx[M];
			u64 p_eL[M], p_eU[M], p_eG[M], p_act[M], p_isDl[M], p_isIu[M];
			u64 p_nD[M], p_nI[M], p_gap[M], p_cread[M];
			auto phase1 = [&](const int j, const float misx_) {
				float uV = (j > 0) ? V[j > 0 ? j - 1 : 0] : uV0;
				const run_t uI = (j > 0) ? irun[j > 0 ? j - 1 : 0] : uI0;
				const u64 mIu = (j > 0) ? mI[j > 0 ? j - 1 : 0] : mIu0;
				float lcv = Hc[j];
				if (TAB) {
					if (j > 0) {
						offers(j > 0 ? j - 1 : 0);
						uV = lanes(mIu) ? p_E[j > 0 ? j - 1 : 0] : p_O[j > 0 ? j - 1 : 0];
					}
					lcv = lanes(mD[j]) ? p_E[j] : p_O[j];
				}
				const int refc = (int) ((cw[j] >> (8 * i)) & 0xffu);
				const bool eq = (refc == qch[j]);
				/* TWIN: eq is still the byte compare -- an 'x' of the read against an 'x' of the window is a match; the select goes
				 * through a lane mask like every other one of the step (the compare writes the mask, v_cndmask reads it) */
				float mv = vmis;
				if (TWIN) mv = lanes(ballot(refc == 'x')) ? misx_ : vmis;
				const float diag_cell = dg[j] + (eq ? vmat : mv);
				float lc = lcv, dc = diag_cell, uc = uV;
				/* SCALED: one v_max3_f32 with the clamp bit.  The sign of a zero result is the instruction's; it is not observable: a
				 * zero is never positive and enters compares only as equal to zero */
				if (FAST) {
					/* Row activity through EXEC: v_cmpx writes act = cnt < len to EXEC as well, the clamped maximum is then written
					 * into a register that holds 0 and the three equalities into masks that come back clear outside the row -- sc
					 * without its select, nD and nI without their `& act` (phase2, phase3), one half-rate op and one scalar op less
					 * per cell for one full-rate v_mov.  Everything else of the slot runs under full EXEC, outside the block: a lane
					 * outside its row still shifts its plane words, counts, rotates and offers.  EXEC goes back to all lanes: the
					 * workgroup is one full wave (no gang) and the step loops are wave-uniform -- a constant, because a saved copy
					 * handed in changed the code of the other forms.  Five instructions lie between v_cmpx and whatever follows the
					 * block, the wait states a DPP op needs after a VALU write of EXEC; the compiler does not look inside
					 * (profiles/r26_fill_cell.txt) */
					float sc = 0.0f;
					u64 act, eL, eU, eG;
					asm volatile("v_cmpx_lt_u32_e64 %1, %5, %6\n\t"
					             "v_max3_f32 %0, %7, %8, %9 clamp\n\t"
					             "v_cmp_eq_f32_e64 %2, %0, %7\n\t"
					             "v_cmp_eq_f32_e64 %3, %0, %9\n\t"
					             "v_cmp_eq_f32_e64 %4, %0, %8\n\t"
					             "s_mov_b64 exec, -1"
					             : "+v"(sc), "=&s"(act), "=&s"(eL), "=&s"(eU), "=&s"(eG)
					             : "v"(cnt[j]), "v"(len[j]), "v"(lc), "v"(dc), "v"(uc));
					p_lc[j] = lc; p_dc[j] = dc; p_uc[j] = uc; p_mx[j] = sc;
					p_eL[j] = asm_mask(eL); p_eU[j] = asm_mask(eU); p_eG[j] = asm_mask(eG); p_act[j] = asm_mask(act);
				} else {
					const float mx = SCALED ? __builtin_amdgcn_fmed3f(fmaxf(fmaxf(lc, dc), uc), 0.0f, 1.0f) : fmaxf(fmaxf(fmaxf(lc, dc), uc), 0.0f);
					p_lc[j] = lc; p_dc[j] = dc; p_uc[j] = uc; p_mx[j] = mx;
					p_eL[j] = ballot(mx == lc);
					p_eU[j] = ballot(mx == uc);
					p_eG[j] = ballot(mx == dc);
					p_act[j] = ballot((unsigned) cnt[j] < (unsigned) len[j]);
				}
				p_isDl[j] = WRAP ? ballot(drun[j] > 0) : mD[j];
				p_isIu[j] = WRAP ? ballot(uI > 0) : mIu;
			};
			auto phase2 = [&](const int j) {
				const u64 eL = p_eL[j], eU = p_eU[j], eG = p_eG[j], act = p_act[j], isDl = p_isDl[j], isIu = p_isIu[j];
				/* priority: del-extend > ins-extend > diag > del-open > ins-open > stop
				 * (src/ConvexAlignFast.cpp:703-738), on lane masks; nothing fires on a
				 * lane that is outside its row */
				const u64 c2 = isIu & eU;
				/* (FAST: the equalities are clear outside the row already) */
				const u64 nD = FAST ? eL & (isDl | ~(c2 | eG)) : eL & (isDl | ~(c2 | eG)) & act;
				const u64 nI = FAST ? ~nD & eU & (isIu | ~eG) : ~nD & eU & (isIu | ~eG) & act;
				p_nD[j] = nD; p_nI[j] = nI;
				p_gap[j] = nD | nI;
				/* plane 1 = nI | nG with nG = eG & ~gap & act; the act term is dropped: direction
				 * bits of cells outside a row are never read (backtrack_walk masks them) */
				p_cread[j] = nI | (eG & ~nD);
			};
			auto phase3 = [&](const int j) {
				const float uS = (j > 0) ? S[j > 0 ? j - 1 : 0] : uS0;
				const run_t uI = (j > 0) ? irun[j > 0 ? j - 1 : 0] : uI0;
				const u64 nD = p_nD[j], nI = p_nI[j], isDl = p_isDl[j], isIu = p_isIu[j];
				const float mx = p_mx[j];
				/* outside the row the new "cell" is the empty element: score 0 (FAST: p_mx is that already) */
				const float sc = FAST ? mx : (lanes(p_act[j]) ? mx : 0.0f);
				run_t nd, ni;
				float runf = 0.0f;
				if (FAST) {
					/* the registers hold the table address of entry run + 1 -- the {penalty, next address} pair of a cell that
					 * extends this one -- and the new cell's register comes back with its penalty; as in the float form they are
					 * only ever read through the masks (isDl, isIu) */
					const u64 extD = nD & isDl, extI = nI & isIu;
					const int t1 = lanes(extI) ? (int) uI : kPenPairStride;
					const int ra = lanes(extD) ? (int) drun[j] : t1;
					const float2 pn = *reinterpret_cast<const float2 *>(reinterpret_cast<const char *>(s_pen2) + ra);
					nd = (run_t) __float_as_int(pn.y);
					ni = nd;
					penp[j] = pn.x;
				} else if (TAB) {
					/* the registers hold 4 * (run + 1), the table address of the penalty a cell that extends this one pays
					 * for; as in the float form they are only ever read through the masks (isDl, isIu) */
					const u64 extD = nD & isDl, extI = nI & isIu;
					const int t1 = lanes(extI) ? (int) uI : 4;
					const int ra = lanes(extD) ? (int) drun[j] : t1;
					nd = (run_t) (ra + 4);
					ni = nd;
					penp[j] = *reinterpret_cast<const float *>(reinterpret_cast<const char *>(s_pen) + ra);
				} else if (WRAP) {
					/* indelRun is a short in the reference (src/AlignmentMatrixFast.h:43) */
					nd = lanes(nD) ? (lanes(isDl) ? (run_t) (short) ((int) drun[j] + 1) : (run_t) 1) : (run_t) 0;
					ni = lanes(nI) ? (lanes(isIu) ? (run_t) (short) ((int) uI + 1) : (run_t) 1) : (run_t) 0;
					runf = (float) (lanes(nD) ? nd : ni);
				} else {
					/* One run register per cell: the run of a gap cell (plus one), anything otherwise.  It is only
					 * ever read through the masks "left cell was D" / "up cell was I" (isDl, isIu), so
					 * nothing needs zeroing: an extension continues the run of the cell it extends, an
					 * opening starts at 1 (src/ConvexAlignFast.cpp:655-668,703-738). */
					/* The register holds run + 1, the run of a cell that extends this one, so an extension
					 * is one select and needs no "either extension" mask. */
					const u64 extD = nD & isDl, extI = nI & isIu;
					const float t1 = lanes(extI) ? (float) uI : 1.0f;
					runf = lanes(extD) ? (float) drun[j] : t1;
					nd = (run_t) (runf + 1.0f);
					ni = nd;
				}
				dg[j] = uS;
				S[j] = sc;
				drun[j] = nd;
				irun[j] = ni;
				if (!TAB) {
					/* the arithmetic forms work the cell's offers out at once (TAB: one step later, in offers()) */
					const float E = gap_extend_value(sc, runf, gem, gext, decay);
					const float O = sc + go;
					V[j] = lanes(nI) ? E : O;
					Hc[j] = lanes(nD) ? E : O;
				}
				if (TRACK) {
					const u64 better = ballot(sc > best[j]);   /* sc is 0 outside the row, best >= 0 */
					best[j] = lanes(better) ? mx : best[j];
					best_r[j] = lanes(better) ? r : best_r[j];
				} else if (i >= 2) {
					/* early phase: the running maximum samples steps 2 and 3 of every group only.  A cell of
					 * step 0 or 1 scores at most `match` more than its best predecessor (left / up cost, the
					 * diagonal adds at most `match`), and its predecessors lie in sampled steps (or in step 0,
					 * bounded the same way), so every untracked score is <= lbest + match; the acceptance test
					 * at the end carries that slack. */
					lbest = fmaxf(lbest, sc);
				}
				mD[j] = nD;
				mI[j] = nI;
				cnt[j] += 1;
				accA[j] = shl1_in(accA[j], p_gap[j]);       /* plane 0: I or D */
				accB[j] = shl1_in(accB[j], p_cread[j]);     /* plane 1: I or diagonal */
			};
#pragma unroll
			for (int j = M - 1; j >= 0; --j) {
				if (GANG && j == 0) gang_take();
				phase1(j, misx); phase2(j);
				phase3(j);
				if (GANG && j == M - 1) gang_give();
				if (CHAIN && j == out_j && ct.has_next) {
					/* the last row's new cell goes to the boundary stream (record index = its column in the row) */
					if (lane == out_lane && (unsigned) (cnt[j] - 1) < (unsigned) len[j]) {
						const unsigned run16 = WRAP ? ((unsigned) (int) irun[j] & 0xffffu) : ((unsigned) (int) (float) irun[j] & 0xffffu);
						const unsigned meta = run16 | (unsigned) (((mI[j] >> out_lane) & 1ull) << 16) | (epoch << 17);
						__hip_atomic_store(bnd_out + (cnt[j] - 1), ((u64) meta << 32) | (u64) __float_as_uint(S[j]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
					}
				}
			}
			r += 1;
		}
		/* hand finished slots to their next row (y + N): a row's last cell is consumed
		 * by the row below one step after it was computed, so wait for cnt > len
		 * (a chained block has at most N rows: nothing is ever handed on) */
		/* (wave-uniform: a row that is a multiple of 16 M is handed over in this group) */
		const bool stage_now = !CHAIN && (ballot(cnt[0] > len[0]) & 0x0001000100010001ull) != 0ull;
#pragma unroll
		for (int j = 0; j < M; ++j) {
			if (!CHAIN && cnt[j] > len[j]) {     /* finished a real row (slots beyond the tile count up from -2^30) */
				if (TRACK) {
					const int yy = (int) (ref_base - (xa[j] - (unsigned) r - 4u));
					if (best_r[j] >= r - cnt[j]) s_besty[j][tid] = yy;
				}
				take_row(j, s_rec[CHAIN ? 0 : wv * M + j][lane], r, false);
			}
		}
		if (stage_now) {
			stage_rows(stage_next, stage_slot);
			stage_advance();
		}
	};

	for (int g = 0; g < gswitch; ++g) group(BoolTag<false>(), g);
	for (int g = gswitch; g < ngroups; ++g) group(BoolTag<true>(), g);

	if (ngroups > 0) {
		/* last block (complete or partial): left-align so that step (t & 31) sits at
		 * bit 31 - (t & 31) */
		const int done = ((ngroups - 1) & 7) + 1;     /* groups in the last block */
		const int sh = 32 - 4 * done;
		uint32_t *d = dirs + ((size_t) ((ngroups - 1) >> 3) * N + (size_t) tid * M) * 2;
#pragma unroll
		for (int j = 0; j < M; ++j) { d[2 * j] = sh ? accA[j] << sh : accA[j]; d[2 * j + 1] = sh ? accB[j] << sh : accB[j]; }
	}

	/* argmax with the reference's tie-break: first strict maximum in (y, x) order
	 * (src/ConvexAlignFast.cpp:758-763 / :1165-1170) among the exactly tracked cells */
	float b = -1.0f;
	int by = 0x7fffffff, bx = 0x7fffffff;
#pragma unroll
	for (int j = 0; j < M; ++j) {
		int vy = s_besty[j][tid];
		const int ycur = (int) (ref_base - (xa[j] - (unsigned) r - 4u));      /* the row the slot holds now */
		if (ycur < H && best_r[j] >= r - cnt[j]) vy = ycur;
		const float v = SCALED ? best[j] * kScoreUnscale : best[j];      /* (best[] is +0 or positive) */
		const int vx = best_r[j] - vy;
		if (v > 0.0f) {     /* best[] starts at 0: a slot that never saw a positive score has no candidate */
			if (v > b || (v == b && (vy < by || (vy == by && vx < bx)))) { b = v; by = vy; bx = vx; }
		}
	}
	float be = SCALED ? lbest * kScoreUnscale : lbest;       /* maximum over the cells that were not tracked exactly */
#pragma unroll
	for (int off = 32; off >= 1; off >>= 1) {
		const float ob = __shfl_xor(b, off, 64);
		const int oy = __shfl_xor(by, off, 64);
		const int ox = __shfl_xor(bx, off, 64);
		if (ob > b || (ob == b && (oy < by || (oy == by && ox < bx)))) { b = ob; by = oy; bx = ox; }
		if (!EXACT) be = fmaxf(be, __shfl_xor(be, off, 64));
	}
	if (CHAIN) {
		if (lane == 0) {
			ChainOut co;
			co.score = b;
			co.best_y = (b > -1.0f) ? by + y0 : 0;
			co.best_x = (b > -1.0f) ? bx - y0 : 0;      /* bx was computed against block-local rows */
			co.failed = chain_failed;
			a.chain_out[ct.blk] = co;
			unsigned long long *ticks = reinterpret_cast<unsigned long long *>(a.redo_count + kCtrChainTicks);
			atomicAdd(ticks, (unsigned long long) (__builtin_amdgcn_s_memtime() - chain_t0));
			if (chain_polled) atomicAdd(ticks + 1, (unsigned long long) chain_polled);
		}
		return;
	}
	if (GANG) {
		/* the waves' partial results, combined by wave 0 in wave order with the same tie-break */
		if (lane == 0) {
			s_gred[wv][0] = b; s_gred[wv][1] = __int_as_float(by); s_gred[wv][2] = __int_as_float(bx);
			s_gred[wv][3] = EXACT ? 0.0f : be;
			s_gfail[wv] = gang_failed;
		}
		__syncthreads();
		if (wv != 0) return;
#pragma unroll
		for (int w = 1; w < G; ++w) {
			const float ob = s_gred[w][0];
			const int oy = __float_as_int(s_gred[w][1]), ox = __float_as_int(s_gred[w][2]);
			if (ob > b || (ob == b && (oy < by || (oy == by && ox < bx)))) { b = ob; by = oy; bx = ox; }
			if (!EXACT) be = fmaxf(be, s_gred[w][3]);
		}
	}
	if (lane == 0) {
		/* b == -1: no positive score among the tracked cells.  If there is none anywhere either,
		 * the reference (curr_max starts at -1) takes the first cell in (y, x) order, score 0;
		 * backtrack_kernel resolves that rare case. */
		TileOut o;
		o.score = b;
		o.status = 0;
		o.best_x = (b > -1.0f) ? bx : 0;
		o.best_y = (b > -1.0f) ? by : 0;
		o.ref_position = 0; o.qstart = 0; o.qend = 0; o.n_ops = 0; o.ops_first = 0;
		/* pad = 0: filled, not backtracked yet; kPadRedo: an untracked cell scored at least as much
		 * as the best tracked one, so the first strict maximum is not known -> exact pass */
		/* be under-estimates the early maximum by at most `match` (steps 0 and 1 of a group are not sampled);
		 * 2 * match + 1 also covers the rounding of the float adds behind that bound */
		o.pad = (!EXACT && gswitch > 0 && !(b > be + 2.0f * a.sp.mat + 1.0f)) ? kPadRedo : 0;
		if (GANG) {
			/* a wave that gave up waiting for its neighbour's record: CVX_TILE_UNSUPPORTED, loud, never a hang or a wrong answer */
			bool failed = gang_failed != 0;
			for (int w = 1; w < G; ++w) failed = failed || s_gfail[w] != 0;
			if (failed) { o.status = -1; o.pad = 0; }
		}
		a.tout[t] = o;
	}
}
