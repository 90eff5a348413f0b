/*
 * cvx_score_wave.h -- the scoring kernel for pairs whose shorter side fits in one wave's registers (cvx_score_wave.hip).
 * Kept apart from cvx_launch.h, whose hash names the fill / search kernel families (Makefile FILL_ID / SEARCH_ID).
 */
#ifndef CVX_SCORE_WAVE_H
#define CVX_SCORE_WAVE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cvx_launch.h"

namespace cvx {

/* the shorter string of a pair (NUL included) fits in 64 lanes x kScoreWaveMaxRows rows */
static const int kScoreWaveMaxRows = 16;
static const int kScoreWaveMaxShort = 64 * kScoreWaveMaxRows;

/* rows per lane the kernel uses for a shorter side of `short_len` characters (NUL included): 1, 2, 4, 8 or 16; 0 = too long */
inline int score_wave_rows(int64_t short_len) {
	for (int k = 1; k <= kScoreWaveMaxRows; k *= 2)
		if (short_len <= 64 * k) return k;
	return 0;
}

/* every pair of [pairs, pairs + n) has min(ref_len, qry_len) <= 64 * rows (rows as score_wave_rows gives it); out[i] for pairs[i] */
hipError_t launch_score_wave(const uint8_t *seq, const ScorePair *pairs, float *out, int n, int rows, hipStream_t st);

}  // namespace cvx

#endif
