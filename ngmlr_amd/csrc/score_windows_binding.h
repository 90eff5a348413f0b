/*
 * score_windows_binding.h -- what score_windows_binding.inc needs in front of ScoreBuffer's functions (tools/build_ngmlr_hip.sh
 * adds the include to src/ScoreBuffer.cpp for the variant ngmlr_hip_scorewin).
 */
#ifndef CVX_SCORE_WINDOWS_BINDING_H
#define CVX_SCORE_WINDOWS_BINDING_H

#include <stdlib.h>
#include <map>
#include <vector>

#include "convex_align_hip.h"
#include "stripped_sw_hip.h"

/* CVX_SCORE_WINDOWS=0 keeps the reference's string path inside the same binary (A/B runs, tests/test_gpu_e2e_scorewin.py) */
static inline bool cvxScoreWindowsOn() {
	static int on = -1;
	if (on < 0) {
		char const * e = getenv("CVX_SCORE_WINDOWS");
		on = (e != 0 && atoi(e) == 0) ? 0 : 1;
	}
	return on != 0;
}

#endif
