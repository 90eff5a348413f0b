/*
 * cs_feed_binding.h -- what cs_feed_binding.inc needs in front of CS::RunBatch (tools/build_ngmlr_hip.sh adds the include to
 * src/CS.cpp and defines CVX_CS_FEED_BINDING for the variant ngmlr_hip_feed).
 */
#ifndef CVX_CS_FEED_BINDING_H
#define CVX_CS_FEED_BINDING_H

#include <stdlib.h>

#include "convex_align_hip.h"
#include "stripped_sw_hip.h"

#define CVX_CS_FEED_BINDING 1

/* CVX_CS_FEED=0 keeps the two device calls per batch inside the same binary (A/B runs, tests/test_gpu_e2e_feed.py) */
static inline bool cvxCsFeedOn() {
	/* (read once, by whichever CS thread asks first: the initialisation of a function-local static is thread-safe) */
	static bool const on = []() { char const * e = getenv("CVX_CS_FEED"); return !(e != 0 && atoi(e) == 0); }();
	return on;
}

#endif
