/*
 * cvx_fill_occupancy.hip -- the occupancy of the two-phase whole-tile fills, asked of the runtime.
 *
 * The kernels are cvx_kernels.hip's: they are only DECLARED here, with the template heads of cvx_fill_ring.inc, so that this file
 * names the very instantiations launch_fill_t picks -- a head that no longer matches fails at link time -- and the kernels'
 * own sources, which the build's fill id is the hash of, stay as they are.  Nothing here runs on the device.
 */
#include <hip/hip_runtime.h>

#include "cvx_types.h"
#include "cvx_fill_occupancy.h"

namespace cvx {

enum { kOccTwoPhase = 0 };      /* FillMode::kFillTwoPhase (cvx_kernels.hip) */

template <int M, bool WRAP, int MODE, bool TAB, int G> __global__ void fill_ring_kernel(const FillArgs a);
template <int M, bool WRAP, int MODE, bool TAB, int G> __global__ void fill_ring_twin_kernel(const FillArgs a);

/* waves of one CU / its four SIMDs; one workgroup of these kernels is one wave */
template <typename K>
static int waves_per_simd(K kernel) {
	int blocks = 0;
	if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, kernel, 64, 0) != hipSuccess) { (void) hipGetLastError(); return -1; }
	return blocks > 0 ? blocks / 4 : -1;
}

/* the ladder of launch_fill_t / launch_fill_twin_t for kModeTwoPhase */
template <int M, bool WRAP>
static int two_phase_t(bool pen_table, bool twin) {
	if (twin) {
		if (!WRAP && pen_table) return waves_per_simd(fill_ring_twin_kernel<M, false, kOccTwoPhase, true, 1>);
		return waves_per_simd(fill_ring_twin_kernel<M, WRAP, kOccTwoPhase, false, 1>);
	}
	if (!WRAP && pen_table) return waves_per_simd(fill_ring_kernel<M, false, kOccTwoPhase, true, 1>);
	return waves_per_simd(fill_ring_kernel<M, WRAP, kOccTwoPhase, false, 1>);
}

int fill_two_phase_waves_per_simd(int m, bool wrap, bool pen_table, bool twin) {
	switch (m) {
	case 1: return wrap ? two_phase_t<1, true>(pen_table, twin) : two_phase_t<1, false>(pen_table, twin);
	case 2: return wrap ? two_phase_t<2, true>(pen_table, twin) : two_phase_t<2, false>(pen_table, twin);
	case 3: return wrap ? two_phase_t<3, true>(pen_table, twin) : two_phase_t<3, false>(pen_table, twin);
	case 4: return wrap ? two_phase_t<4, true>(pen_table, twin) : two_phase_t<4, false>(pen_table, twin);
	default: return -1;
	}
}

}  // namespace cvx
