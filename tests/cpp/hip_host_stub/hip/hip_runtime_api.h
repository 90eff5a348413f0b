/*
 * Host stand-in for the HIP runtime's headers, for tests/cpp/score_stage_emu_test.cpp only: enough of the language extensions and
 * of two gfx9 builtins to compile cvx_score_stage.hip with plain g++ and run its kernel one lane at a time.  v_perm_b32 is
 * emulated as the ISA defines it (bytes 0-3 of the selector pick from {S0:S1}, 12 gives 0x00, 13 and above 0xFF); a kernel whose
 * lanes exchange data (LDS, DPP, ballots) cannot be run this way.
 */
#ifndef CVX_HIP_HOST_STUB_H
#define CVX_HIP_HOST_STUB_H

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define __device__
#define __global__
#define __host__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __restrict__

typedef int hipError_t;
typedef void *hipStream_t;
#define hipSuccess 0
static inline hipError_t hipGetLastError() { return hipSuccess; }
#define hipLaunchKernelGGL(...) ((void) 0)

struct uint2 { uint32_t x, y; };
struct uint4 { uint32_t x, y, z, w; };
static inline uint4 make_uint4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) { uint4 v = {a, b, c, d}; return v; }
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
static dim3 threadIdx, blockIdx;      /* set by the test in front of every lane */

static inline int hip_stub_readfirstlane(int x) { return x; }      /* (only ever applied to wave-uniform values) */
static inline uint32_t hip_stub_perm(uint32_t s0, uint32_t s1, uint32_t sel) {
	const uint64_t v = ((uint64_t) s0 << 32) | s1;
	uint32_t out = 0;
	for (int b = 0; b < 4; ++b) {
		const unsigned k = (sel >> (8 * b)) & 0xFFu;
		uint32_t byte;
		if (k < 8) byte = (uint32_t) ((v >> (8 * k)) & 0xFFu);
		else if (k == 12) byte = 0;
		else if (k >= 13) byte = 0xFFu;
		else { fprintf(stderr, "hip_stub_perm: selector %u (sign replication) is not emulated\n", k); abort(); }
		out |= byte << (8 * b);
	}
	return out;
}
#define __builtin_amdgcn_readfirstlane hip_stub_readfirstlane
#define __builtin_amdgcn_perm hip_stub_perm

#endif
