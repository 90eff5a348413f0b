/*
 * cvx_score_stage.hip -- the strings of a scoring call written on the device (gfx950): for every (sub-read, candidate) pair the
 * window of the resident 4-bit genome and the read, as it is or reverse-complemented, go straight into the scoring job's
 * sequence arena, and the ScorePair table the scoring kernels read is filled in.  What ScoreBuffer::DoRun's preparation loop does
 * on the host per pair (reference src/ScoreBuffer.cpp:94-121: DecodeRefSequence, src/SequenceProvider.cpp:567-625, and
 * computeReverseSeq, src/MappedRead.cpp:35-73); here only the reads (once per call) and 56 bytes per pair cross PCIe.
 *
 * The shape of every string is worked out on the host in closed form (cvx_score_windows.h: score_window_shape); the kernel
 * looks at the genome only for the characters themselves:
 *   window[k] = the nibble of position + k for k < n_plain, 'x' for n_plain <= k < ref_chars, NUL at ref_chars;
 *   query[k]  = read[k], or cpl(read[read_len - 1 - k]) on the reverse strand, NUL at read_len.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cvx_score_stage.h"

namespace cvx {

namespace {

/* (dec4_char, lut4, expand8: the nibble expansion of cvx_genome.hip, restated here because that file's hash names the builds
 * its counters were collected on) */
__device__ __forceinline__ uint8_t dec4_char(unsigned v) {
	return v == 0u ? 'A' : v == 1u ? 'T' : v == 2u ? 'G' : v == 3u ? 'C' : v == 4u ? 'N' : '?';
}
/* four nibble values, one per byte -> four characters: v_perm_b32 as an eight-entry byte table (A T G C | N ? ? ?), a second one
 * that turns bit 3 of a value into a byte mask for the values the table does not hold */
__device__ __forceinline__ uint32_t lut4(const uint32_t x) {
	const uint32_t c = __builtin_amdgcn_perm(0x3F3F3F4Eu, 0x43475441u, x & 0x07070707u);
	const uint32_t m = __builtin_amdgcn_perm(0u, 0u, ((x >> 3) & 0x01010101u) | 0x0C0C0C0Cu);
	return (c & ~m) | (0x3F3F3F3Fu & m);
}
/* eight nibbles, the first in bits 31:28 -> their characters in memory order */
__device__ __forceinline__ void expand8(const uint32_t d, uint32_t &o0, uint32_t &o1) {
	const uint32_t ch = lut4((d >> 4) & 0x0F0F0F0Fu), cl = lut4(d & 0x0F0F0F0Fu);
	o0 = __builtin_amdgcn_perm(ch, cl, 0x02060307u);
	o1 = __builtin_amdgcn_perm(ch, cl, 0x00040105u);
}

__device__ __forceinline__ uint8_t cpl_char(const uint8_t c) {      /* cpl, src/MappedRead.cpp:35-46 */
	return c == 'A' ? 'T' : c == 'T' ? 'A' : c == 'C' ? 'G' : c == 'G' ? 'C' : c;
}
/* Four bytes complemented and their order reversed.  Bits 2:1 of a byte tell A, C, T and G apart (0, 1, 2, 3): v_perm_b32 looks
 * up, per byte, the letter those bits stand for and its complement; a byte that IS that letter takes the complement, every other
 * byte (N, lower case, anything) stays. */
__device__ __forceinline__ uint32_t cpl_rev4(const uint32_t x) {
	const uint32_t idx = (x >> 1) & 0x03030303u;
	const uint32_t letter = __builtin_amdgcn_perm(0u, 0x47544341u, idx);      /* A C T G */
	const uint32_t comp = __builtin_amdgcn_perm(0u, 0x43414754u, idx);        /* T G A C */
	const uint32_t t = x ^ letter;
	const uint32_t nz = (((t & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | t) & 0x80808080u;   /* bit 7 of every byte that differs */
	const uint32_t keep = (nz >> 7) * 0xFFu;
	return __builtin_bswap32((comp & ~keep) | (x & keep));
}

}  // namespace

__global__ void __launch_bounds__(256)
stage_score_windows_kernel(const uint8_t * __restrict__ bin, const uint8_t * __restrict__ reads, const ScoreWinDesc * __restrict__ desc,
		int n, uint8_t * __restrict__ seq, ScorePair * __restrict__ pairs) {
	/* one WAVE per pair, four pairs per workgroup, in the manner of decode_windows_kernel: the slot is wave-uniform and says so
	 * (readfirstlane), its descriptor comes through scalar loads */
	const int si = __builtin_amdgcn_readfirstlane((int) (blockIdx.x * 4u + (threadIdx.x >> 6)));
	const int lane = (int) (threadIdx.x & 63u);
	if (si >= n) return;
	const ScoreWinDesc d = desc[si];
	/* Sixteen characters per lane: a lane owns one 16-byte-ALIGNED piece of the destination (the string's address in the arena
	 * is whatever the strings in front of it left), stored with one dwordx4; the ragged head and tail go byte by byte.  A window
	 * of 306 characters is 19 pieces, a 256-base read 16: one trip each. */
	{
		uint8_t *out = seq + d.ref_off;
		const int n_chars = d.ref_chars, n_plain = d.n_plain;
		const unsigned long long pos = d.position;
		auto char_at = [&](const int i) -> uint8_t {
			if (i >= n_plain) return (uint8_t) 'x';
			const unsigned long long p = pos + (unsigned long long) i;      /* <= L = n_nibbles - 1: a nibble of the genome */
			const unsigned b = bin[p >> 1];
			return dec4_char((p & 1ull) ? (b & 0xFu) : (b >> 4));
		};
		int head = (int) ((16u - (unsigned) ((uintptr_t) out & 15u)) & 15u);
		if (head > n_chars) head = n_chars;
		for (int i = lane; i < head; i += 64) out[i] = char_at(i);
		const int n_pieces = (n_chars - head + 15) / 16;
		for (int pc = lane; pc < n_pieces; pc += 64) {
			const int i0 = head + 16 * pc;
			if (i0 + 16 <= n_plain) {
				/* The 8 genome bytes behind the piece with one unaligned load, a ninth when the piece starts on a low nibble.
				 * All sixteen nibbles are plain ones, i.e. nibbles of the genome: from an even p0 they fill exactly the 8
				 * bytes loaded, from an odd one the sixteenth lies in the ninth -- either way the last byte read holds a nibble
				 * of the genome, so no load leaves it and nothing is clamped.  (The allocation is PADDED as well:
				 * cvx_genome_upload puts 64 bytes of N behind the genome, which decode_windows_kernel relies on; here that is
				 * a margin, not a need.) */
				const unsigned long long p0 = pos + (unsigned long long) i0;
				const uint8_t *src = bin + (p0 >> 1);
				unsigned long long lo8;
				__builtin_memcpy(&lo8, src, 8);
				unsigned long long nb = __builtin_bswap64(lo8);      /* sixteen nibbles, the first in bits 63:60 */
				if (p0 & 1ull) nb = (nb << 4) | (unsigned long long) (src[8] >> 4);
				uint32_t wv[4];
				expand8((uint32_t) (nb >> 32), wv[0], wv[1]);
				expand8((uint32_t) nb, wv[2], wv[3]);
				*reinterpret_cast<uint4 *>(out + i0) = make_uint4(wv[0], wv[1], wv[2], wv[3]);
			} else {
				const int i1 = i0 + 16 < n_chars ? i0 + 16 : n_chars;
				for (int i = i0; i < i1; ++i) out[i] = char_at(i);
			}
		}
		if (lane == 0) out[n_chars] = 0;
	}
	{
		uint8_t *out = seq + d.qry_off;
		const uint8_t *rd = reads + d.read_off;      /* read-only: the same read may serve forward and reverse pairs of one call */
		const int len = d.read_len;
		const bool rev = d.reverse != 0;             /* (wave-uniform) */
		auto byte_at = [&](const int i) -> uint8_t { return rev ? cpl_char(rd[len - 1 - i]) : rd[i]; };
		int head = (int) ((16u - (unsigned) ((uintptr_t) out & 15u)) & 15u);
		if (head > len) head = len;
		for (int i = lane; i < head; i += 64) out[i] = byte_at(i);
		const int n_pieces = (len - head + 15) / 16;
		for (int pc = lane; pc < n_pieces; pc += 64) {
			const int i0 = head + 16 * pc;
			if (i0 + 16 <= len) {      /* sixteen source bytes, all inside the read */
				uint4 v;
				if (!rev) {
					__builtin_memcpy(&v, rd + i0, 16);
				} else {
					uint4 s;
					__builtin_memcpy(&s, rd + (len - 16 - i0), 16);
					v = make_uint4(cpl_rev4(s.w), cpl_rev4(s.z), cpl_rev4(s.y), cpl_rev4(s.x));
				}
				*reinterpret_cast<uint4 *>(out + i0) = v;
			} else {
				const int i1 = i0 + 16 < len ? i0 + 16 : len;
				for (int i = i0; i < i1; ++i) out[i] = byte_at(i);
			}
		}
		if (lane == 0) out[len] = 0;
	}
	if (lane == 0) {
		ScorePair p;
		p.ref_off = d.ref_off; p.qry_off = d.qry_off; p.scratch_off = d.scratch_off;
		p.ref_len = d.ref_chars + 1; p.qry_len = d.read_len + 1;
		pairs[si] = p;
	}
}

hipError_t launch_stage_score_windows(const uint8_t *bin, const uint8_t *reads, const ScoreWinDesc *desc, int n,
		uint8_t *seq, ScorePair *pairs, hipStream_t st) {
	if (n <= 0) return hipSuccess;
	hipLaunchKernelGGL(stage_score_windows_kernel, dim3((n + 3) / 4), dim3(256), 0, st, bin, reads, desc, n, seq, pairs);
	return hipGetLastError();
}

}  // namespace cvx
