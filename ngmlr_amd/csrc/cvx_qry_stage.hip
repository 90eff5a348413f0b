/*
 * cvx_qry_stage.hip -- the queries of an alignment job written on the device (gfx950): every tile names its query as a segment
 * of the call's read block, and the string -- the segment as it is, or reverse-complemented -- goes straight into the job's
 * sequence arena, in front of plan_kernel.  What AlignmentBuffer::extractReadSeq does on a worker core per SingleAlign (reference
 * src/AlignmentBuffer.cpp:1515-1549: strncpy, or computeReverseSeq, :1130-1141, over cplBase, :1117-1128); here every distinct
 * read crosses PCIe once per call and 24 bytes per tile.
 *
 * The rule and the work split are cvx_segments.h's: query[k] = read[start + k], or cpl(read[start + len - 1 - k]); a string is
 * cut into chunks of 256 aligned 16-byte pieces (segment_chunk_shape), one wave per chunk.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cvx_qry_stage.h"

namespace cvx {

namespace {

__device__ __forceinline__ uint8_t seg_cpl_char(const uint8_t c) {      /* cplBase, src/AlignmentBuffer.cpp:1117-1128 */
	return c == 'A' ? 'T' : c == 'T' ? 'A' : c == 'C' ? 'G' : c == 'G' ? 'C' : c;
}
/* Four bytes complemented and their order reversed (cpl_rev4 of cvx_score_stage.hip, restated here: that file's object code
 * stays what it was).  Bits 2:1 of a byte tell A, C, T and G apart (0, 1, 2, 3): v_perm_b32 looks up, per byte, the letter
 * those bits stand for and its complement; a byte that IS that letter takes the complement, every other byte (N, lower case,
 * anything) stays. */
__device__ __forceinline__ uint32_t seg_cpl_rev4(const uint32_t x) {
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
stage_segments_kernel(const uint8_t * __restrict__ reads, const SegDesc * __restrict__ desc, const SegChunk * __restrict__ chunks,
		int n_chunks, uint8_t * __restrict__ seq) {
	/* one WAVE per chunk, four chunks per workgroup, in the manner of stage_score_windows_kernel: the chunk is wave-uniform and
	 * says so (readfirstlane), its two descriptors come through scalar loads */
	const int ci = __builtin_amdgcn_readfirstlane((int) (blockIdx.x * 4u + (threadIdx.x >> 6)));
	const int lane = (int) (threadIdx.x & 63u);
	if (ci >= n_chunks) return;
	const SegChunk ch = chunks[ci];
	const SegDesc d = desc[ch.seg];
	uint8_t *out = seq + d.dst_off;
	const uint8_t *rd = reads + d.src_off;      /* read-only: tiles that share a read share its bytes, forward and reverse */
	const int len = d.len;
	const bool rev = (d.flags & CVX_SEG_REVCOMP) != 0;      /* (wave-uniform) */
	const SegChunkShape sh = segment_chunk_shape((uint32_t) ((uintptr_t) out & 15u), len, ch.piece0);
	/* Whole pieces: a lane owns every 64th 16-byte-ALIGNED piece of the destination, kSegLanePieces of them, and asks for the
	 * source bytes of all of them before it converts the first -- one round trip to memory per chunk, not four.  The source of
	 * a piece is one unaligned 16-byte load: [i0, i0 + 16) of the segment, or its mirror image [len - 16 - i0, len - i0); with
	 * i0 + 16 <= len (what makes a piece a whole one, segment_chunk_shape) both lie inside the segment, so no load leaves the
	 * read and nothing depends on what lies around it. */
	uint4 v[kSegLanePieces];
#pragma unroll
	for (int t = 0; t < kSegLanePieces; ++t) {
		const int i0 = sh.full_lo + kSegPiece * (lane + 64 * t);
		v[t] = make_uint4(0u, 0u, 0u, 0u);
		if (i0 < sh.full_hi) __builtin_memcpy(&v[t], rd + (rev ? len - kSegPiece - i0 : i0), kSegPiece);
	}
#pragma unroll
	for (int t = 0; t < kSegLanePieces; ++t) {
		const int i0 = sh.full_lo + kSegPiece * (lane + 64 * t);
		if (i0 < sh.full_hi) {
			const uint4 s = v[t];
			*reinterpret_cast<uint4 *>(out + i0) = rev ? make_uint4(seg_cpl_rev4(s.w), seg_cpl_rev4(s.z), seg_cpl_rev4(s.y), seg_cpl_rev4(s.x)) : s;
		}
	}
	/* the ragged ends, fewer than sixteen bytes each, one byte per lane */
	auto byte_at = [&](const int i) -> uint8_t { return rev ? seg_cpl_char(rd[len - 1 - i]) : rd[i]; };
	if (lane < sh.head_hi) out[lane] = byte_at(lane);
	if (sh.tail_lo + lane < sh.tail_hi) out[sh.tail_lo + lane] = byte_at(sh.tail_lo + lane);
}

hipError_t launch_stage_segments(const uint8_t *reads, const SegDesc *desc, const SegChunk *chunks, int n_chunks, uint8_t *seq, hipStream_t st) {
	if (n_chunks <= 0) return hipSuccess;
	hipLaunchKernelGGL(stage_segments_kernel, dim3((n_chunks + 3) / 4), dim3(256), 0, st, reads, desc, chunks, n_chunks, seq);
	return hipGetLastError();
}

}  // namespace cvx
