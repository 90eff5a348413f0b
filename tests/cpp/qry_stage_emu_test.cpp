/*
 * qry_stage_emu_test.cpp -- stage_segments_kernel (ngmlr_amd/csrc/cvx_qry_stage.hip) compiled for the host and run one lane at a
 * time, every lane of every workgroup in turn, against stage_segments_host: the kernel's chunk indexing, its 16-byte pieces with
 * their byte-wise heads and tails, and its two v_perm_b32 tables (emulated, tests/cpp/hip_host_stub).  Built with
 * -fsanitize=address,undefined by tests/test_qry_stage_emu_cpu.py: the read block the kernel sees is allocated to the byte (no
 * NUL behind the last read, nothing in front of the first) and its reads lie 32 POISONED guard bytes apart, so a load that leaves
 * its own read -- into a neighbour's direction or off the block -- is a report; every destination lies between guard bytes that
 * must come back untouched.
 * No device, no HIP: what it cannot show is anything the compiler for gfx950 does differently.
 */
#include <algorithm>
#include <string>
#include <vector>

#include "../../ngmlr_amd/csrc/cvx_qry_stage.hip"

#if defined(__has_include)
#if __has_include(<sanitizer/asan_interface.h>)
#include <sanitizer/asan_interface.h>
#endif
#endif
#ifndef ASAN_POISON_MEMORY_REGION
#define ASAN_POISON_MEMORY_REGION(p, n) ((void) (p), (void) (n))
#define ASAN_UNPOISON_MEMORY_REGION(p, n) ((void) (p), (void) (n))
#endif

using namespace cvx;

static int fails = 0;
static long long n_strings = 0, n_bytes = 0;

struct Seg { int read, start, len, flags; unsigned phase; };

/* the segments of one case over `reads`, every destination at its own phase with at least 16 guard bytes on either side */
static void run_case(const char *name, const std::vector<std::string> &reads, const std::vector<Seg> &segs) {
	std::vector<uint8_t> arena;
	std::vector<uint64_t> off(1, 0);
	for (const std::string &r : reads) { arena.insert(arena.end(), r.begin(), r.end()); arena.push_back(0); off.push_back(arena.size()); }
	const int n = (int) segs.size();
	std::vector<cvx_read_segment> rs((size_t) n);
	std::vector<uint64_t> dst((size_t) n);
	uint64_t at = 0;
	for (int i = 0; i < n; ++i) {
		rs[(size_t) i] = {segs[(size_t) i].read, segs[(size_t) i].start, segs[(size_t) i].flags, 0};
		dst[(size_t) i] = at + 16 + segs[(size_t) i].phase;
		at = (dst[(size_t) i] + (uint64_t) segs[(size_t) i].len + 16 + 15) / 16 * 16;
	}
	SegPlan pl;
	int64_t bad = 0;
	if (segments_plan((int32_t) reads.size(), off.data(), n, rs.data(), [&](int32_t i) { return segs[(size_t) i].len; },
			[&](int32_t i) { return dst[(size_t) i]; }, pl, &bad) != CVX_OK) { printf("%s: plan failed at %lld\n", name, (long long) bad); ++fails; return; }
	const size_t cap = ((size_t) at + 256 + 255) / 256 * 256;
	std::vector<uint8_t> want(cap, 0xA5);
	stage_segments_host(arena.data(), pl.desc, want.data());
	/* the kernel's read block: to the byte, no NUL behind the last read, and a poisoned guard between neighbours (the
	 * descriptors' source offsets follow the reads to their places) */
	const size_t kGuard = 32;
	std::vector<size_t> base;
	size_t rbytes = 0;
	for (const std::string &r : reads) { base.push_back(rbytes); rbytes += r.size() + kGuard; }
	rbytes -= kGuard;
	uint8_t *rd = (uint8_t *) malloc(rbytes ? rbytes : 1);
	memset(rd, 0x5A, rbytes);
	for (size_t r = 0; r < reads.size(); ++r) {
		memcpy(rd + base[r], reads[r].data(), reads[r].size());
		if (r + 1 < reads.size()) ASAN_POISON_MEMORY_REGION(rd + base[r] + reads[r].size(), kGuard);
	}
	std::vector<SegDesc> kdesc = pl.desc;
	for (int i = 0; i < n; ++i) kdesc[(size_t) i].src_off = base[(size_t) segs[(size_t) i].read] + (uint64_t) segs[(size_t) i].start;
	uint8_t *seq = (uint8_t *) aligned_alloc(256, cap);      /* aligned like a device allocation: offsets are addresses modulo 16 */
	memset(seq, 0xA5, cap);
	const int nc = (int) pl.chunks.size();
	for (int b = 0; b < (nc + 3) / 4; ++b)
		for (int t = 0; t < 256; ++t) {
			blockIdx.x = (unsigned) b; threadIdx.x = (unsigned) t;
			stage_segments_kernel(rd, kdesc.data(), pl.chunks.data(), nc, seq);
		}
	int diffs = 0;
	for (size_t k = 0; k < cap; ++k) if (seq[k] != want[k] && ++diffs < 6) printf("%s: byte %zu: %02x, want %02x\n", name, k, seq[k], want[k]);
	ASAN_UNPOISON_MEMORY_REGION(rd, rbytes ? rbytes : 1);
	free(seq); free(rd);
	if (diffs) { printf("%s: %d differences\n", name, diffs); ++fails; }
	n_strings += n; n_bytes += (long long) pl.seg_bytes;
}

int main() {
	uint32_t rsd = 11;
	auto rnd = [&]() { rsd = rsd * 1664525u + 1013904223u; return rsd >> 8; };
	auto mixed = [&](int len) { std::string s; for (int k = 0; k < len; ++k) s.push_back("ACGTNacgtnRY*-ACGTACGT"[rnd() % 22]); return s; };

	/* every byte value in every position of a dword, both directions, the read's dwords at every offset against the loads (start
	 * 0..3) and every destination phase.  (The host's strings carry byte 0 like any other; the NULs of the block are outside.) */
	{
		std::string r;
		for (int p = 0; p < 4; ++p)
			for (int v = 0; v < 256; ++v) { char q[4] = {'A', 'C', 'G', 'T'}; q[p] = (char) v; r.append(q, 4); }
		std::vector<Seg> segs;
		for (int start = 0; start < 4; ++start)
			for (unsigned ph = 0; ph < 16; ++ph)
				for (int f = 0; f < 2; ++f) segs.push_back({0, start, (int) r.size() - start, f, ph});
		run_case("byte values", {r}, segs);
	}
	/* every source misalignment x destination phase, the lengths around one and two pieces, both directions */
	{
		const std::string r = mixed(80);
		std::vector<Seg> segs;
		for (int start = 0; start < 16; ++start)
			for (unsigned ph = 0; ph < 16; ++ph)
				for (int len : {1, 15, 16, 17, 31, 32, 33, 64})
					for (int f = 0; f < 2; ++f) segs.push_back({0, start, len, f, ph});
		run_case("misalignment x phase", {r}, segs);
	}
	/* around the chunk: one piece less, exact, one more, two chunks and their neighbours; flush with the read's start and with its
	 * end, and the whole read */
	{
		const int C = kSegChunkPieces * kSegPiece;
		for (int len : {C - 17, C - 16, C - 1, C, C + 1, C + 15, C + 16, C + 17, 2 * C - 1, 2 * C, 2 * C + 1, 3 * C + 5}) {
			const std::string r = mixed(len + 23);
			std::vector<Seg> segs;
			for (unsigned ph : {0u, 1u, 7u, 15u})
				for (int f = 0; f < 2; ++f) {
					segs.push_back({0, 0, len, f, ph});                          /* flush with the start */
					segs.push_back({0, 23, len, f, ph});                         /* flush with the end */
					segs.push_back({0, 0, len + 23, f, ph});                     /* the whole read */
					segs.push_back({0, 11, len, f, ph});
				}
			run_case("chunk boundary", {r}, segs);
		}
	}
	/* short reads flush at both ends (a read of exactly the segment's length, alone in its block): lengths 1 .. 70 */
	for (int len = 1; len <= 70; ++len) {
		const std::string r = mixed(len);
		std::vector<Seg> segs;
		for (unsigned ph = 0; ph < 16; ++ph)
			for (int f = 0; f < 2; ++f) segs.push_back({0, 0, len, f, ph});
		run_case("whole short read", {r}, segs);
	}
	/* several reads in one block, several tiles per read, mixed flags, empty strings among them */
	{
		std::vector<std::string> reads;
		for (int len : {1, 300, 17, 5000, 64, 1500}) reads.push_back(mixed(len));
		std::vector<Seg> segs;
		for (int k = 0; k < 400; ++k) {
			const int r = (int) (rnd() % reads.size()), L = (int) reads[(size_t) r].size();
			const int start = (int) (rnd() % (unsigned) (L + 1)), len = (int) (rnd() % (unsigned) (L - start + 1));
			segs.push_back({r, start, k % 37 == 0 ? 0 : len, (int) (rnd() & 1), rnd() % 16});
		}
		run_case("read block", reads, segs);
	}
	if (fails) { printf("qry_stage_emu_test: %d cases failed\n", fails); return 1; }
	printf("qry_stage_emu_test: ok (%lld strings, %lld bytes)\n", n_strings, n_bytes);
	return 0;
}
