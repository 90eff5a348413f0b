/*
 * score_stage_emu_test.cpp -- stage_score_windows_kernel (ngmlr_amd/csrc/cvx_score_stage.hip) compiled for the host and run one
 * lane at a time, every lane of every workgroup in turn, against score_windows_stage_host: the kernel's indexing, its 16-byte
 * pieces with their byte-wise heads and tails, and its two v_perm_b32 tables (emulated, tests/cpp/hip_host_stub).  Built with
 * -fsanitize=address,undefined by tests/test_score_stage_emu_cpu.py: the genome and the read block are allocated to the byte
 * (the genome without the 64 bytes cvx_genome_upload allocates behind it), so a load outside them is a report.
 * No device, no HIP: what it cannot show is anything the compiler for gfx950 does differently.
 */
#include <algorithm>
#include <string>
#include <vector>

#include "../../ngmlr_amd/csrc/cvx_score_stage.hip"

using namespace cvx;

int main() {
	uint32_t rs = 7;
	auto rnd = [&]() { rs = rs * 1664525u + 1013904223u; return rs >> 8; };
	std::vector<uint8_t> bin(500, 0x44);
	for (int n : {37, 64, 1001}) {
		std::vector<unsigned> c;
		for (int k = 0; k < n; ++k) c.push_back(rnd() % 29 == 0 ? 4u : rnd() % 4u);
		if (n & 1) c.push_back(4u);
		for (size_t k = 0; k < c.size(); k += 2) bin.push_back((uint8_t) ((c[k] << 4) | c[k + 1]));
		bin.insert(bin.end(), 500, 0x44);
	}
	const uint64_t L = score_windows_concat_len(bin.size() * 2);
	/* (no tail behind the genome here, though cvx_genome_upload allocates one: the kernel's loads must not need it) */
	std::vector<uint8_t> arena;
	std::vector<uint64_t> off(1, 0);
	for (int len : {1, 15, 16, 17, 31, 33, 40, 255, 256, 257, 600}) {
		for (int k = 0; k < len; ++k) arena.push_back((uint8_t) "ACGTNacgtR*-"[rnd() % 12]);
		arena.push_back(0);
		off.push_back(arena.size());
	}
	const int n_reads = (int) off.size() - 1;
	std::vector<cvx_score_window> pairs;
	for (uint64_t pos = 0; pos < L + 3; pos += 1 + rnd() % 7)
		for (int bl : {3, 4, 5, 17, 40, 41, 308, 309, 600, 1300})
			if (rnd() % 3 == 0) pairs.push_back({pos, bl, (int32_t) (rnd() % (unsigned) n_reads), (int32_t) (rnd() & 1)});
	for (uint64_t k = 1; k <= 45; ++k)
		for (int bl = 3; bl < 70; ++bl) pairs.push_back({L - k, bl, (int32_t) (rnd() % (unsigned) n_reads), (int32_t) (rnd() & 1)});
	pairs.push_back({(uint64_t) 5 - 20, 308, 0, 1});
	const int n = (int) pairs.size();
	ScoreWinPlan pl;
	int64_t bad = 0;
	if (score_windows_plan(L, n_reads, off.data(), n, pairs.data(), false, pl, &bad) != CVX_OK) { printf("plan failed\n"); return 1; }
	std::vector<uint8_t> want((size_t) pl.seq_bytes);
	if (!score_windows_stage_host(bin.data(), L, pairs.data(), pl, arena.data(), want.data())) { printf("host strings failed\n"); return 1; }
	const size_t cap = ((size_t) pl.seq_bytes + 256 + 255) / 256 * 256;
	uint8_t *seq = (uint8_t *) aligned_alloc(256, cap);      /* aligned like a device allocation: offsets are addresses modulo 16 */
	memset(seq, 0xA5, cap);
	std::vector<ScorePair> sp((size_t) n);
	for (int b = 0; b < (n + 3) / 4; ++b)
		for (int t = 0; t < 256; ++t) {
			blockIdx.x = (unsigned) b; threadIdx.x = (unsigned) t;
			stage_score_windows_kernel(bin.data(), arena.data(), pl.desc.data(), n, seq, sp.data());
		}
	int diffs = 0;
	for (size_t k = 0; k < pl.seq_bytes; ++k) if (seq[k] != want[k] && ++diffs < 10) printf("byte %zu: %02x, want %02x\n", k, seq[k], want[k]);
	for (size_t k = (size_t) pl.seq_bytes; k < cap; ++k) if (seq[k] != 0xA5) { ++diffs; printf("a store behind the arena, at %zu\n", k); break; }
	for (int s = 0; s < n; ++s) {
		const ScoreWinDesc &d = pl.desc[(size_t) s];
		const ScorePair &p = sp[(size_t) s];
		if (p.ref_off != d.ref_off || p.qry_off != d.qry_off || p.ref_len != d.ref_chars + 1 || p.qry_len != d.read_len + 1 || p.scratch_off != d.scratch_off) { ++diffs; printf("ScorePair %d\n", s); }
	}
	free(seq);
	if (diffs) { printf("score_stage_emu_test: %d differences\n", diffs); return 1; }
	printf("score_stage_emu_test: ok (%d pairs, %llu bytes)\n", n, (unsigned long long) pl.seq_bytes);
	return 0;
}
