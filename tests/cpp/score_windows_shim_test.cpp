/*
 * score_windows_shim_test.cpp -- StrippedSWHip::BatchScoreWindows against StrippedSWHip::BatchScore on host-built strings
 * (cvx_stage_windows_host), over engineered windows of a small genome: every parity of position and buffer length, windows in
 * and across the N spacers, the end of the genome, positions whose decode fails.  On every logical device of the process
 * (CVX_ALIAS_DEVICES=2: two scorers, one genome each).  tests/test_gpu_shim_score_windows.py runs it.
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "convex_align_hip.h"
#include "service_device.h"
#include "stripped_sw_hip.h"

int main() {
	uint32_t rs = 4242;
	auto rnd = [&]() { rs = rs * 1664525u + 1013904223u; return rs >> 8; };
	std::vector<std::string> seqs;
	for (int n : {37, 64, 1001}) {
		std::string s;
		for (int k = 0; k < n; ++k) s.push_back("ACGTN"[rnd() % 53 == 0 ? 4 : rnd() % 4]);
		seqs.push_back(s);
	}
	std::vector<char const *> sp;
	std::vector<uint64_t> lens;
	for (std::string const & s : seqs) { sp.push_back(s.c_str()); lens.push_back(s.size()); }
	std::vector<uint8_t> bin((size_t) cvx_genome_encoded_bytes(3, lens.data()));
	uint64_t nNibbles = 0, starts[4];
	int32_t nStarts = 0;
	if (cvx_genome_encode(3, sp.data(), lens.data(), bin.data(), &nNibbles, starts, &nStarts) != CVX_OK) { printf("encode failed\n"); return 1; }
	uint64_t L = 0;
	cvx_genome_concat_len(nNibbles, starts, nStarts, &L);
	Convex::DeviceWindows::SetGenome(bin.data(), nNibbles, (unsigned long long const *) starts, nStarts);

	/* reads: a piece of the third sequence (so that scores are not all noise), its neighbours in length, one with other bytes */
	std::vector<uint8_t> arena;
	std::vector<uint64_t> offsets(1, 0);
	for (int len : {256, 40, 255, 257, 1}) {
		for (int k = 0; k < len; ++k) arena.push_back((uint8_t) (k < 200 ? seqs[2][(size_t) (100 + k)] : "ACGTNacgtR*"[rnd() % 11]));
		arena.push_back(0);
		offsets.push_back(arena.size());
	}
	int const nReads = (int) offsets.size() - 1;
	std::vector<cvx_score_window> pairs;
	uint64_t const s2 = starts[2];
	auto add = [&](uint64_t pos, int32_t bl) { int32_t const k = (int32_t) pairs.size(); pairs.push_back({pos, bl, k % nReads, (k / nReads) & 1}); };
	for (uint64_t pos : {s2 + 98, s2 + 99}) for (int32_t bl : {40, 41, 3, 4, 5, 17, 308, 600}) add(pos, bl);
	add(0, 308); add(1, 17); add(s2 - 202, 308); add(s2 + 799, 307); add(starts[1] - 38, 1200); add(starts[1] - 600, 308);
	for (uint64_t k = 40; k >= 1; --k) { add(L - k, 60 + (int32_t) (k % 3)); add(L - k, (int32_t) k + 2); }
	add(L - 1, 308); add(L, 308); add(L + 5, 308); add((uint64_t) 5 - 20, 308);
	int const n = (int) pairs.size();

	std::vector<uint8_t> out((size_t) n * 1600);
	std::vector<uint64_t> ro((size_t) n), qo((size_t) n);
	std::vector<int32_t> hostStatus((size_t) n);
	uint64_t used = 0;
	if (cvx_stage_windows_host(bin.data(), nNibbles, starts, nStarts, nReads, arena.data(), offsets.data(), n, pairs.data(), out.data(), out.size(),
			ro.data(), qo.data(), hostStatus.data(), &used) != CVX_OK) { printf("cvx_stage_windows_host: %s\n", cvx_last_error()); return 1; }
	std::vector<char const *> refs, qrys;
	std::vector<int> which;
	for (int i = 0; i < n; ++i) if (!hostStatus[(size_t) i]) { refs.push_back((char const *) out.data() + ro[(size_t) i]); qrys.push_back((char const *) out.data() + qo[(size_t) i]); which.push_back(i); }

	int nl = 0, np = 0, bad = 0;
	Convex::DeviceLayout(nl, np);
	if (nl < 1) { printf("no device\n"); return 1; }
	{
		std::vector<StrippedSWHip *> scorers;
		for (int d = 0; d < nl; ++d) scorers.push_back(new StrippedSWHip(d));
		for (int d = 0; d < nl; ++d) {
			std::vector<float> want(refs.size(), -2.0f), got((size_t) n, -2.0f);
			std::vector<int> status((size_t) n, -1);
			scorers[(size_t) d]->BatchScore(0, (int) refs.size(), refs.data(), qrys.data(), want.data(), 0);
			int const rc = scorers[(size_t) d]->BatchScoreWindows(nReads, arena.data(), (unsigned long long const *) offsets.data(), n, pairs.data(), got.data(), status.data());
			if (rc != n) { printf("device %d: BatchScoreWindows returned %d\n", d, rc); ++bad; }
			size_t w = 0;
			int failed = 0;
			for (int i = 0; i < n; ++i) {
				if (status[(size_t) i] != hostStatus[(size_t) i]) { printf("device %d pair %d: status %d, host %d\n", d, i, status[(size_t) i], hostStatus[(size_t) i]); ++bad; continue; }
				if (status[(size_t) i]) { ++failed; if (got[(size_t) i] != -1.0f) { printf("device %d pair %d: failed decode scored %g\n", d, i, got[(size_t) i]); ++bad; } continue; }
				if (memcmp(&got[(size_t) i], &want[w], 4) != 0) { printf("device %d pair %d: %g, strings give %g\n", d, i, got[(size_t) i], want[w]); ++bad; }
				++w;
			}
			if (failed != 3) { printf("device %d: %d failed decodes, expected 3\n", d, failed); ++bad; }
			printf("device %d of %d: %d pairs, %d failed decodes\n", d, nl, n, failed);
		}
		for (StrippedSWHip * s : scorers) delete s;
	}
	if (bad) { printf("score_windows_shim_test: %d differences\n", bad); return 1; }
	printf("score_windows_shim_test: ok\n");
	return 0;
}
