/*
 * search_score_shim_test.cpp -- CandidateSearchHip::SearchAndScore against CandidateSearchHip::Search followed by
 * StrippedSWHip::BatchScoreWindows on the pairs built on the host from the lists, over a small two-contig genome with a repeat
 * (a list that reaches maxCmrs) and reads at the contigs' ends.  On every logical device of the process (CVX_ALIAS_DEVICES=2:
 * the searcher and a scorer per device share ONE upload of the genome there: Convex::DeviceGenome::Uploads).
 * tests/test_gpu_shim_search_score.py runs it.
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "candidate_search_hip.h"
#include "convex_align_hip.h"
#include "device_genome.h"
#include "service_device.h"
#include "stripped_sw_hip.h"

namespace {

std::string revcomp(std::string const & s) {
	std::string r(s.rbegin(), s.rend());
	for (char & c : r) c = c == 'A' ? 'T' : c == 'T' ? 'A' : c == 'C' ? 'G' : c == 'G' ? 'C' : c;
	return r;
}

int const kBufferLen = 308, kLead = 20, kMaxCmrs = 4;
int g_bad = 0;

/* one CS thread: its logical device is the order in which threads first ask (service_device.h) */
void run(Convex::CandidateSearchHip * search, std::vector<std::string> const * reads, int * deviceOut) {
	int const dv = Convex::ServiceDeviceOfThisThread();
	*deviceOut = dv;
	StrippedSWHip scorer(dv);
	Convex::CandidateSearchHip::Batch a, b;
	for (std::string const & r : *reads) { a.seqs.push_back(r.c_str()); a.lens.push_back((int32_t) r.size()); }
	b.seqs = a.seqs; b.lens = a.lens;
	search->SearchAndScore(a, 0.8f, 0.0f, 4, 16, kBufferLen, kLead, kMaxCmrs);
	search->Search(b, 0.8f, 0.0f, 4, 16);
	size_t const n = reads->size();
	uint64_t used = 0;
	for (size_t i = 0; i < n; ++i) {
		if (a.nCand[i] != b.nCand[i] || a.begin[i] != b.begin[i] || a.maxHit[i] != b.maxHit[i] || a.kmerMisses[i] != b.kmerMisses[i] || a.attempts[i] != b.attempts[i]) {
			printf("device %d read %zu: the search's outputs differ (%d / %d candidates)\n", dv, i, a.nCand[i], b.nCand[i]); ++g_bad;
		}
		if (b.nCand[i] > 0) used += (uint64_t) b.nCand[i];
	}
	if (used && memcmp(a.cands.data(), b.cands.data(), (size_t) used * sizeof(cvx_candidate)) != 0) { printf("device %d: the lists differ\n", dv); ++g_bad; }
	/* the second call of the two-call path: one pair per candidate of every list shorter than maxCmrs */
	std::vector<cvx_score_window> pairs;
	std::vector<uint64_t> owner;
	std::vector<int> want_status((size_t) used, 0);
	for (size_t i = 0; i < n; ++i)
		for (int k = 0; k < b.nCand[i]; ++k) {
			uint64_t const q = b.begin[i] + (uint64_t) k;
			if (b.nCand[i] >= kMaxCmrs) { want_status[(size_t) q] = 2; continue; }
			cvx_score_window w;
			w.position = b.cands[(size_t) q].location - (uint64_t) kLead; w.buffer_len = kBufferLen; w.read = (int32_t) i; w.reverse = b.cands[(size_t) q].reverse;
			pairs.push_back(w); owner.push_back(q);
		}
	std::vector<float> want((size_t) used, -1.0f), got(pairs.size(), -2.0f);
	std::vector<int> st(pairs.size(), -1);
	if (!pairs.empty()) scorer.BatchScoreWindows((int) n, a.arena.data(), (unsigned long long const *) a.offsets.data(), (int) pairs.size(), pairs.data(), got.data(), st.data());
	for (size_t p = 0; p < pairs.size(); ++p) { want[(size_t) owner[p]] = got[p]; want_status[(size_t) owner[p]] = st[p]; }
	int scored = 0, dropped = 0, failed = 0;
	for (uint64_t q = 0; q < used; ++q) {
		if (a.swStatus[(size_t) q] != want_status[(size_t) q]) { printf("device %d candidate %llu: status %d, want %d\n", dv, (unsigned long long) q, a.swStatus[(size_t) q], want_status[(size_t) q]); ++g_bad; }
		if (memcmp(&a.swScores[(size_t) q], &want[(size_t) q], 4) != 0) { printf("device %d candidate %llu: %g, the two calls give %g\n", dv, (unsigned long long) q, a.swScores[(size_t) q], want[(size_t) q]); ++g_bad; }
		scored += want_status[(size_t) q] == 0; failed += want_status[(size_t) q] == 1; dropped += want_status[(size_t) q] == 2;
	}
	if (scored < 6 || dropped < 4) { printf("device %d: %d scored, %d of dropped lists: the case is not what it was built to be\n", dv, scored, dropped); ++g_bad; }
	printf("device %d: %llu candidates, %d scored, %d without a window, %d of dropped lists, %ld genome uploads\n", dv, (unsigned long long) used, scored, failed, dropped,
			Convex::DeviceGenome::Uploads(dv));
	if (Convex::DeviceGenome::Uploads(dv) != 1) { printf("device %d: %ld uploads of the genome, expected 1\n", dv, Convex::DeviceGenome::Uploads(dv)); ++g_bad; }
}

}  // namespace

int main() {
	uint32_t rs = 99;
	auto rnd = [&]() { rs = rs * 1664525u + 1013904223u; return rs >> 8; };
	auto random_seq = [&](int n) { std::string s; for (int k = 0; k < n; ++k) s.push_back("ACGT"[rnd() % 4]); return s; };
	std::string a = random_seq(2301), b = random_seq(1800);
	std::string const unit = random_seq(256);
	a.replace(500, 256, unit); a.replace(1100, 256, unit);
	b.replace(400, 256, unit); b.replace(1000, 256, unit);
	char const * sp[2] = { a.c_str(), b.c_str() };
	uint64_t lens[2] = { a.size(), b.size() };
	std::vector<uint8_t> bin((size_t) cvx_genome_encoded_bytes(2, lens));
	uint64_t nNibbles = 0, starts[3];
	int32_t nStarts = 0;
	if (cvx_genome_encode(2, sp, lens, bin.data(), &nNibbles, starts, &nStarts) != CVX_OK) { printf("encode failed\n"); return 1; }
	int const k = 13;
	std::vector<uint8_t> index((((size_t) 1 << (2 * k)) + 2) * 5);
	std::vector<uint32_t> locs((a.size() + b.size()) / 3 + 64);
	uint64_t nLocs = 0;
	if (cvx_index_build(bin.data(), nNibbles, starts, lens, 2, k, 2, 4, index.data(), locs.data(), locs.size(), &nLocs) != CVX_OK) { printf("cvx_index_build: %s\n", cvx_last_error()); return 1; }
	Convex::DeviceWindows::SetGenome(bin.data(), nNibbles, (unsigned long long const *) starts, nStarts);

	std::vector<std::string> reads = { a.substr(0, 256), revcomp(a.substr(0, 256)), unit, a.substr(a.size() - 256), std::string(256, 'N'),
			b.substr(0, 256), revcomp(unit), b.substr(b.size() - 256), revcomp(b.substr(b.size() - 256)), a.substr(1500, 200) };
	int nl = 0, np = 0;
	Convex::DeviceLayout(nl, np);
	if (nl < 1) { printf("no device\n"); return 1; }
	Convex::CandidateSearchHip * search = Convex::CandidateSearchHip::Get(k, index.data(), locs.data(), (uint32_t) nLocs, 0);
	std::vector<int> device((size_t) nl, -1);
	for (int t = 0; t < nl; ++t) {      /* one thread per logical device, one after the other: thread t is dealt device t */
		std::thread th(run, search, &reads, &device[(size_t) t]);
		th.join();
		if (device[(size_t) t] != t) { printf("thread %d ran on device %d\n", t, device[(size_t) t]); ++g_bad; }
	}
	/* the scorers are gone, the searcher still uses the genome: a second round uploads nothing */
	for (int t = 0; t < nl; ++t) if (Convex::DeviceGenome::Uploads(t) != 1) { printf("device %d: %ld uploads after the scorers went\n", t, Convex::DeviceGenome::Uploads(t)); ++g_bad; }
	Convex::CandidateSearchHip::Shutdown();
	if (g_bad) { printf("search_score_shim_test: %d differences\n", g_bad); return 1; }
	printf("search_score_shim_test: ok\n");
	return 0;
}
