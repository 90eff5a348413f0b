/*
 * ladder_merge_test.cpp -- the merge rule of a ladder job's per-rung stage outputs (cvx::ladder_merge_plan / ladder_merge_records,
 * ngmlr_amd/csrc/cvx_ladder_merge.h) as a program of its own: host code only, no device, no library, never loaded into Python
 * (tests/test_ladder_merge_cpu.py builds it plain and under -fsanitize=address,undefined).
 *
 * Seeded ladders of one to five rungs are built the way a job builds them -- every rung lists, in the previous rung's order, the
 * tiles that climb to it -- each rung's arena is filled with items that name their (rung, entry, index), allocated at exactly its
 * size, and the merged arena is compared with a straightforward per-tile rebuild: tile after tile, item after item.
 */
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "cvx_ladder_merge.h"

using cvx::LadderSpan;

static int g_fail = 0;
static int g_reported[6][5];      /* [rungs of the ladder][rung]: cases in which that rung reported a tile */
#define CHECK(cond, ...) do { if (!(cond)) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); ++g_fail; } } while (0)

static uint64_t g_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() { g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17; return (uint32_t) (g_state >> 11); }

struct Item { int32_t rung, entry; uint32_t k; uint32_t pad; };
struct Rec { int32_t rung, entry; };

struct Rung {
	std::vector<int32_t> tile;          /* job tile of every entry */
	std::vector<uint64_t> off;          /* entries + 1 */
	std::vector<Item> arena;            /* exactly off.back() items */
	std::vector<Rec> rec;               /* one per entry */
};

/* mode 0: random counts; 1: no tile has an item; 2: only the failed last attempts (tiles still live on the last rung) have none */
static void build(int n, int n_rungs, int climb_pct, int mode, std::vector<Rung> &rungs, std::vector<int32_t> &rung_of, std::vector<int32_t> &at) {
	rungs.assign((size_t) n_rungs, Rung());
	rung_of.assign((size_t) n, 0);
	at.assign((size_t) n, 0);
	for (int i = 0; i < n; ++i) rungs[0].tile.push_back(i);
	for (int r = 1; r < n_rungs; ++r)
		for (size_t j = 0; j < rungs[(size_t) r - 1].tile.size(); ++j)
			if ((int) (rnd() % 100u) < climb_pct || (j == 0 && r < n_rungs)) rungs[(size_t) r].tile.push_back(rungs[(size_t) r - 1].tile[j]);      /* (entry 0 always climbs: every rung is reported by a tile) */
	for (int r = 0; r < n_rungs; ++r) {
		Rung &R = rungs[(size_t) r];
		for (size_t j = 0; j < R.tile.size(); ++j) { rung_of[(size_t) R.tile[j]] = r; at[(size_t) R.tile[j]] = (int32_t) j; }
	}
	for (int r = 0; r < n_rungs; ++r) {
		Rung &R = rungs[(size_t) r];
		R.off.assign(R.tile.size() + 1, 0);
		for (size_t j = 0; j < R.tile.size(); ++j) {
			const bool reported_here = rung_of[(size_t) R.tile[j]] == r;
			uint64_t count = rnd() % 4u == 0 ? 0 : rnd() % 7u;
			if (rnd() % 50u == 0) count = 200 + rnd() % 300u;
			if (mode == 1) count = 0;
			if (mode == 2 && reported_here && r == n_rungs - 1) count = 0;      /* the last attempt failed: no items */
			if (!reported_here && mode != 1) count = rnd() % 5u;                  /* an attempt that failed may still have left items nobody reports */
			R.off[j + 1] = R.off[j] + count;
		}
		R.arena.resize((size_t) R.off.back());
		R.rec.resize(R.tile.size());
		for (size_t j = 0; j < R.tile.size(); ++j) {
			R.rec[j].rung = r; R.rec[j].entry = (int32_t) j;
			for (uint64_t k = R.off[j]; k < R.off[j + 1]; ++k) { Item it = { r, (int32_t) j, (uint32_t) (k - R.off[j]), 0u }; R.arena[(size_t) k] = it; }
		}
	}
}

static void run_case(int n, int n_rungs, int climb_pct, int mode) {
	std::vector<Rung> rungs;
	std::vector<int32_t> rung_of, at;
	build(n, n_rungs, climb_pct, mode, rungs, rung_of, at);
	std::vector<const uint64_t *> off((size_t) n_rungs);
	std::vector<const void *> rec((size_t) n_rungs);
	std::vector<int32_t> rn((size_t) n_rungs);
	for (int r = 0; r < n_rungs; ++r) { off[(size_t) r] = rungs[(size_t) r].off.data(); rec[(size_t) r] = rungs[(size_t) r].rec.data(); rn[(size_t) r] = (int32_t) rungs[(size_t) r].tile.size(); }
	std::vector<uint64_t> merged((size_t) n + 1, 0xdeadbeefull);
	std::vector<LadderSpan> spans;
	const bool ok = cvx::ladder_merge_plan(n, rung_of.data(), at.data(), n_rungs, off.data(), rn.data(), merged.data(), spans);
	CHECK(ok, "plan refused n %d rungs %d", n, n_rungs);
	if (!ok) return;
	/* the straightforward rebuild */
	std::vector<uint64_t> want_off((size_t) n + 1, 0);
	std::vector<Item> want;
	for (int i = 0; i < n; ++i) {
		const Rung &R = rungs[(size_t) rung_of[(size_t) i]];
		const size_t j = (size_t) at[(size_t) i];
		for (uint64_t k = R.off[j]; k < R.off[j + 1]; ++k) want.push_back(R.arena[(size_t) k]);
		want_off[(size_t) i + 1] = want.size();
	}
	CHECK(merged == want_off, "offsets differ: n %d rungs %d mode %d", n, n_rungs, mode);
	std::vector<Item> got((size_t) merged[(size_t) n]);      /* exactly the merged total: a span past it is the sanitizer's */
	std::vector<uint8_t> covered(got.size(), 0);
	uint64_t next = 0;
	for (const LadderSpan &s : spans) {
		CHECK(s.len > 0 && s.rung >= 0 && s.rung < n_rungs, "span rung %d len %llu", s.rung, (unsigned long long) s.len);
		CHECK(s.dst == next, "spans are not dense in destination order: %llu after %llu", (unsigned long long) s.dst, (unsigned long long) next);
		CHECK(s.src + s.len <= rungs[(size_t) s.rung].arena.size() && s.dst + s.len <= got.size(), "span outside an arena");
		if (s.src + s.len > rungs[(size_t) s.rung].arena.size() || s.dst + s.len > got.size()) return;
		memcpy(got.data() + s.dst, rungs[(size_t) s.rung].arena.data() + s.src, (size_t) s.len * sizeof(Item));
		for (uint64_t k = 0; k < s.len; ++k) covered[(size_t) (s.dst + k)] += 1;
		next = s.dst + s.len;
	}
	CHECK(next == got.size(), "spans end at %llu of %zu", (unsigned long long) next, got.size());
	for (size_t k = 0; k < covered.size(); ++k) CHECK(covered[k] == 1, "item %zu written %d times", k, covered[k]);
	CHECK(got.size() == want.size() && (got.empty() || memcmp(got.data(), want.data(), got.size() * sizeof(Item)) == 0), "merged arena differs: n %d rungs %d mode %d", n, n_rungs, mode);
	std::vector<Rec> recs((size_t) n);
	cvx::ladder_merge_records(n, rung_of.data(), at.data(), rec.data(), sizeof(Rec), recs.data());
	std::vector<int> reported((size_t) n_rungs, 0);
	for (int i = 0; i < n; ++i) {
		CHECK(recs[(size_t) i].rung == rung_of[(size_t) i] && recs[(size_t) i].entry == at[(size_t) i], "record of tile %d", i);
		reported[(size_t) rung_of[(size_t) i]] += 1;
	}
	for (int r = 0; r < n_rungs; ++r) if (reported[(size_t) r] > 0) g_reported[n_rungs][r] += 1;
}

int main() {
	int cases = 0;
	for (int n_rungs = 1; n_rungs <= 5; ++n_rungs)
		for (int n : { 0, 1, 2, 7, 64, 300 })
			for (int pct : { 0, 30, 70, 100 })
				for (int mode = 0; mode < 3; ++mode)
					for (int rep = 0; rep < 3; ++rep) { run_case(n, n_rungs, pct, mode); ++cases; }
	for (int n_rungs = 1; n_rungs <= 5; ++n_rungs)
		for (int r = 0; r < n_rungs; ++r) CHECK(g_reported[n_rungs][r] >= 10, "rung %d of %d reported a tile in %d cases only", r + 1, n_rungs, g_reported[n_rungs][r]);
	/* what the plan refuses: a rung or an entry that does not exist, offsets that descend */
	{
		const uint64_t o0[] = { 0, 2, 5 }, bad[] = { 0, 4, 3 };
		const uint64_t *offs[] = { o0 };
		const uint64_t *boffs[] = { bad };
		const int32_t rn[] = { 2 };
		uint64_t merged[3];
		std::vector<LadderSpan> spans;
		int32_t r0[] = { 0, 0 }, a0[] = { 0, 1 }, r1[] = { 0, 1 }, a1[] = { 0, 2 }, am[] = { 0, -1 };
		CHECK(cvx::ladder_merge_plan(2, r0, a0, 1, offs, rn, merged, spans) && merged[2] == 5 && spans.size() == 1 && spans[0].len == 5, "the plain case: one span");
		CHECK(!cvx::ladder_merge_plan(2, r1, a0, 1, offs, rn, merged, spans), "a rung that does not exist");
		CHECK(!cvx::ladder_merge_plan(2, r0, a1, 1, offs, rn, merged, spans), "an entry that does not exist");
		CHECK(!cvx::ladder_merge_plan(2, r0, am, 1, offs, rn, merged, spans), "a negative entry");
		CHECK(!cvx::ladder_merge_plan(2, r0, a0, 1, boffs, rn, merged, spans), "offsets that descend");
		uint64_t m0[1] = { 7 };
		CHECK(cvx::ladder_merge_plan(0, nullptr, nullptr, 1, offs, rn, m0, spans) && m0[0] == 0 && spans.empty(), "n = 0");
	}
	if (g_fail) { printf("ladder_merge_test: %d failures\n", g_fail); return 1; }
	printf("ladder_merge_test: ok (%d cases)\n", cases);
	return 0;
}
