// The tail split of build_schedule (cvx_host_logic.h): a whole-tile class whose last tiles are filled by a launch of their own.
// Mixed batches as tests/cpp/host_logic_test.cpp builds them (+ gang tiles) and one-class batches of 1, 2, 600 and 49 300 tiles, each
// under tail sizes 0, 1, count - n_direct - 1 and count - n_direct of every whole-tile class, and more than the batch; then the
// thresholds of the automatic rule.  Host only, plain g++ (tests/test_tail_split_cpu.py).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <set>
#include <vector>

#include "cvx_host_logic.h"

using namespace cvx;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

struct Batch {
	std::vector<TilePlan> plan; std::vector<TileIn> tin; uint64_t n_rows = 0;
	void add(std::mt19937 &rng, int need, int H, int steps, uint32_t flags = 0) {
		TilePlan p; memset(&p, 0, sizeof(p));
		p.r0 = 0; p.rend = steps; p.need = need; p.flags = flags;
		p.active = 1000 + rng() % 5000; p.cells = p.active + rng() % 100;     // (few values: LPT ties)
		TileIn in; memset(&in, 0, sizeof(in));
		in.H = H; in.W = H + 50;
		plan.push_back(p); tin.push_back(in); n_rows += (uint64_t) H;
	}
	int n() const { return (int) plan.size(); }
};
struct Built { HostPlan hp; std::vector<int32_t> lists; ComputeSchedule s; };

static void build(const Batch &B, const RowDesc *rows, const ScheduleTuning &st, Built &o, int num_cus = 256) {
	host_plan(B.n(), B.plan.data(), B.tin.data(), rows, PlanTuning(), o.hp);
	o.lists.assign((size_t) 2 * B.n() + 16, -1);
	build_schedule(o.hp, B.plan.data(), B.tin.data(), B.n(), B.n_rows, num_cus, st, o.lists.data(), o.s);
}

static bool same_walk(const WalkPlan &a, const WalkPlan &b) { return a.n_long == b.n_long && a.long_lanes == b.long_lanes && a.bulk_lanes == b.bulk_lanes; }

// lists[at, at + count) is a walk segment of exactly the tiles `fill` (a stretch of a class's list), ordered as the rule orders a
// segment: H >> 5 never increases, and reads of one bucket keep the class's own order
static void check_segment(const Batch &B, const Built &o, size_t at, int count, const int32_t *fill, int n_fill, std::vector<int> &walked) {
	CHECK(count == n_fill);      // (a whole-tile class holds computed tiles only)
	std::vector<int> pos((size_t) B.n(), -1);
	for (int q = 0; q < n_fill; ++q) pos[(size_t) fill[q]] = q;
	for (int q = 0; q < count; ++q) {
		const int32_t t = o.lists[at + (size_t) q];
		if (t < 0 || t >= B.n() || pos[(size_t) t] < 0) { CHECK(!"a part's walk segment holds that part's fill tiles"); return; }
		walked[(size_t) t]++;
		if (q > 0) {
			const int32_t u = o.lists[at + (size_t) q - 1];
			const int ku = B.tin[(size_t) u].H >> 5, kt = B.tin[(size_t) t].H >> 5;
			if (!(ku > kt || (ku == kt && pos[(size_t) u] < pos[(size_t) t]))) { CHECK(!"backtrack order inside a part"); return; }
		}
	}
}

// the split a forced tail of N tiles must give launch L of the unsplit schedule
static int want_forced(const FillLaunch &L, const ScheduleTuning &st) {
	if (L.kind != CVX_LAUNCH_WHOLE || st.overlap_post || !st.bt_per_class) return 0;
	return (st.tail_tiles > 0 && st.tail_tiles < L.count - L.n_direct) ? st.tail_tiles : 0;
}

// every invariant of a schedule built with a forced tail (st.tail_tiles >= 0), against the same batch's schedule without (`d`, st0)
static void check_split(const Batch &B, const Built &o, const ScheduleTuning &st, const Built &d, const ScheduleTuning &st0) {
	const ComputeSchedule &s = o.s, &s0 = d.s;
	const int n = B.n();
	CHECK(s.launches.size() == s0.launches.size() && s.bt_begin == s0.bt_begin && s.n_listed == s0.n_listed && s.n_walk == s0.n_walk);
	if (s.launches.size() != s0.launches.size()) return;
	// the fill lists and their order are the unsplit schedule's; so are the flags of the direct-exact tiles
	CHECK(memcmp(o.lists.data(), d.lists.data(), s.bt_begin * sizeof(int32_t)) == 0);
	for (int i = 0; i < n; ++i) if (o.hp.tout[(size_t) i].pad != d.hp.tout[(size_t) i].pad) { CHECK(!"kPadRedo flags"); break; }
	std::vector<int> filled((size_t) n, 0), walked((size_t) n, 0);
	bool any = false;
	size_t bt_at = s.bt_begin;
	for (size_t i = 0; i < s.launches.size(); ++i) {
		const FillLaunch &L = s.launches[i], &L0 = s0.launches[i];
		CHECK(L.kind == L0.kind && L.m == L0.m && L.gang == L0.gang && L.wrap == L0.wrap && L.slot == L0.slot && L.list_off == L0.list_off &&
				L.n_direct == L0.n_direct && L.count == L0.count && L.pad_lds == L0.pad_lds && L.prio == L0.prio && L.stream == L0.stream);
		// one record per class, the unsplit launch's
		CHECK(memcmp(&L.info, &L0.info, sizeof(L.info)) == 0);
		CHECK(L.bt_off == bt_at && L.bt_off == L0.bt_off && L.bt_count == L0.bt_count);
		bt_at += (size_t) L.bt_count;
		// which launches split: whole tiles only, both parts non-empty, the direct-exact prefix wholly in the head
		CHECK(L.tail_count == want_forced(L0, st));
		if (L.kind != CVX_LAUNCH_WHOLE) CHECK(L.tail_count == 0 && L.bt_tail_count == 0);
		if (L.tail_count > 0) {
			any = true;
			CHECK(L.n_direct + L.tail_count < L.count && L.bt_tail_count == L.tail_count);
			const int n_head = L.count - L.tail_count;
			// the head = the front of the class's list, the tail = its end; each part's walk sub-segment holds that part's tiles
			check_segment(B, o, L.bt_off, L.bt_count - L.bt_tail_count, o.lists.data() + L.list_off, n_head, walked);
			check_segment(B, o, L.bt_off + (size_t) (L.bt_count - L.bt_tail_count), L.bt_tail_count, o.lists.data() + L.list_off + (size_t) n_head, L.tail_count, walked);
			for (int q = 0; q < L.count; ++q) filled[(size_t) o.lists[L.list_off + (size_t) q]]++;
			// every tile of the tail is at most as large as every tile of the head's two-phase part (the list is in LPT order behind the prefix)
			if (n_head > L.n_direct) CHECK(B.plan[(size_t) o.lists[L.list_off + (size_t) n_head - 1]].active >= B.plan[(size_t) o.lists[L.list_off + (size_t) n_head]].active);
			// each part is walked with the lanes its own count gives it
			const WalkPlan wh = walk_plan(n_head, s.n_walk, st.bt_group, B.n_rows / (uint64_t) n, o.lists.data() + L.bt_off, B.tin.data());
			const WalkPlan wt = walk_plan(L.tail_count, s.n_walk, st.bt_group, B.n_rows / (uint64_t) n, o.lists.data() + L.bt_off + (size_t) n_head, B.tin.data());
			CHECK(same_walk(L.walk, wh) && same_walk(L.walk_tail, wt));
		} else {
			CHECK(L.bt_tail_count == 0);
			// an unsplit launch of a split schedule: its segment is the unsplit schedule's
			CHECK(memcmp(o.lists.data() + L.bt_off, d.lists.data() + L0.bt_off, (size_t) L.bt_count * sizeof(int32_t)) == 0);
			for (int q = 0; q < L.bt_count; ++q) walked[(size_t) o.lists[L.bt_off + (size_t) q]]++;
			if (L.kind == CVX_LAUNCH_CHAINED) { for (int32_t t : *L.tiles) filled[(size_t) t]++; }
			else for (int q = 0; q < L.count; ++q) filled[(size_t) o.lists[L.list_off + (size_t) q]]++;
			if (s.per_class) {
				const WalkPlan w = walk_plan(L.bt_count, s.n_walk, st.bt_group, B.n_rows / (uint64_t) n, o.lists.data() + L.bt_off, B.tin.data());
				CHECK(same_walk(L.walk, w));
			}
		}
	}
	CHECK(bt_at == s.n_listed);
	for (int i = 0; i < n; ++i) {
		const int want = o.hp.trun[(size_t) i].skip ? 0 : 1;
		if (filled[(size_t) i] != want || walked[(size_t) i] != want) { CHECK(!"every computed tile once in a fill list and once in a walk segment"); break; }
	}
	// a schedule with a split launch walks per launch whatever its size; one without is the unsplit schedule
	CHECK(s.per_class == (s0.per_class || any));
	if (!any) {
		CHECK(memcmp(o.lists.data(), d.lists.data(), o.lists.size() * sizeof(int32_t)) == 0 && same_walk(s.walk, s0.walk));
		for (size_t i = 0; i < s.launches.size(); ++i) CHECK(same_walk(s.launches[i].walk, s0.launches[i].walk));
	}
	(void) st0;
}

// the batch under every tail size the issue names, for every whole-tile class it has
static void run_tail_sizes(const Batch &B, const RowDesc *rows, const ScheduleTuning &st0, int *splits = nullptr) {
	Built d;
	build(B, rows, st0, d);
	std::set<int> sizes = {0, 1, B.n() + 1, 2 * B.n() + 7};
	for (const FillLaunch &L : d.s.launches)
		if (L.kind == CVX_LAUNCH_WHOLE) { sizes.insert(std::max(0, L.count - L.n_direct - 1)); sizes.insert(L.count - L.n_direct); }
	for (const int N : sizes) {
		ScheduleTuning st = st0;
		st.tail_tiles = N;
		Built o;
		build(B, rows, st, o);
		check_split(B, o, st, d, st0);
		if (splits) for (const FillLaunch &L : o.s.launches) *splits += L.tail_count > 0;
	}
}

int main() {
	std::mt19937 rng(11);
	// the struct's default is "no split"
	CHECK(ScheduleTuning().tail_tiles == 0);
	// rows of a slope-1 band no ring holds (~1050 live rows): shared by every chained tile of the batches below
	const int cH = 3001, cw = 2100;
	std::vector<RowDesc> crow((size_t) cH);
	for (int y = 0; y < cH; ++y) { crow[(size_t) y].off = y - cw / 2; crow[(size_t) y].len = cw; }
	// a mixed batch of `count` tiles: four ring classes, int16-run tiles, irregular tiles, skipped tiles, `chained` wide tiles;
	// gangs: every 41st tile needs a ring of 384 slots (a gang of two waves where the plan builds gangs)
	auto mixed = [&](int count, int chained, bool gangs, Batch &B) {
		static const int needs[] = {40, 100, 150, 150, 150, 250};
		for (int i = 0; i < count; ++i) {
			uint32_t fl = 0;
			if (i % 97 == 5) fl |= kPlanEmpty;
			if (i % 89 == 7) fl |= kPlanTooLarge;
			if (i % 53 == 9) fl |= kPlanIrregular;
			if (i % 31 == 3) fl |= kPlanWrap16;
			const int H = (count >= kSmallBatchTiles && i % 211 == 0) ? 60000 + (int) (rng() % 30000) : 200 + (int) (rng() % 12000);
			if (i < chained) B.add(rng, 1054, cH, 2 * cH);
			else if (gangs && i % 41 == 11) B.add(rng, 300, H, 2 * H + 100);
			else B.add(rng, needs[i % 6], H, 2 * H + 100, fl);
		}
	};
	for (const int count : {600, 4200, 6300, 12400, 49300}) {
		for (int variant = 0; variant < 5; ++variant) {
			Batch B;
			mixed(count, 5, variant == 4, B);
			ScheduleTuning st;
			if (variant == 1) st.overlap_post = true;
			if (variant == 2) { st.bt_group = -1; st.wide_prio = 2; st.chain_prio = 0; }
			if (variant == 3) { st.bt_per_class = false; st.bt_group = 8; st.exact_steps = 0; }
			int splits = 0;
			run_tail_sizes(B, crow.data(), st, &splits);
			// one walk behind all fills (overlap_post, or the per-class walks switched off) is no place for a split
			CHECK((splits > 0) == (variant != 1 && variant != 3));
			if (variant == 4) {
				Built d;
				build(B, crow.data(), st, d);
				bool gang = false;
				for (const FillLaunch &L : d.s.launches) gang = gang || L.kind == CVX_LAUNCH_GANG;
				CHECK(gang && d.s.launches.front().kind == CVX_LAUNCH_CHAINED && d.s.launches.back().kind == CVX_LAUNCH_CATCH_ALL);
			}
		}
	}
	// one-class batches (M = 3) of 1, 2, 600 and 49 300 tiles; every hundredth tile of the larger ones long enough for the direct-exact prefix
	for (const int count : {1, 2, 600, 49300}) {
		Batch B;
		for (int i = 0; i < count; ++i) {
			const int H = 800 + (int) (rng() % 3000);
			B.add(rng, 150, H, (count >= 600 && i % 100 == 50) ? kExactDirectSteps + (int) (rng() % 5) : 2 * H + 100);
		}
		{
			Built d;
			build(B, nullptr, ScheduleTuning(), d);
			CHECK(d.s.launches.size() == 1 && d.s.launches[0].kind == CVX_LAUNCH_WHOLE && d.s.launches[0].n_direct == (count >= 600 ? count / 100 : 0) && !d.s.per_class);
		}
		int splits = 0;
		run_tail_sizes(B, nullptr, ScheduleTuning(), &splits);
		// tails of 1 and of count - n_direct - 1 split a class of three two-phase tiles or more (of two: these are the same size)
		CHECK(splits == (count >= 600 ? 2 : count == 2 ? 1 : 0));
		ScheduleTuning st;
		st.exact_steps = 0;
		run_tail_sizes(B, nullptr, st);
	}
	// the automatic rule: tail = tail_rounds x (CUs x 4 SIMDs x waves per SIMD of the class), for a class of at least kTailMinRounds such
	// rounds in a batch that walks at least kTailMinWalk tiles, with overlap_post off
	{
		const int slot = 2 * 2;      // HostPlan::cls index of M = 3 with float runs
		auto one_class = [&](int count, Batch &B) { for (int i = 0; i < count; ++i) { const int H = 800 + (int) (rng() % 3000); B.add(rng, 150, H, 2 * H + 100); } };
		auto auto_tail = [&](const Batch &B, int num_cus, int waves, float rounds, bool overlap, Built &o) {
			ScheduleTuning st;
			st.tail_tiles = kTailAuto; st.tail_rounds = rounds; st.tail_waves_per_simd[slot] = waves; st.overlap_post = overlap;
			build(B, nullptr, st, o, num_cus);
			CHECK(o.s.launches.size() == 1);
			return o.s.launches[0].tail_count;
		};
		const int resident = 256 * 4 * 7;
		Built o;
		{
			Batch B; one_class(kTailMinRounds * resident - 1, B);
			CHECK(auto_tail(B, 256, 7, 1.0f, false, o) == 0 && !o.s.per_class);      // one tile short of four rounds
		}
		{
			Batch B; one_class(kTailMinRounds * resident, B);
			CHECK(auto_tail(B, 256, 7, 1.0f, false, o) == resident && o.s.per_class && o.s.launches[0].bt_tail_count == resident);
			CHECK(auto_tail(B, 256, 7, 0.5f, false, o) == resident / 2);
			CHECK(auto_tail(B, 256, 7, 1.5f, false, o) == resident * 3 / 2);
			CHECK(auto_tail(B, 256, 7, 2.0f, false, o) == resident * 2);
			CHECK(auto_tail(B, 256, 7, 0.0f, false, o) == 0);                        // no tail, no split
			CHECK(auto_tail(B, 256, 7, 4.0f, false, o) == 0);                        // ... and no head
			CHECK(auto_tail(B, 256, 7, 1.0f, true, o) == 0);                         // overlap_post
			CHECK(auto_tail(B, 256, 0, 1.0f, false, o) == 0);                        // occupancy unknown
			CHECK(auto_tail(B, 256, 8, 1.0f, false, o) == 0);                        // eight waves per SIMD: not four rounds any more
			CHECK(auto_tail(B, 256, 6, 1.0f, false, o) == 256 * 4 * 6);
			CHECK(auto_tail(B, 128, 7, 1.0f, false, o) == 128 * 4 * 7);
		}
		// a class of many rounds on a small device in a batch whose walk is not issue-bound
		{
			Batch B; one_class(kTailMinWalk - 1, B);
			CHECK(auto_tail(B, 2, 7, 1.0f, false, o) == 0);
			Batch B2; one_class(kTailMinWalk, B2);
			CHECK(auto_tail(B2, 2, 7, 1.0f, false, o) == 2 * 4 * 7);
		}
		// the batch bench.py builds: one class of ~49 120 tiles and a class of a few dozen -- the large one splits, the small one never
		{
			Batch B;
			for (int i = 0; i < 49152; ++i) { const int H = 9000 + (int) (rng() % 2000); B.add(rng, i % 1536 == 7 ? 250 : 150, H, 2 * H + 100); }
			ScheduleTuning st;
			st.tail_tiles = kTailAuto; st.tail_waves_per_simd[slot] = 7; st.tail_waves_per_simd[3 * 2] = 5;
			build(B, nullptr, st, o);
			CHECK(o.s.launches.size() == 2 && o.s.launches[0].m == 4 && o.s.launches[0].tail_count == 0 && o.s.launches[1].m == 3 && o.s.launches[1].tail_count == resident);
			Built d;
			build(B, nullptr, ScheduleTuning(), d);
			st.tail_tiles = resident;
			check_split(B, o, st, d, ScheduleTuning());      // (the same schedule as a forced tail of that size gives)
		}
		// the launches an aligner makes on its own (50 - 4 000 tiles) and a mix of a few thousand tiles keep today's schedule
		for (const int count : {50, 4000, 6144}) {
			Batch B;
			mixed(count, 5, false, B);
			ScheduleTuning st;
			st.tail_tiles = kTailAuto;
			for (int &w : st.tail_waves_per_simd) w = 7;
			Built a, d;
			build(B, crow.data(), st, a);
			build(B, crow.data(), ScheduleTuning(), d);
			CHECK(a.lists == d.lists && a.s.per_class == d.s.per_class);
			for (const FillLaunch &L : a.s.launches) CHECK(L.tail_count == 0);
		}
	}
	printf(fails ? "tail_split_logic_test: %d FAILED\n" : "tail_split_logic_test: ok\n", fails);
	return fails ? 1 : 0;
}
