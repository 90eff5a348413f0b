/*
 * search_plan_test.cpp -- the host half of the candidate search (ngmlr_amd/csrc/cvx_search_plan.h) on the CPU: every rule at the
 * smallest cases on each side of its edge, against values written out by hand.  No device and no library: plain g++ over
 * tests/cpp/hip_host_stub, under -fsanitize=address,undefined (tests/test_search_plan_cpu.py).
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "cvx_search_plan.h"

using namespace cvx;

#define CHECK(cond)                                                                  \
	do {                                                                             \
		if (!(cond)) {                                                               \
			fprintf(stderr, "search_plan_test: %s:%d: %s\n", __FILE__, __LINE__, #cond); \
			exit(1);                                                                 \
		}                                                                            \
	} while (0)

template <typename T, size_t N>
static bool same(const std::vector<T> &got, const T (&want)[N]) {
	if (got.size() != N) return false;
	for (size_t i = 0; i < N; ++i) if (got[i] != want[i]) return false;
	return true;
}

static const SearchTuning kDefault = search_tuning(nullptr, nullptr, nullptr, nullptr, nullptr);

static void test_tuning() {
	CHECK(kDefault.use_wave && !kDefault.lane_serial && kDefault.classify_min == 2048 && kDefault.forced_log2 == 0 && kDefault.slot8 == -1 && !kDefault.trace);
	const SearchTuning lane = search_tuning("0", "0", nullptr, "0", "");
	CHECK(!lane.use_wave && lane.lane_serial && lane.classify_min == 0 && lane.slot8 == 0 && lane.trace);
	const SearchTuning hbm = search_tuning("2", nullptr, nullptr, "1", nullptr);
	CHECK(!hbm.use_wave && !hbm.lane_serial && hbm.slot8 == 1);
	CHECK(search_tuning(nullptr, nullptr, "8", nullptr, nullptr).forced_log2 == 9);       /* clamped to 9..12 */
	CHECK(search_tuning(nullptr, nullptr, "9", nullptr, nullptr).forced_log2 == 9);
	CHECK(search_tuning(nullptr, nullptr, "12", nullptr, nullptr).forced_log2 == 12);
	CHECK(search_tuning(nullptr, nullptr, "13", nullptr, nullptr).forced_log2 == 12);
	CHECK(search_tuning(nullptr, nullptr, "0", nullptr, nullptr).forced_log2 == 9);       /* set at all: forced */
}

static void test_classify() {
	/* k = 4: n_index = 4^4 + 2 = 258, a big table from 3 * 256 = 768 locations */
	CHECK(!search_classify(kDefault, 2047, 767, 258));
	CHECK(search_classify(kDefault, 2048, 767, 258));
	CHECK(search_classify(kDefault, 1, 768, 258));
	CHECK(!search_classify(kDefault, 1, 767, 258));
	const SearchTuning forced = search_tuning(nullptr, nullptr, "11", nullptr, nullptr);
	CHECK(!search_classify(forced, 5000, 768, 258));
	CHECK(!search_classify(search_tuning("2", nullptr, nullptr, nullptr, nullptr), 5000, 768, 258));
	CHECK(!search_classify(search_tuning("0", nullptr, nullptr, nullptr, nullptr), 5000, 768, 258));
	const SearchTuning sorted = search_tuning(nullptr, "0", nullptr, nullptr, nullptr);
	CHECK(search_classify(sorted, 1, 0, 258));
}

static void test_map_sizes() {
	const unsigned long long votes[] = {0, 1, 384, 385, 768, 769, 1536, 1537, 5000};
	const int want[] = {9, 9, 9, 10, 10, 11, 11, 12, 12};
	for (int i = 0; i < 9; ++i) CHECK(search_wave_log2(votes[i]) == want[i]);
	CHECK(search_wave_entries(9) == 384 && search_wave_entries(10) == 768 && search_wave_entries(11) == 1536 && search_wave_entries(12) == 3072);
	{   /* classified: two slots per vote where that is fewer than two per bin */
		const int32_t len[] = {256, 256, 256, 256};
		const unsigned long long v[] = {0, 384, 385, 5000};
		std::vector<uint8_t> map(4, 77);
		std::vector<uint64_t> src(4, 77);
		const uint64_t fixed = search_assign_maps(kDefault, true, 4, len, v, map.data(), src.data());
		const uint8_t want_map[] = {9, 9, 10, 12};
		const uint64_t want_src[] = {0, 0, 768, 1538};
		CHECK(same(map, want_map) && same(src, want_src) && fixed == 7682);
	}
	{   /* not classified: the default map, 2 * 1 536 slots per read; the votes are not looked at */
		const int32_t len[] = {10, 0, 300};
		std::vector<uint8_t> map(3, 77);
		std::vector<uint64_t> src(3, 77);
		const uint64_t fixed = search_assign_maps(kDefault, false, 3, len, nullptr, map.data(), src.data());
		const uint8_t want_map[] = {11, 11, 11};
		const uint64_t want_src[] = {0, 3072, 6144};
		CHECK(same(map, want_map) && same(src, want_src) && fixed == 9216);
	}
	{   /* a forced size: two per bin of that size, no min against the votes (a forced call is never classified) */
		const SearchTuning forced = search_tuning(nullptr, nullptr, "9", nullptr, nullptr);
		const int32_t len[] = {256, 256};
		std::vector<uint8_t> map(2, 77);
		std::vector<uint64_t> src(2, 77);
		const uint64_t fixed = search_assign_maps(forced, false, 2, len, nullptr, map.data(), src.data());
		const uint8_t want_map[] = {9, 9};
		const uint64_t want_src[] = {0, 768};
		CHECK(same(map, want_map) && same(src, want_src) && fixed == 1536);
		const SearchTuning forced12 = search_tuning(nullptr, nullptr, "12", nullptr, nullptr);
		CHECK(search_assign_maps(forced12, false, 2, len, nullptr, map.data(), src.data()) == 12288 && src[1] == 6144 && map[0] == 12);
	}
	{   /* 4 095 characters and the NUL fill the kernel's sequence buffer; 4 096 do not fit: no map, no slots, the running offset */
		const int32_t len[] = {4095, 4096, 4095};
		std::vector<uint8_t> map(3, 77);
		std::vector<uint64_t> src(3, 77);
		const uint64_t fixed = search_assign_maps(kDefault, false, 3, len, nullptr, map.data(), src.data());
		const uint8_t want_map[] = {11, 0, 11};
		const uint64_t want_src[] = {0, 3072, 3072};
		CHECK(same(map, want_map) && same(src, want_src) && fixed == 6144);
	}
	for (const char *mode : {"0", "2"}) {   /* the lane and HBM-only forms: no map at all */
		const SearchTuning t = search_tuning(mode, nullptr, nullptr, nullptr, nullptr);
		const int32_t len[] = {256, 10};
		std::vector<uint8_t> map(2, 77);
		std::vector<uint64_t> src(2, 77);
		const uint8_t want_map[] = {0, 0};
		const uint64_t want_src[] = {0, 0};
		CHECK(search_assign_maps(t, false, 2, len, nullptr, map.data(), src.data()) == 0 && same(map, want_map) && same(src, want_src));
	}
}

static std::vector<int> ladder(int first_bits) {
	std::vector<int> v;
	for (int attempt = 0; search_ladder_bits(first_bits, attempt) <= kSearchLadderMaxBits; ++attempt) v.push_back(search_ladder_bits(first_bits, attempt));
	return v;
}

static void test_ladder() {
	const int from16[] = {16, 18, 19, 20};
	CHECK(same(ladder(0), from16) && same(ladder(16), from16));
	const int from8[] = {8, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20};
	CHECK(same(ladder(8), from8) && ladder(8).size() == 12);
	const int from18[] = {18, 20};
	CHECK(same(ladder(18), from18));
	const int from19[] = {19};
	const int from20[] = {20};
	CHECK(same(ladder(19), from19) && same(ladder(20), from20));
	CHECK(kSearchLadderMaxBits == 20);
	CHECK(search_ladder_factor(0) == 0.333f && search_ladder_factor(1) == 0.777f && search_ladder_factor(11) == 0.777f);
}

static bool slot8_of(const SearchTuning &t, int bits, int l, int longest) {
	const std::vector<int32_t> ww = {0};
	const uint8_t map[] = {(uint8_t) l};
	const int32_t len[] = {longest};
	int32_t work[1];
	SearchWaveLaunch out[kSearchWaveSizes];
	CHECK(search_wave_launches(t, bits, ww, map, len, work, out) == 1 && out[0].log2 == l && out[0].longest == longest);
	return out[0].slot8;
}

static void test_wave_launches() {
	{   /* reads 1, 2, 4, 5, 7 of a call are on the LDS form, with maps 11, 9, 11, 12, 9 */
		const std::vector<int32_t> ww = {1, 2, 4, 5, 7};
		const uint8_t map[] = {0, 11, 9, 0, 11, 12, 0, 9};
		const int32_t len[] = {5000, 100, 63, 5000, 300, 64, 5000, 20};
		std::vector<int32_t> work(8, -7);
		SearchWaveLaunch out[kSearchWaveSizes];
		CHECK(search_wave_launches(kDefault, 16, ww, map, len, work.data(), out) == 3);
		const int32_t want_work[] = {2, 7, 1, 4, 5, -7, -7, -7};
		CHECK(same(work, want_work));
		CHECK(out[0].log2 == 9 && out[0].first == 0 && out[0].count == 2 && out[0].longest == 63 && out[0].seq_cap == 128 && out[0].slot8);
		CHECK(out[1].log2 == 11 && out[1].first == 2 && out[1].count == 2 && out[1].longest == 300 && out[1].seq_cap == 384 && !out[1].slot8);
		CHECK(out[2].log2 == 12 && out[2].first == 4 && out[2].count == 1 && out[2].longest == 64 && out[2].seq_cap == 192 && !out[2].slot8);
	}
	{   /* nothing on the LDS form: no launch, the work list untouched */
		const std::vector<int32_t> none;
		int32_t work[1] = {-7};
		SearchWaveLaunch out[kSearchWaveSizes];
		CHECK(search_wave_launches(kDefault, 16, none, nullptr, nullptr, work, out) == 0 && work[0] == -7);
	}
	{   /* seq_cap: the longest read + 65, up to a multiple of 64 */
		const std::vector<int32_t> ww = {0};
		const uint8_t map[] = {10};
		int32_t work[1];
		SearchWaveLaunch out[kSearchWaveSizes];
		const int32_t l0[] = {0}, l63[] = {63}, l64[] = {64};
		CHECK(search_wave_launches(kDefault, 16, ww, map, l0, work, out) == 1 && out[0].seq_cap == 128);
		CHECK(search_wave_launches(kDefault, 16, ww, map, l63, work, out) == 1 && out[0].seq_cap == 128);
		CHECK(search_wave_launches(kDefault, 16, ww, map, l64, work, out) == 1 && out[0].seq_cap == 192);
	}
	const SearchTuning off = search_tuning(nullptr, nullptr, nullptr, "0", nullptr), on = search_tuning(nullptr, nullptr, nullptr, "1", nullptr);
	/* unset: table of 2^16 or below, not the largest map, sub-reads */
	CHECK(slot8_of(kDefault, 16, 11, 268));
	CHECK(!slot8_of(kDefault, 17, 11, 268));
	CHECK(!slot8_of(kDefault, 16, 12, 268));
	CHECK(!slot8_of(kDefault, 16, 11, 269));
	CHECK(slot8_of(kDefault, 8, 9, 0));
	/* = 1: the same without the length */
	CHECK(slot8_of(on, 16, 11, 268));
	CHECK(!slot8_of(on, 17, 11, 268));
	CHECK(!slot8_of(on, 16, 12, 268));
	CHECK(slot8_of(on, 16, 11, 269));
	CHECK(slot8_of(on, 16, 11, 4095));
	/* = 0: never */
	CHECK(!slot8_of(off, 16, 11, 268));
	CHECK(!slot8_of(off, 17, 11, 268));
	CHECK(!slot8_of(off, 16, 12, 268));
	CHECK(!slot8_of(off, 16, 11, 269));
	CHECK(!slot8_of(off, 8, 9, 0));
}

static void test_budgets() {
	CHECK(search_hbm_tables(20000, 16) == 8192);      /* as many as can be resident */
	CHECK(search_hbm_tables(20000, 17) == 4096);      /* as 8 GB hold: 2^33 / (2^17 * 16) */
	CHECK(search_hbm_tables(20000, 20) == 512);
	CHECK(search_hbm_tables(20000, 8) == 8192);
	CHECK(search_hbm_tables(1, 16) == 1 && search_hbm_tables(1, 20) == 1);
	CHECK(search_hbm_tables(513, 20) == 512 && search_hbm_tables(511, 20) == 511);
	CHECK(search_hbm_table_words(8192, 16) == (size_t) 8192 * 65536 * 2);
	CHECK(search_hbm_table_words(1, 8) == 512);
	CHECK(search_hbm_table_words(512, 20) == (size_t) 1 << 30);      /* 8 GB of 8-byte words */
	CHECK(search_lane_chunk(600, 20) == 512);
	CHECK(search_lane_chunk(600, 16) == 600);         /* (no cap at the resident waves: a lane per read) */
	CHECK(search_lane_chunk(20000, 16) == 8192 && search_lane_chunk(1, 20) == 1);
	CHECK(search_lane_keys(512, 20) == (size_t) 512 << 20 && search_lane_scores(512, 20) == (size_t) 1024 << 20);
	CHECK(search_lane_keys(3, 8) == 768 && search_lane_scores(3, 8) == 1536);
}

static void test_regions() {
	const unsigned long long votes[] = {10, 20, 30, 40, 50};
	std::vector<uint8_t> has(5, 0);
	std::vector<uint64_t> off(5, 99);
	uint64_t total = 0;
	const std::vector<int32_t> first = {3, 1}, second = {1, 0, 3}, third = {0, 1};
	CHECK(search_give_regions(first, votes, has.data(), off.data(), &total));
	const uint64_t want1[] = {99, 40, 99, 0, 99};      /* in hand-out order, not read order */
	const uint8_t has1[] = {0, 1, 0, 1, 0};
	CHECK(same(off, want1) && same(has, has1) && total == 60);
	CHECK(search_give_regions(second, votes, has.data(), off.data(), &total));      /* reads 1 and 3 keep theirs */
	const uint64_t want2[] = {60, 40, 99, 0, 99};
	const uint8_t has2[] = {1, 1, 0, 1, 0};
	CHECK(same(off, want2) && same(has, has2) && total == 70);
	CHECK(!search_give_regions(third, votes, has.data(), off.data(), &total));      /* nothing new: nothing grew */
	CHECK(same(off, want2) && same(has, has2) && total == 70);
	CHECK(!search_give_regions(std::vector<int32_t>(), votes, has.data(), off.data(), &total) && total == 70);
	CHECK(search_hbm_src_off(7682, 0) == 7682 && search_hbm_src_off(7682, 40) == 7762);
	CHECK(search_cand_needed(7682, 70) == 7682 + 140 + 64);
	CHECK(search_cand_grown(7682, 70) == 7682 + 140 + 35 + 64);
	CHECK(search_cand_needed(0, 0) == 64 && search_cand_grown(0, 1) == 66 && search_cand_grown(0, 3) == 71);
}

static void test_dense_offsets() {
	const int32_t ncand[] = {-1, 0, 3, kSearchNeedsHbm, 2};
	std::vector<uint64_t> begin(6, 99), cand_begin(5, 99);
	std::vector<int32_t> n_candidates(5, 99);
	CHECK(search_dense_offsets(5, ncand, begin.data(), cand_begin.data(), n_candidates.data()) == 5);
	const uint64_t want_begin[] = {0, 0, 0, 3, 3, 5}, want_cb[] = {0, 0, 0, 3, 3};
	const int32_t want_n[] = {-1, 0, 3, -2, 2};
	CHECK(kSearchNeedsHbm == -2);
	CHECK(same(begin, want_begin) && same(cand_begin, want_cb) && same(n_candidates, want_n));
	uint64_t b0[1] = {99};
	CHECK(search_dense_offsets(0, nullptr, b0, nullptr, nullptr) == 0 && b0[0] == 0);
}

/* [p, p + bytes) of every array, in order: each aligned to its element, none reaching into the next, the last inside the block */
struct Span { const void *p; size_t bytes, align; };
static void check_spans(const uint8_t *block, size_t block_bytes, const Span *s, int n) {
	const uint8_t *at = block;
	for (int i = 0; i < n; ++i) {
		const uint8_t *p = static_cast<const uint8_t *>(s[i].p);
		CHECK(p >= at && (size_t) (p - block) % s[i].align == 0);
		at = p + s[i].bytes;
	}
	CHECK(at <= block + block_bytes);
}

static void test_layout() {
	CHECK(search_meta_bytes(1) == 32 + 8 + 64 && search_out_bytes(1) == 20 + 64);
	CHECK(search_meta_bytes(7) == 224 + 8 + 64 && search_out_bytes(7) == 140 + 64);
	for (size_t n : {(size_t) 1, (size_t) 7}) {
		/* exactly the stated sizes, from the allocator: the sanitizer sees a write past either end */
		std::vector<uint64_t> meta_block(search_meta_bytes(n) / 8), out_block((search_out_bytes(n) + 7) / 8);
		CHECK(search_meta_bytes(n) % 8 == 0);
		const SearchMeta m = search_meta_view(meta_block.data(), n);
		const Span ms[] = {{m.off, 8 * n, 8}, {m.list_off, 8 * n, 8}, {m.begin, 8 * (n + 1), 8}, {m.len, 4 * n, 4}, {m.work, 4 * n, 4}};
		check_spans(reinterpret_cast<const uint8_t *>(meta_block.data()), search_meta_bytes(n), ms, 5);
		CHECK(static_cast<void *>(m.off) == meta_block.data());
		const SearchOut o = search_out_view(out_block.data(), n);
		const Span os[] = {{o.events, 8 * n, 8}, {o.ncand, 4 * n, 4}, {o.miss, 4 * n, 4}, {o.maxhit, 4 * n, 4}};
		check_spans(reinterpret_cast<const uint8_t *>(out_block.data()), search_out_bytes(n), os, 4);
		CHECK(static_cast<void *>(o.events) == out_block.data());
		for (size_t i = 0; i < n; ++i) {
			m.off[i] = 1; m.list_off[i] = 2; m.begin[i] = 3; m.len[i] = 4; m.work[i] = 5;
			o.events[i] = 6; o.ncand[i] = 7; o.miss[i] = 8; o.maxhit[i] = 9.0f;
		}
		m.begin[n] = 3;
		for (size_t i = 0; i < n; ++i)
			CHECK(m.off[i] == 1 && m.list_off[i] == 2 && m.begin[i] == 3 && m.len[i] == 4 && m.work[i] == 5 && o.events[i] == 6 && o.ncand[i] == 7 && o.miss[i] == 8 && o.maxhit[i] == 9.0f);
		CHECK(m.begin[n] == 3);
	}
}

static void test_reads() {
	/* "ACG", "T", "" and "GG" behind two bytes that are not the call's: a single NUL is a read of length 0 */
	const uint8_t arena[] = {'x', 'x', 'A', 'C', 'G', 0, 'T', 0, 0, 'G', 'G', 0};
	{
		const uint64_t offsets[] = {2, 6, 8, 9, 12};
		uint64_t bytes = 99;
		CHECK(search_arena_reads_check(4, arena, offsets, &bytes) == -1 && bytes == 10);
		std::vector<uint64_t> off(4, 99);
		std::vector<int32_t> len(4, 99);
		search_arena_reads_layout(4, offsets, off.data(), len.data());
		const uint64_t want_off[] = {0, 4, 6, 7};
		const int32_t want_len[] = {3, 1, 0, 2};
		CHECK(same(off, want_off) && same(len, want_len));
	}
	uint64_t bytes = 99;
	const uint64_t no_nul[] = {2, 6, 7, 9};          /* read 1 ends on the 'T' */
	CHECK(search_arena_reads_check(3, arena, no_nul, &bytes) == 1 && bytes == 99);
	const uint64_t empty[] = {2, 6, 8, 8, 9};        /* read 2 has not even its NUL */
	CHECK(search_arena_reads_check(4, arena, empty, &bytes) == 2);
	const uint64_t descending[] = {2, 6, 8, 6, 9};   /* read 2 again */
	CHECK(search_arena_reads_check(4, arena, descending, &bytes) == 2);
	const uint64_t first_bad[] = {6, 6, 8};
	CHECK(search_arena_reads_check(2, arena, first_bad, &bytes) == 0);
	/* 2 GB: the length is kept in an int32 (the check must not read the arena there: nothing lies behind the offsets) */
	const uint64_t huge[] = {0, 0x80000000ull}, largest[] = {6, 8};
	CHECK(search_arena_reads_check(1, arena, huge, &bytes) == 0);
	CHECK(search_arena_reads_check(1, arena, largest, &bytes) == -1 && bytes == 2);
	CHECK(search_arena_reads_check(0, arena, largest, &bytes) == -1 && bytes == 0);

	const char *seqs[] = {"ACG", "", "TT"};
	const int32_t lens[] = {3, 0, 2};
	CHECK(search_string_reads_check(3, seqs, lens, &bytes) == -1 && bytes == 8);
	std::vector<uint64_t> off(3, 99);
	std::vector<int32_t> len(3, 99);
	search_string_reads_layout(3, lens, off.data(), len.data());
	const uint64_t want_off[] = {0, 4, 5};
	const int32_t want_len[] = {3, 0, 2};
	CHECK(same(off, want_off) && same(len, want_len));
	const char *with_null[] = {"ACG", nullptr, "TT"};
	bytes = 99;
	CHECK(search_string_reads_check(3, with_null, lens, &bytes) == 1 && bytes == 99);
	const int32_t negative[] = {3, 0, -1};
	CHECK(search_string_reads_check(3, seqs, negative, &bytes) == 2);
}

int main() {
	test_tuning();
	test_classify();
	test_map_sizes();
	test_ladder();
	test_wave_launches();
	test_budgets();
	test_regions();
	test_dense_offsets();
	test_layout();
	test_reads();
	printf("search_plan_test: ok\n");
	return 0;
}
