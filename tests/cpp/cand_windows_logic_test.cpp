/*
 * cand_windows_logic_test.cpp -- plan_candidate_windows_kernel (ngmlr_amd/csrc/cvx_score_cands.hip) compiled for the host
 * (tests/cpp/hip_host_stub) and run one thread at a time, every thread of every workgroup, against score_windows_plan
 * (cvx_score_windows.h) on the pairs the host would have built from the same lists: one (location - window_lead, buffer_len, read,
 * strand) per candidate of every read whose list is shorter than max_cmrs.  Built with -fsanitize=address,undefined by
 * tests/test_cand_windows_logic_cpu.py; every array is allocated to the element, so an access outside one is a report.
 * No device: what it cannot show is anything the compiler for gfx950 does differently.
 */
#include <algorithm>
#include <string>
#include <vector>

#include "../../ngmlr_amd/csrc/cvx_score_cands.hip"

using namespace cvx;

namespace {

uint32_t g_rs = 11;
uint32_t rnd() { g_rs = g_rs * 1664525u + 1013904223u; return g_rs >> 8; }

struct Call {
	uint64_t L = 0;
	int32_t buffer_len = 0, window_lead = 0, max_cmrs = 0;
	std::vector<int32_t> n_cand;                 /* per read; negative: the ladder gave up */
	std::vector<int32_t> read_len;               /* per read, characters */
	std::vector<SearchCandidate> cand;           /* dense, in read order */
};

int g_failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++g_failures < 20) { printf("%s: ", name); printf(__VA_ARGS__); printf("\n"); } } } while (0)

/* runs the kernel over the call and holds it against the host plan; returns the status counts */
void run(const char *name, const Call &c, int count[3]) {
	const int n = (int) c.n_cand.size();
	std::vector<uint64_t> begin((size_t) n + 1), offsets((size_t) n + 1), read_off((size_t) n);
	uint64_t need = 0, at = 4096;                /* (a block that does not begin at 0: the search's offsets are relative to its start) */
	uint64_t max_read_bytes = 1;
	for (int i = 0; i < n; ++i) {
		begin[(size_t) i] = need;
		if (c.n_cand[(size_t) i] > 0) need += (uint64_t) c.n_cand[(size_t) i];
		offsets[(size_t) i] = at;
		read_off[(size_t) i] = at - 4096;
		at += (uint64_t) c.read_len[(size_t) i] + 1;
		max_read_bytes = std::max<uint64_t>(max_read_bytes, (uint64_t) c.read_len[(size_t) i] + 1);
	}
	begin[(size_t) n] = need; offsets[(size_t) n] = at;
	CHECK(need == c.cand.size(), "the case has %zu candidates for lists of %llu", c.cand.size(), (unsigned long long) need);
	if (need != c.cand.size()) return;
	/* the pairs of the two-call path, and where each candidate's pair is among them */
	std::vector<cvx_score_window> pairs;
	std::vector<int64_t> pair_of((size_t) need, -1);
	std::vector<int> owner((size_t) need, -1);
	for (int i = 0; i < n; ++i)
		for (int k = 0; k < c.n_cand[(size_t) i]; ++k) {
			const uint64_t q = begin[(size_t) i] + (uint64_t) k;
			owner[(size_t) q] = i;
			if (c.n_cand[(size_t) i] >= c.max_cmrs) continue;      /* no AllocScores: nothing of this list reaches ScoreBuffer */
			pair_of[(size_t) q] = (int64_t) pairs.size();
			cvx_score_window w;
			w.position = c.cand[(size_t) q].location - (uint64_t) c.window_lead;
			w.buffer_len = c.buffer_len; w.read = i; w.reverse = c.cand[(size_t) q].reverse;
			pairs.push_back(w);
		}
	ScoreWinPlan pl;
	int64_t bad = 0;
	if (score_windows_plan(c.L, n, offsets.data(), (int32_t) pairs.size(), pairs.data(), false, pl, &bad) != CVX_OK) { CHECK(false, "score_windows_plan refused the pairs (%lld)", (long long) bad); return; }
	std::vector<size_t> slot_of(pairs.size());
	for (size_t s = 0; s < pl.order.size(); ++s) slot_of[(size_t) pl.order[s]] = s;

	const CandWinSlots slots = cand_windows_slots(c.buffer_len, max_read_bytes, need);
	/* allocated to the element (new[]: the sanitizer's red zones lie right behind), filled with a pattern no field should keep */
	ScoreWinDesc *desc = new ScoreWinDesc[(size_t) need];
	int32_t *status = new int32_t[(size_t) need];
	memset(desc, 0xA5, (size_t) need * sizeof(ScoreWinDesc));
	memset(status, 0xA5, (size_t) need * sizeof(int32_t));
	const SearchCandidate *cand = c.cand.data();
	for (unsigned b = 0; b < (unsigned) ((need + 255) / 256); ++b)
		for (unsigned t = 0; t < 256; ++t) {
			blockIdx.x = b; threadIdx.x = t;
			plan_candidate_windows_kernel(cand, begin.data(), c.n_cand.data(), read_off.data(), c.read_len.data(), n, need, c.L,
					c.buffer_len, c.window_lead, c.max_cmrs, slots, desc, status);
		}
	std::vector<std::pair<uint64_t, uint64_t> > spans;
	for (uint64_t q = 0; q < need; ++q) {
		const ScoreWinDesc &d = desc[q];
		const int i = owner[(size_t) q];
		const int64_t p = pair_of[(size_t) q];
		int want_status;
		int32_t want_plain = 0, want_chars = 0, want_len = 0;
		const uint64_t want_pos = c.cand[(size_t) q].location - (uint64_t) c.window_lead;
		if (p < 0) want_status = 2;
		else if (pl.cls[(size_t) p] == kScClasses) want_status = 1;
		else {
			want_status = 0;
			/* (buffer_len 2048 with the 'x' tail behind an odd position is 2 048 characters, 2 049 with the NUL: one more than score_class
			 * calls diagonal; the fused call still sends it to score_diag_kernel, whose row holds 2 048 + 64 codes) */
			CHECK(pl.cls[(size_t) p] == kScDiag || (c.buffer_len == 2048 && pl.desc[slot_of[(size_t) p]].ref_chars == 2048), "candidate %llu is of class %d: the case is not of the diagonal kernel's shape", (unsigned long long) q, pl.cls[(size_t) p]);
			const ScoreWinDesc &w = pl.desc[slot_of[(size_t) p]];
			want_plain = w.n_plain; want_chars = w.ref_chars; want_len = w.read_len;
			CHECK(d.read_off == w.read_off, "candidate %llu: read_off %llu, the plan has %llu", (unsigned long long) q, (unsigned long long) d.read_off, (unsigned long long) w.read_off);
			CHECK(w.position == want_pos && w.reverse == (c.cand[(size_t) q].reverse != 0), "candidate %llu: the plan's own pair", (unsigned long long) q);
		}
		if (want_status >= 0 && want_status <= 2) ++count[want_status];
		CHECK(status[q] == want_status, "candidate %llu (read %d): status %d, want %d", (unsigned long long) q, i, status[q], want_status);
		CHECK(d.position == want_pos, "candidate %llu: position %llu, want %llu", (unsigned long long) q, (unsigned long long) d.position, (unsigned long long) want_pos);
		CHECK(d.n_plain == want_plain && d.ref_chars == want_chars, "candidate %llu: n_plain %d ref_chars %d, want %d %d", (unsigned long long) q, d.n_plain, d.ref_chars, want_plain, want_chars);
		CHECK(d.read_len == want_len, "candidate %llu: read_len %d, want %d", (unsigned long long) q, d.read_len, want_len);
		CHECK(d.read_off == read_off[(size_t) i], "candidate %llu: read_off %llu is not read %d's", (unsigned long long) q, (unsigned long long) d.read_off, i);
		CHECK(d.reverse == (c.cand[(size_t) q].reverse != 0), "candidate %llu: reverse %d", (unsigned long long) q, d.reverse);
		CHECK(d.scratch_off == 0, "candidate %llu: scratch_off", (unsigned long long) q);
		CHECK((d.ref_off & 15ull) == 0 && (d.qry_off & 15ull) == 0, "candidate %llu: slots at %llu / %llu are not 16-byte aligned", (unsigned long long) q, (unsigned long long) d.ref_off, (unsigned long long) d.qry_off);
		/* the bytes the stage kernel writes for this slot: both strings and their NULs */
		spans.push_back(std::make_pair(d.ref_off, d.ref_off + (uint64_t) d.ref_chars + 1));
		spans.push_back(std::make_pair(d.qry_off, d.qry_off + (uint64_t) d.read_len + 1));
	}
	std::sort(spans.begin(), spans.end());
	for (size_t k = 0; k < spans.size(); ++k) {
		CHECK(spans[k].second <= slots.seq_bytes, "a string ends at %llu of %llu arena bytes", (unsigned long long) spans[k].second, (unsigned long long) slots.seq_bytes);
		if (k) CHECK(spans[k - 1].second <= spans[k].first, "two strings share bytes at %llu", (unsigned long long) spans[k].first);
	}
	delete[] desc;
	delete[] status;
}

void add(Call &c, int read, uint64_t location, int reverse) {
	(void) read;
	SearchCandidate s;
	s.location = location; s.score = (float) (rnd() % 100); s.reverse = reverse;
	c.cand.push_back(s);
}

/* lists of the given lengths with locations all over the genome, the corners of the window rule among them */
Call make(uint64_t L, int32_t buffer_len, int32_t window_lead, int32_t max_cmrs, const std::vector<int32_t> &lists) {
	Call c;
	c.L = L; c.buffer_len = buffer_len; c.window_lead = window_lead; c.max_cmrs = max_cmrs;
	const uint64_t len = (uint64_t) buffer_len - 2, lead = (uint64_t) window_lead;
	/* positions (before the lead is added back): the first nibbles, both parities; windows that end one before L, at L, one past
	 * it; the last position that decodes, the first two that do not */
	std::vector<uint64_t> corner;
	for (uint64_t p : {(uint64_t) 0, (uint64_t) 1, (uint64_t) 2, (uint64_t) 7}) corner.push_back(p + lead);
	if (L > len + 2) for (uint64_t p : {L - len - 2, L - len - 1, L - len, L - len + 1, L - len + 2}) corner.push_back(p + lead);
	for (uint64_t p : {L - 2, L - 1, L, L + 1}) corner.push_back(p + lead);
	/* locations inside the lead: the position wraps */
	for (uint64_t loc : {(uint64_t) 0, (uint64_t) 1, lead / 2, lead - 1}) if (loc < lead) corner.push_back(loc);
	size_t k = 0;
	for (size_t i = 0; i < lists.size(); ++i) {
		c.n_cand.push_back(lists[i]);
		c.read_len.push_back((int32_t) (i % 5 == 0 ? 1 + rnd() % 40 : i % 5 == 1 ? 511 : 200 + rnd() % 112));
		for (int j = 0; j < lists[i]; ++j) {
			const bool use_corner = k < 2 * corner.size() || rnd() % 4 == 0;
			const uint64_t loc = use_corner ? corner[k % corner.size()] : lead + rnd() % (L > 0 ? L : 1);
			add(c, (int) i, loc, (int) ((k / corner.size()) & 1) ^ (use_corner ? 0 : (int) (rnd() & 1)));
			++k;
		}
	}
	return c;
}

std::vector<int32_t> split(int total, int parts_hint) {      /* lists that sum to total, empty reads sprinkled in */
	std::vector<int32_t> v;
	int left = total;
	while (left > 0) {
		if (rnd() % 3 == 0) v.push_back(rnd() % 2 ? 0 : -1);
		const int take = std::min(left, 1 + (int) (rnd() % (unsigned) parts_hint));
		v.push_back(take);
		left -= take;
	}
	return v;
}

}  // namespace

int main() {
	int count[3] = {0, 0, 0};
	for (uint64_t L : {100000ull, 100001ull}) {
		for (int32_t bl : {308, 309}) {
			const int32_t lead = (bl - 256) >> 1;      /* refMaxLen = corridor + 256 + 2 around a 256-base sub-read, lead = corridor >> 1 */
			/* list lengths 0, 1, max_cmrs - 1, max_cmrs, max_cmrs + 1; reads without a list (0: nothing listed, -1: the ladder gave up)
			 * at the start, at the end and between long lists */
			run("lengths", make(L, bl, lead, 30, {0, -1, 29, 0, 1, 30, -1, 0, 0, 31, 29, 0, 30, 1, 0, -1}), count);
			run("max_cmrs 1", make(L, bl, lead, 1, {0, 1, 0, 2, 0}), count);      /* every list is dropped */
			for (int need : {1, 255, 256, 257}) {
				run("one list", make(L, bl, lead, 1000, {0, need, 0}), count);
				run("many lists", make(L, bl, lead, 1000, split(need, 9)), count);
				run("single reads", make(L, bl, lead, 1000, std::vector<int32_t>((size_t) need, 1)), count);
			}
		}
		/* a lead far larger than the first contig's spacer, windows longer than what is left of the genome, the largest shape */
		run("lead 1200", make(L, 1500, 1200, 3, {2, 0, 3, 2, 4, 1}), count);
		run("largest diagonal", make(L, 2047, 0, 1000, split(300, 40)), count);
		run("largest", make(L, 2048, 0, 1000, split(300, 40)), count);
		run("largest, odd lead", make(L, 2048, 21, 1000, split(300, 40)), count);
		run("smallest", make(L, 3, 1, 1000, split(300, 40)), count);
	}
	run("tiny genome", make(40, 308, 26, 1000, split(70, 5)), count);      /* every window runs past L */
	if (!count[0] || !count[1] || !count[2]) { printf("cand_windows_logic_test: status counts %d %d %d: a status was never produced\n", count[0], count[1], count[2]); return 1; }
	if (g_failures) { printf("cand_windows_logic_test: %d differences\n", g_failures); return 1; }
	printf("cand_windows_logic_test: ok (%d scored, %d without a window, %d of dropped lists)\n", count[0], count[1], count[2]);
	return 0;
}
