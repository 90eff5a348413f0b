/*
 * job_text_capacity_test.cpp -- the host logic of a CVX_CREATE_JOB_TEXT job (ngmlr_amd/csrc/cvx_job_text_logic.h) against a brute-force
 * restatement: the first capacity of the string arena, which tiles a write into an arena of `cap` bytes touches, and the
 * CVX_TUNE_JOB_TEXT_CAP knob.  No device, no library (tests/test_job_text_capacity_cpu.py).
 */
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "cvx_job_text_logic.h"

static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); ++g_fail; } } while (0)

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

int main() {
	/* ---- the first capacity: never below the measured need plus a quarter, per row, and 64 bytes per tile on top */
	CHECK(cvx::kJobTextBytesPerRow >= 1.181 * 1.25 && cvx::kJobTextBytesPerRow < 1.181 * 1.25 + 0.01);
	const uint64_t rows_of[] = {0, 1, 2, 63, 64, 65, 1000, 10000, 245760000ull, 1ull << 40};
	const uint64_t tiles_of[] = {0, 1, 2, 24576, 1u << 20};
	for (uint64_t rows : rows_of) for (uint64_t n : tiles_of) {
		const uint64_t cap = cvx::job_text_first_capacity(rows, n, 0);
		const long double need = (long double) cvx::kJobTextBytesPerRow * (long double) rows + 64.0L * (long double) n;
		CHECK((long double) cap >= need);              /* rounded up, never down */
		CHECK((long double) cap <= need + 2.0L + need * 1e-12L);
		CHECK(cap >= 2 * n);                           /* a job of invalid tiles (two NULs each) always fits */
		CHECK(cvx::job_text_first_capacity(rows, n, 256) == 256);      /* the knob replaces the rule */
		CHECK(cvx::job_text_first_capacity(rows, n, 1) == 1);
	}
	CHECK(cvx::job_text_first_capacity(100, 3, 0) >= cvx::job_text_first_capacity(99, 3, 0));

	/* ---- which tiles are written: a byte map of the arena says it the long way */
	int written = 0, dropped = 0, exact = 0;
	for (int round = 0; round < 400; ++round) {
		const int n = 1 + (int) (rnd() % 40);
		std::vector<unsigned long long> len((size_t) n), off((size_t) n);
		unsigned long long total = 0;
		for (int i = 0; i < n; ++i) { len[(size_t) i] = 2 + rnd() % 50; off[(size_t) i] = total; total += len[(size_t) i]; }
		/* capacities around every tile boundary, below the first tile and past the total */
		std::vector<unsigned long long> caps = {0, 1, 2, total - 1, total, total + 1, total + 1000};
		for (int i = 0; i < n; ++i) { caps.push_back(off[(size_t) i]); caps.push_back(off[(size_t) i] + 1); caps.push_back(off[(size_t) i] + len[(size_t) i] - 1); }
		for (unsigned long long cap : caps) {
			std::vector<unsigned char> arena((size_t) cap, 0);
			for (int i = 0; i < n; ++i) {
				/* the long way: every byte of the tile has to exist */
				bool fits = true;
				for (unsigned long long b = off[(size_t) i]; b < off[(size_t) i] + len[(size_t) i]; ++b) if (b >= cap) { fits = false; break; }
				CHECK(cvx::job_text_tile_fits(off[(size_t) i], len[(size_t) i], cap) == fits);
				if (cvx::job_text_tile_fits(off[(size_t) i], len[(size_t) i], cap)) {
					for (unsigned long long b = off[(size_t) i]; b < off[(size_t) i] + len[(size_t) i]; ++b) arena.at((size_t) b) += 1;      /* (at: throws past cap) */
					++written;
					exact += off[(size_t) i] + len[(size_t) i] == cap;
				} else ++dropped;
			}
			/* the written tiles are a prefix of the job, each byte written once; with cap >= total nothing is dropped */
			bool gap = false;
			for (int i = 0; i < n; ++i) {
				const bool f = cvx::job_text_tile_fits(off[(size_t) i], len[(size_t) i], cap);
				if (!f) gap = true;
				CHECK(!(f && gap));
				if (cap >= total) CHECK(f);
			}
			for (unsigned char c : arena) CHECK(c <= 1);
		}
	}
	CHECK(written > 1000 && dropped > 1000 && exact > 100);
	/* no wrap at the top of the range */
	CHECK(!cvx::job_text_tile_fits(~0ull - 4, 10, ~0ull));
	CHECK(cvx::job_text_tile_fits(~0ull - 10, 10, ~0ull));
	CHECK(!cvx::job_text_tile_fits(300, 0, 256));
	CHECK(cvx::job_text_tile_fits(256, 0, 256));

	/* ---- the knob */
	CHECK(cvx::job_text_cap_knob(nullptr) == 0);
	CHECK(cvx::job_text_cap_knob("") == 0);
	CHECK(cvx::job_text_cap_knob("0") == 0);
	CHECK(cvx::job_text_cap_knob("256") == 256);
	CHECK(cvx::job_text_cap_knob("0256") == 256);
	CHECK(cvx::job_text_cap_knob("4294967296") == 4294967296ull);
	CHECK(cvx::job_text_cap_knob("-5") == 0);
	CHECK(cvx::job_text_cap_knob("12k") == 0);
	CHECK(cvx::job_text_cap_knob(" 12") == 0);
	CHECK(cvx::job_text_cap_knob("1e3") == 0);
	if (g_fail) { printf("job_text_capacity_test: %d failures\n", g_fail); return 1; }
	printf("job_text_capacity_test: ok (%d tiles written, %d dropped, %d ending at the capacity)\n", written, dropped, exact);
	return 0;
}
