/*
 * cvx_ladder_merge.h -- how cvx_wait strings the per-rung stage outputs of a ladder job (cvx_submit_ladder_ex on a handle with
 * CVX_CREATE_NM_REGIONS / _INV_CHECKS / _JOB_TEXT) into the one dense arena an ordinary job hands out, as plain host code free
 * of HIP calls, so that ladder_finish (cvx_rt_ladder.cpp) and the CPU suite (tests/cpp/ladder_merge_test.cpp) run one rule.
 *
 * Every rung's batch keeps its own offsets (an exclusive scan over ITS tiles, the total behind them) and its own arena -- regions
 * and their checks in records, the two strings of a tile in bytes.  Tile i of the job is reported by rung rung_of[i], where it
 * is entry at[i]; its items are that rung's [off[at[i]], off[at[i] + 1]).  The merged arena holds the items of every tile's
 * reporting rung in tile order: merged_off is the exclusive scan of their counts, and the copies are spans (source rung, source
 * item, destination item, count), neighbours that continue each other in source and destination joined into one.
 */
#ifndef CVX_LADDER_MERGE_H
#define CVX_LADDER_MERGE_H

#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace cvx {

struct LadderSpan {
	int32_t rung;          /* index of the source rung (0: rung 1) */
	uint64_t src, dst;     /* first item in the rung's arena, in the merged arena */
	uint64_t len;          /* items, never 0 */
};

/* rung_of[n], at[n]: the reporting rung of every job tile and its entry there; rung_off[r]: the offsets of rung r, rung_n[r] + 1
 * of them (the last one the rung's total).  -> merged_off[n + 1] and the copy spans; false (nothing usable written) when a tile
 * names a rung or an entry that does not exist, or a rung's offsets descend. */
inline bool ladder_merge_plan(const int32_t n, const int32_t *rung_of, const int32_t *at, const int32_t n_rungs,
		const uint64_t *const *rung_off, const int32_t *rung_n, uint64_t *merged_off, std::vector<LadderSpan> &spans) {
	spans.clear();
	uint64_t used = 0;
	merged_off[0] = 0;
	for (int32_t i = 0; i < n; ++i) {
		const int32_t r = rung_of[i], j = at[i];
		if (r < 0 || r >= n_rungs || j < 0 || j >= rung_n[r]) return false;
		const uint64_t b = rung_off[r][j], e = rung_off[r][j + 1];
		if (e < b) return false;
		const uint64_t len = e - b;
		if (len > 0) {
			if (!spans.empty() && spans.back().rung == r && spans.back().src + spans.back().len == b && spans.back().dst + spans.back().len == used)
				spans.back().len += len;
			else {
				LadderSpan s;
				s.rung = r; s.src = b; s.dst = used; s.len = len;
				spans.push_back(s);
			}
		}
		used += len;
		merged_off[i + 1] = used;
	}
	return true;
}

/* the per-tile records that travel beside the offsets (end states, text records): out[i] = rung_rec[rung_of[i]][at[i]], records
 * of `bytes` bytes; the plan above has checked the indices */
inline void ladder_merge_records(const int32_t n, const int32_t *rung_of, const int32_t *at, const void *const *rung_rec, const size_t bytes, void *out) {
	for (int32_t i = 0; i < n; ++i) {
		const unsigned char *src = static_cast<const unsigned char *>(rung_rec[rung_of[i]]) + (size_t) at[i] * bytes;
		unsigned char *dst = static_cast<unsigned char *>(out) + (size_t) i * bytes;
		for (size_t k = 0; k < bytes; ++k) dst[k] = src[k];
	}
}

}  // namespace cvx

#endif
