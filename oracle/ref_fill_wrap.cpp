/*
 * ref_fill_wrap.cpp -- exposes the raw forward fill of the REFERENCE's own
 * Convex::ConvexAlignFast: fwdFillMatrixSSESimple's curr_max, its best cell and every
 * direction code it wrote.  Test infrastructure only (see oracle_abi.h).
 *
 * Built by oracle/Makefile into oracle/_ref/libcvx_oracle_ref.so beside ref_wrap.cpp,
 * with the reference sources where they lie; nothing of theirs is copied here.
 *
 * The fill and the matrix pointer are private members of ConvexAlignFast.  This one
 * translation unit reads the class declaration with `private` spelled `public`: access
 * specifiers change neither the layout of a class without virtual bases nor the mangled
 * names of its members, so the object files built from the unmodified sources link as
 * they are.  The standard headers come first, untouched by the macro.
 */
#include <stdint.h>
#include <stdlib.h>
#include <algorithm>
#include <climits>
#include <cstring>

#define private public
#include "ConvexAlignFast.h"   /* the reference's src/ (-I$(REF), oracle/Makefile) */
#undef private

#include "oracle_abi.h"

extern "C" {

/* One prepare / fwdFillMatrixSSESimple / clean on handle h (an oracle_create handle of this library).
 * *score: the fill's return value (curr_max; -1 when no cell scored above it).  best[0] / best[1]:
 * best_ref_index / best_read_index (0 / 0 where the fill never set them: its FwdResults starts zeroed here).
 * dirs: the direction code of every cell inside the window, 0 <= x < strlen(ref), row by row in x order
 * (what the fill wrote; cells of a row beyond the window are never written and are left out).
 * dirs_cap: capacity of dirs.  Returns the number of codes written, -1 if the matrix was not allocated,
 * -2 if dirs is too small. */
int64_t oracle_ref_fill(void *h, const char *ref, const char *qry,
		const int32_t *row_offset, const int32_t *row_length, int32_t height,
		float *score, int32_t best[2], int8_t *dirs, int64_t dirs_cap) {
	Convex::ConvexAlignFast *aligner = static_cast<Convex::ConvexAlignFast *>(h);
	int const W = (int) strlen(ref);
	int const H = (int) strlen(qry);

	CorridorLine *lines = new CorridorLine[height > 0 ? height : 1];
	for (int i = 0; i < height; ++i) {
		lines[i].offset = row_offset[i];
		lines[i].length = row_length[i];
		lines[i].offsetInMatrix = 0;
	}

	int64_t n = -1;
	*score = -1.0f;
	best[0] = best[1] = 0;
	if (aligner->matrix->prepare(W, H, lines, height)) {
		Convex::ConvexAlignFast::FwdResults fwd;
		memset(&fwd, 0, sizeof(fwd));
		*score = aligner->fwdFillMatrixSSESimple(ref, qry, fwd, 0);
		best[0] = fwd.best_ref_index;
		best[1] = fwd.best_read_index;
		n = 0;
		for (int y = 0; y < H && y < height && n >= 0; ++y) {
			int const x0 = std::max(0, lines[y].offset);
			int const x1 = std::min(lines[y].offset + lines[y].length, W);
			for (int x = x0; x < x1; ++x) {
				if (n >= dirs_cap) { n = -2; break; }
				dirs[n++] = (int8_t) *aligner->matrix->getDirection(x, y);
			}
		}
	}
	aligner->matrix->clean();
	delete[] lines;
	return n;
}

}
