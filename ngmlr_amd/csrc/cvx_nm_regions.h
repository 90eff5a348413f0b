/*
 * cvx_nm_regions.h -- the low-identity regions of the per-position NM profile, found on the device (nm_regions_kernel in
 * cvx_text.hip): what the peak finder at the top of detectMisalignment (reference src/AlignmentBuffer.cpp:1316-1395) reduces
 * nmPerPosition to.  Kept apart from cvx_types.h / cvx_launch.h, whose bytes name the fill / search kernel families
 * (Makefile FILL_ID / SEARCH_ID).
 */
#ifndef CVX_NM_REGIONS_H
#define CVX_NM_REGIONS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cvx_launch.h"

namespace cvx {

/* a row of the profile is marked iff 0 < (32 - nm) / 32.0f < 0.75 (isInversion, :1143-1148): for an integer nm, 9 <= nm <= 31 */
static const int kNmMarkLo = 9, kNmMarkHi = 31;
/* maxDistance (:1290): up to 20 unmarked rows between two marks merge, the 21st closes the region */
static const int kNmMaxDistance = 20;
/* regions of a tile that the first pass keeps in the tile's own slot (256 bytes): a 10 kb PacBio tile has four or five */
static const int kNmStage = 16;

struct NmRegion {         /* same layout as cvx_nm_region (include/cvx_align.h) */
	int32_t ref_start, ref_stop, read_start, read_stop;
};
struct NmOpen {           /* same layout as cvx_nm_open */
	int32_t open, distance;
	NmRegion r;
};

/* pass 1 over the tiles [first, first + count): closed regions per tile -> len[count], their exclusive prefix sum -> off[count]
 * with the total behind it (*total), the state the scan ends in -> open[count], a tile's first kNmStage regions ->
 * stage[count * kNmStage] */
hipError_t launch_nm_regions_count(const TextArgs &a, int first, int count, unsigned long long *len, unsigned long long *off,
		unsigned long long *total, NmOpen *open, NmRegion *stage, hipStream_t st);
/* pass 2: tile first + i puts its len[i] regions at regions + off[i] (from the stage; a tile with more walks again) */
hipError_t launch_nm_regions_write(const TextArgs &a, int first, int count, const unsigned long long *len, const unsigned long long *off,
		const NmRegion *stage, NmRegion *regions, hipStream_t st);

/* pass 2 of a job that finds its regions with its results (CVX_CREATE_NM_REGIONS), over all `count` tiles of the job: the same
 * write into an arena of `cap` regions sized before the total was known -- what lies past cap is dropped, total[0] (the scan's)
 * says how many there are, total[1] receives cap */
hipError_t launch_nm_regions_bounded(const TextArgs &a, int count, const unsigned long long *len, const unsigned long long *off,
		unsigned long long *total, const NmRegion *stage, NmRegion *regions, unsigned long long cap, hipStream_t st);

}  // namespace cvx

#endif
