/*
 * cvx_inv_checks_dev.h -- what the runtime and inv_checks_kernel (cvx_inv_checks.hip) share: the kernel's arguments and its launch.
 */
#ifndef CVX_INV_CHECKS_DEV_H
#define CVX_INV_CHECKS_DEV_H

#include <hip/hip_runtime.h>

#include "cvx_inv_checks.h"
#include "cvx_nm_regions.h"
#include "cvx_types.h"

namespace cvx {

/* The regions lie dense and in tile order; tile t owns regions [off[t], off[t + 1]) and off[n_tiles] is their total -- the layout
 * of a job's offsets (JobRegions::queue: the scan's total right behind the n offsets) and of cvx_inv_checks' region_off.  The
 * kernel looks at min(off[n_tiles], cap) regions: a job's arena may hold fewer than the job has (the write is bounded), and the
 * launch covers the arena, since only the device knows the total when it is queued. */
struct InvCheckArgs {
	const uint8_t *bin;            /* the resident 4-bit genome */
	unsigned long long L;          /* GetConcatRefLen() */
	const uint8_t *seq;            /* the sequence arena the tiles' queries lie in */
	const TileIn *tin;             /* qry_off, H */
	const WindowDesc *win;         /* position: the tile's ref_position (interval->onRefStart) */
	const ResultRec *rec;          /* ref_position: Align::PositionOffset */
	const unsigned long long *off;
	const NmRegion *regions;
	InvCheck *checks;              /* parallel to regions */
	unsigned long long cap;
	int32_t n_tiles;
};

/* one wave per region, four per workgroup, over the first max_regions regions (those past min(off[n_tiles], cap) return at once) */
hipError_t launch_inv_checks(const InvCheckArgs &a, unsigned long long max_regions, hipStream_t st);

}  // namespace cvx

#endif
