/*
 * device_genome.h -- the genome Convex::DeviceWindows::SetGenome announced, resident once per logical device for the CS threads'
 * stages: StrippedSWHip::BatchScoreWindows scores against it, CandidateSearchHip::SearchAndScore searches and scores against it.
 * One upload per logical device, by whichever of them asks first; every scorer and the searcher's per-device state is a user,
 * and the device's last user frees it.  (ConvexAlignHip keeps its own copy beside its fills, as before.)
 */
#ifndef CVX_DEVICE_GENOME_H
#define CVX_DEVICE_GENOME_H

#include "cvx_align.h"

namespace Convex {

struct DeviceGenome {
	/* one user more of logical device `logical`'s genome (nothing is uploaded yet) */
	static void Retain(int logical);
	/* the genome on that device, uploaded by the first call through `h` -- any handle on the device's physical device.  Throws
	 * without an announced genome or when the upload fails.  Only between the caller's Retain and Release. */
	static cvx_genome Get(int logical, cvx_handle h);
	/* one user fewer; the last one frees the device's copy, through `h` (a handle of that device that is still alive) */
	static void Release(int logical, cvx_handle h);
	/* uploads to that logical device since the process began (tests: once per device, however many users) */
	static long Uploads(int logical);
};

}  // namespace Convex

#endif
