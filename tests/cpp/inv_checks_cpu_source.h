/*
 * inv_checks_cpu_source.h -- test-only source of check records for oracle/_ref/ngmlr_invchecks_cpu (tools/build_ngmlr_hip.sh): the
 * inversion-check binding inside ngmlr on a machine without a device.
 *
 * The CPU aligner behind the request / note exchange (regions_cpu_aligner.h) answers with a regions-only note: it knows neither
 * interval->onRefStart nor the genome.  The finder site (nm_regions_finder_binding.inc) does -- it has detectMisalignment's
 * arguments -- and, where this header is compiled in, fills in the record of every region it walks with cvx::inv_check_host: the
 * rule the device kernel is held to (tests/test_gpu_inv_checks.py), over the pipeline's real regions, the read part the aligner
 * aligned, and ngmlr's own 4-bit genome through the accessor the script adds to SequenceProvider.h.  Every record checkForSV
 * consumes in that binary came from the host rule; under CVX_INV_CHECKS_VERIFY=1 each is compared with the reference's own scoring.
 * Compiled only inside ngmlr's tree.
 */
#ifndef INV_CHECKS_CPU_SOURCE_H
#define INV_CHECKS_CPU_SOURCE_H

#include <string.h>

#include "cvx_inv_checks.h"
#include "nm_regions_note.h"
#include "SequenceProvider.h"

namespace Convex {

inline NmRegionsNote::Check inv_checks_cpu_source(NmRegionsNote::Region const & region, char const * const readPartSeq, unsigned long long const onRefStart, int const positionOffset) {
	cvx::InvCheck const c = cvx::inv_check_host((uint8_t const *) SequenceProvider.cvxBinRef(), (uint64_t) SequenceProvider.GetConcatRefLen(),
			(uint8_t const *) readPartSeq, (int32_t) strlen(readPartSeq), (uint64_t) onRefStart, (int32_t) positionOffset,
			region.refStart, region.refStop, region.readStart, region.readStop);
	NmRegionsNote::Check const out = { c.score_fwd, c.score_rev, c.status, c.window_chars };
	return out;
}

}  // namespace Convex

#define CVX_INV_CHECKS_CPU_SOURCE(region, readPartSeq, onRefStart, positionOffset) \
	Convex::inv_checks_cpu_source(region, readPartSeq, (unsigned long long) (onRefStart), (int) (positionOffset))

#endif
