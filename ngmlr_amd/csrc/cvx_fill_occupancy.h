/*
 * cvx_fill_occupancy.h -- how many waves of a whole-tile class's two-phase fill a SIMD holds, as the runtime reports it for the
 * kernel the launcher would pick (cvx_fill_occupancy.hip).  The schedule sizes the tail of a split class by it (tail_split,
 * cvx_host_logic.h).
 */
#ifndef CVX_FILL_OCCUPANCY_H
#define CVX_FILL_OCCUPANCY_H

namespace cvx {

/* m, wrap, pen_table, twin: as launch_fill(m, 1, wrap, kModeTwoPhase, ...) reads them.  Resident waves per SIMD on the current
 * device, or -1 when the runtime cannot say (an m without a whole-tile kernel, a failed query). */
int fill_two_phase_waves_per_simd(int m, bool wrap, bool pen_table, bool twin);

}  // namespace cvx

#endif
