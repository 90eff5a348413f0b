/*
 * cvx_rt_err.h -- the error layer of libcvxalign.so's C ABI: the thread-local message behind cvx_last_error, and the guard
 * that keeps every C++ exception inside the library.  Internal and free of HIP, so that the host-only sources
 * (cvx_format.cpp, cvx_corridor.cpp, cvx_sam.cpp, cvx_genome_host.cpp) include it as well.  Definitions: cvx_runtime.cpp.
 */
#ifndef CVX_RT_ERR_H
#define CVX_RT_ERR_H

#include <new>
#include <string>

#include "cvx_align.h"

namespace cvx {
extern thread_local std::string g_err;
void set_err(const char *fmt, ...);
}

#define RC_TRY(expr) do { int rc_ = (expr); if (rc_ != CVX_OK) return rc_; } while (0)

/* no C++ exception may cross the C ABI (std::bad_alloc from the host-side vectors): every exported entry that returns a status
 * opens with ABI_GUARD_BEGIN and closes with ABI_GUARD_END, one that returns nothing closes with ABI_GUARD_END_VOID
 * (tests/test_abi_guard_cpu.py) */
#define ABI_GUARD_BEGIN try {
#define ABI_GUARD_END                                                              \
	} catch (const std::bad_alloc &) {                                             \
		cvx::set_err("host allocation failed");                                    \
		return CVX_ERR_OOM;                                                        \
	} catch (...) {                                                                \
		cvx::set_err("unexpected C++ exception");                                  \
		return CVX_ERR_HIP;                                                        \
	}
#define ABI_GUARD_END_VOID                                                         \
	} catch (...) {                                                                \
		cvx::set_err("unexpected C++ exception");                                  \
	}

#endif
