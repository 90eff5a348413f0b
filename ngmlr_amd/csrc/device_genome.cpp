/* device_genome.cpp -- see device_genome.h.  Host-only C++ over the C ABI. */
#include "device_genome.h"
#include "convex_align_hip.h"
#include "service_device.h"

#include <cstdio>
#include <mutex>

namespace Convex {

namespace {
struct PerDevice {
	std::mutex mtx;             /* users, and the upload: seconds for a genome of gigabytes, once per device -- Retain / Release of that device wait that long */
	cvx_genome genome = 0;      /* read without the mutex once it is there (acquire) */
	int users = 0;
	long uploads = 0;
};
PerDevice g_dev[kMaxLogicalDevices];
PerDevice & at(int logical) { return g_dev[logical >= 0 && logical < kMaxLogicalDevices ? logical : 0]; }
}

void DeviceGenome::Retain(int logical) {
	PerDevice & d = at(logical);
	std::lock_guard<std::mutex> g(d.mtx);
	d.users += 1;
}

cvx_genome DeviceGenome::Get(int logical, cvx_handle h) {
	PerDevice & d = at(logical);
	cvx_genome have = __atomic_load_n(&d.genome, __ATOMIC_ACQUIRE);
	if (have != 0) return have;
	std::lock_guard<std::mutex> g(d.mtx);      /* (read again under the lock: another user of the device may have been uploading it) */
	if (d.genome == 0) {
		void const * binRef = 0; unsigned long long nNibbles = 0; unsigned long long const * starts = 0; int nStarts = 0;
		if (!DeviceWindows::Genome(binRef, nNibbles, starts, nStarts)) throw "Convex::DeviceGenome: no genome (Convex::DeviceWindows::SetGenome)";
		cvx_genome up = 0;
		if (cvx_genome_upload(h, (uint8_t const *) binRef, nNibbles, (uint64_t const *) starts, nStarts, &up) != CVX_OK) {
			fprintf(stderr, "Convex::DeviceGenome: %s\n", cvx_last_error());
			throw 1;
		}
		d.uploads += 1;
		__atomic_store_n(&d.genome, up, __ATOMIC_RELEASE);
	}
	return d.genome;
}

void DeviceGenome::Release(int logical, cvx_handle h) {
	PerDevice & d = at(logical);
	std::lock_guard<std::mutex> g(d.mtx);
	if (--d.users > 0) return;
	d.users = 0;
	if (d.genome != 0) {
		cvx_genome_free(h, d.genome);
		__atomic_store_n(&d.genome, (cvx_genome) 0, __ATOMIC_RELEASE);
	}
}

long DeviceGenome::Uploads(int logical) {
	PerDevice & d = at(logical);
	std::lock_guard<std::mutex> g(d.mtx);
	return d.uploads;
}

}  // namespace Convex
