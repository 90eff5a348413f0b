/*
 * batching_scorer.h -- ngmlr's interval and inversion checks scored on the device without blocking a carrier.
 *
 * Two SingleScore call sites of the reference never reach NGM::CreateAlignment (the factory the variants rebind to
 * StrippedSWHip): AlignmentBuffer::scoreInterval (src/AlignmentBuffer.cpp:2515-2548, scorer overlapCheckAligner, one
 * StrippedSW per AlignmentBuffer, src/AlignmentBuffer.h:368) and checkForSV's inversion check (:1158-1235, a new
 * StrippedSW per check).  They score one pair at a time, on the CPU, while the read's context holds its carrier thread.
 *
 * BatchingScorer is the scoring counterpart of BatchingAligner: SingleScore queues (ref, qry, &score) and parks the
 * caller -- FiberApi::Park on a fiber (cvx_fiber.h), a condition variable on a plain thread; the caller's strings stay
 * valid while it is parked, so nothing is copied before the dispatcher packs them.  ONE dispatcher thread per logical
 * device cuts a launch when the device is idle and something is queued, or when maxBatch requests wait, keeps up to
 * two launches in flight (cvx_score_submit / cvx_score_wait: each pair goes to the kernel for its shape), and wakes the
 * callers of a finished launch with their scores.  A failed launch fails its own requests: SingleScore throws in the
 * caller's context.  The destructor scores what is still queued, then stops.
 *
 * The backend is an interface so that tests/cpp/batching_scorer_test.cpp can drive the queue, the parking and the
 * error path with a host function instead of a device.
 *
 * SharedScorer(site) is the per-site proxy the ngmlr_hip_checks variant constructs in place of `new StrippedSW()` at
 * the two sites (tools/build_ngmlr_hip.sh): creating and deleting one is an atomic increment, because the inversion
 * site does it for every check.  Proxies are dealt round-robin over the logical devices (service_device.h; two under
 * CVX_ALIAS_DEVICES=2 on one card), one BatchingScorer + one service handle per device, created on first use.  At exit
 * one stderr line per device:
 *   BatchingScorer: device 0: 1234 interval checks, 56 inversion checks, 78 launches, 17.5 pairs per launch, 3.2 ms of kernels
 * CVX_CHECK_SCORER=0 (read once) sends the proxies to the reference's own StrippedSW instead (inside the ngmlr tree only):
 * the A/B inside one binary.
 */
#ifndef BATCHING_SCORER_H
#define BATCHING_SCORER_H

#include <condition_variable>
#include <deque>
#include <mutex>
#include <thread>
#include <vector>

#include "ngmlr_abi.h"
#include "cvx_fiber.h"

namespace Convex {

/* what the dispatcher launches on: Submit starts a launch (0 = it failed), Wait finishes it (the scores in call order;
 * false = it failed) and releases it.  KernelMs: device time of the launch Wait has just finished (0 if unknown). */
class ScoreBackend {
public:
	virtual ~ScoreBackend() {}
	virtual void * Submit(int n, char const * const * refs, char const * const * qrys) = 0;
	virtual bool Wait(void * launch, float * scores) = 0;
	virtual double KernelMs() { return 0.0; }
};

class BatchingScorer {
public:
	enum Site { kOther = 0, kInterval = 1, kInversion = 2, kSites = 3 };
	/* backend is owned by the caller and outlives the scorer */
	explicit BatchingScorer(ScoreBackend * backend, int maxBatch = 4096, int maxInFlight = 2);
	~BatchingScorer();              /* scores what is queued, then joins the dispatcher */

	/* the score of one pair; parks the caller until its launch is back.  Throws (const char *) when the launch failed or
	 * the scorer is shutting down. */
	float Score(char const * ref, char const * qry, int site = kOther);

	struct Stats { long checks[kSites]; long launches, pairs, failedLaunches, parks, maxQueued; double kernelMs; };
	Stats GetStats();

private:
	struct Request {
		char const * ref;
		char const * qry;
		float score;
		bool done, failed;
		Fiber * fiber;                  /* woken with FiberApi::Wake; 0: a plain thread, sleeping on cv */
		std::condition_variable cv;
	};
	struct Launch { void * handle; std::vector<Request *> reqs; };
	ScoreBackend * backend;
	int maxBatch, maxFlight;
	std::mutex mtx;
	std::condition_variable cvDispatch;
	std::vector<Request *> queue;
	std::deque<Launch> inFlight;       /* dispatcher only */
	bool stop;
	Stats st;
	std::thread dispatcher;
	void dispatchLoop();
	void finish(std::vector<Request *> & reqs, float const * scores, bool ok);   /* hands out scores, wakes the callers */
};

/* IAlignment proxy of one check site (see above).  SingleScore / BatchScore forward to the device's BatchingScorer;
 * the alignment entries throw. */
class SharedScorer: public IAlignment {
public:
	enum { kIntervalCheck = BatchingScorer::kInterval, kInversionCheck = BatchingScorer::kInversion };
	explicit SharedScorer(int site);
	virtual ~SharedScorer();

	virtual int GetScoreBatchSize() const { return 1024; }
	virtual int GetAlignBatchSize() const { return 0; }
	virtual int BatchScore(int const mode, int const batchSize, char const * const * const refSeqList,
			char const * const * const qrySeqList, float * const results, void * extData);
	virtual int SingleScore(int const mode, int const corridor, char const * const refSeq,
			char const * const qrySeq, float & result, void * extData);
	virtual int BatchAlign(int const, int const, char const * const * const, char const * const * const,
			Align * const, void *) { throw "SharedScorer: score-only"; }
	virtual int SingleAlign(int const, int const, char const * const, char const * const, Align &, void *) {
		throw "SharedScorer: score-only";
	}
	virtual int SingleAlign(int const, CorridorLine *, int const, char const * const, char const * const, Align &,
			int const, int const, void *) { throw "SharedScorer: score-only"; }

	/* statistics of a logical device's scorer (zeros when it has none) */
	static BatchingScorer::Stats DeviceStats(int device);

private:
	int site;
	int device;
	IAlignment * cpu;      /* CVX_CHECK_SCORER=0: the reference's StrippedSW, created on the first call */
};

}  // namespace Convex

#endif
