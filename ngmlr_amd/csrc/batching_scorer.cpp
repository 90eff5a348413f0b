/* batching_scorer.cpp -- see batching_scorer.h */
#include "batching_scorer.h"
#include "service_device.h"
#include "cvx_align.h"

#include <atomic>
#include <cstdio>
#include <cstdlib>

#ifdef CVX_IN_NGMLR_TREE
#include "StrippedSW.h"
#endif

namespace Convex {

BatchingScorer::BatchingScorer(ScoreBackend * backend_, int maxBatch_, int maxInFlight_)
		: backend(backend_), maxBatch(maxBatch_ > 0 ? maxBatch_ : 1), maxFlight(maxInFlight_ > 0 ? maxInFlight_ : 1), stop(false), st() {
	dispatcher = std::thread(&BatchingScorer::dispatchLoop, this);
}

BatchingScorer::~BatchingScorer() {
	{
		std::lock_guard<std::mutex> lk(mtx);
		stop = true;
	}
	cvDispatch.notify_all();
	dispatcher.join();
}

float BatchingScorer::Score(char const * ref, char const * qry, int site) {
	Request r;
	r.ref = ref;
	r.qry = qry;
	r.score = 0.0f;
	r.done = r.failed = false;
	r.fiber = FiberApi::Current();
	{
		std::unique_lock<std::mutex> lk(mtx);
		if (stop) throw "BatchingScorer: shutting down";
		queue.push_back(&r);
		st.checks[site >= 0 && site < kSites ? site : kOther] += 1;
		if ((long) queue.size() > st.maxQueued) st.maxQueued = (long) queue.size();
		if (r.fiber) st.parks += 1;
		cvDispatch.notify_one();
		if (!r.fiber) r.cv.wait(lk, [&r] { return r.done; });
	}
	if (r.fiber) FiberApi::Park();      /* one Wake per request (finish), after which r is never touched by the dispatcher */
	if (r.failed) throw "BatchingScorer: scoring launch failed";
	return r.score;
}

BatchingScorer::Stats BatchingScorer::GetStats() {
	std::lock_guard<std::mutex> lk(mtx);
	return st;
}

void BatchingScorer::finish(std::vector<Request *> & reqs, float const * scores, bool ok) {
	std::vector<Fiber *> wake;
	{
		std::lock_guard<std::mutex> lk(mtx);
		for (size_t i = 0; i < reqs.size(); ++i) {
			Request * r = reqs[i];
			r->failed = !ok;
			if (ok) r->score = scores[i];
			if (r->fiber) wake.push_back(r->fiber);
			r->done = true;
			if (!r->fiber) r->cv.notify_one();      /* under the lock: the caller cannot leave before it is released */
		}
		if (!ok) st.failedLaunches += 1;      /* (launches / pairs count the launches that came back) */
	}
	for (Fiber * f : wake) FiberApi::Wake(f);
}

void BatchingScorer::dispatchLoop() {
	std::vector<char const *> refs, qrys;
	std::vector<float> scores;
	std::unique_lock<std::mutex> lk(mtx);
	for (;;) {
		cvDispatch.wait(lk, [this] { return stop || !inFlight.empty() || !queue.empty(); });
		/* cut: the device is idle and something waits, or maxBatch requests wait (up to maxFlight launches in flight) */
		if (!queue.empty() && (int) inFlight.size() < maxFlight && (inFlight.empty() || (int) queue.size() >= maxBatch)) {
			Launch l;
			const size_t take = std::min(queue.size(), (size_t) maxBatch);
			l.reqs.assign(queue.begin(), queue.begin() + take);
			queue.erase(queue.begin(), queue.begin() + take);
			lk.unlock();
			refs.resize(take); qrys.resize(take);
			for (size_t i = 0; i < take; ++i) { refs[i] = l.reqs[i]->ref; qrys[i] = l.reqs[i]->qry; }
			l.handle = backend->Submit((int) take, refs.data(), qrys.data());
			if (!l.handle) {
				finish(l.reqs, 0, false);
				lk.lock();
				continue;
			}
			lk.lock();
			inFlight.push_back(std::move(l));
			continue;
		}
		if (!inFlight.empty()) {
			Launch l = std::move(inFlight.front());
			inFlight.pop_front();
			lk.unlock();
			scores.resize(l.reqs.size());
			const bool ok = backend->Wait(l.handle, scores.data());
			const double ms = ok ? backend->KernelMs() : 0.0;
			{
				std::lock_guard<std::mutex> g(mtx);
				if (ok) {
					st.launches += 1;
					st.pairs += (long) l.reqs.size();
					st.kernelMs += ms;
				}
			}
			finish(l.reqs, scores.data(), ok);
			lk.lock();
			continue;
		}
		if (stop && queue.empty()) break;
	}
}

/* ------------------------------------------------------------------ the device backend and the per-site proxy */

namespace {

class HipScoreBackend: public ScoreBackend {
public:
	explicit HipScoreBackend(int physical) : h(0), lastMs(0.0) {
		cvx_params p = { 2.0f, -5.0f, -5.0f, -5.0f, -1.0f, 0.15f };      /* the scoring kernels have fixed weights; any valid set */
		if (cvx_create_ex(physical, &p, 0, CVX_CREATE_SERVICE, &h) != CVX_OK) {
			fprintf(stderr, "BatchingScorer: %s\n", cvx_last_error());
			throw "BatchingScorer: no usable MI355X";
		}
	}
	void * Submit(int n, char const * const * refs, char const * const * qrys) {
		cvx_score_job job = 0;
		if (cvx_score_submit(h, n, refs, qrys, &job) != CVX_OK) {
			fprintf(stderr, "BatchingScorer: cvx_score_submit: %s\n", cvx_last_error());
			return 0;
		}
		return job;
	}
	bool Wait(void * launch, float * scores) {
		if (cvx_score_wait((cvx_score_job) launch, scores) != CVX_OK) {
			fprintf(stderr, "BatchingScorer: cvx_score_wait: %s\n", cvx_last_error());
			return false;
		}
		float ms = 0.0f;
		lastMs = cvx_stage_kernel_ms(h, CVX_STAGE_SCORE, &ms) == CVX_OK ? ms : 0.0;
		return true;
	}
	double KernelMs() { return lastMs; }
private:
	cvx_handle h;       /* lives as long as the process: the dispatcher is its only user */
	double lastMs;
};

std::mutex g_devMtx;
BatchingScorer * g_scorer[kMaxLogicalDevices] = {0};
std::atomic<long> g_nextDevice(0);
int g_nLogical = -1;

int logical_devices() {
	std::lock_guard<std::mutex> g(g_devMtx);
	if (g_nLogical < 0) {
		int np = 0;
		DeviceLayout(g_nLogical, np);
	}
	return g_nLogical;
}

/* CVX_CHECK_SCORER (read once): 0 = the reference's StrippedSW at the check sites */
bool device_checks() {
	static int const on = getenv("CVX_CHECK_SCORER") ? atoi(getenv("CVX_CHECK_SCORER")) != 0 : 1;
	return on != 0;
}

void print_stats() {
	for (int d = 0; d < kMaxLogicalDevices; ++d) {
		BatchingScorer * s = g_scorer[d];
		if (!s) continue;
		BatchingScorer::Stats const t = s->GetStats();
		fprintf(stderr, "BatchingScorer: device %d: %ld interval checks, %ld inversion checks, %ld launches, %.1f pairs per launch, %.1f ms of kernels"
				"%s\n", d, t.checks[BatchingScorer::kInterval], t.checks[BatchingScorer::kInversion], t.launches,
				t.launches ? (double) t.pairs / (double) t.launches : 0.0, t.kernelMs, t.failedLaunches ? " (some launches failed)" : "");
	}
}

/* the device's scorer, created on first use (it and its handle live until the process ends: checks can come from any
 * context up to the last read, and the line above is printed at exit) */
BatchingScorer * scorer_of(int device) {
	std::lock_guard<std::mutex> g(g_devMtx);
	if (!g_scorer[device]) {
		static bool registered = false;
		ScoreBackend * b = new HipScoreBackend(PhysicalDeviceOf(device));
		g_scorer[device] = new BatchingScorer(b);
		if (!registered) { atexit(print_stats); registered = true; }
	}
	return g_scorer[device];
}

}  // namespace

SharedScorer::SharedScorer(int site_) : site(site_), device(0), cpu(0) {
	const int n = logical_devices();
	device = n > 1 ? (int) (g_nextDevice.fetch_add(1, std::memory_order_relaxed) % n) : 0;
}

SharedScorer::~SharedScorer() {
	delete cpu;
}

int SharedScorer::SingleScore(int const mode, int const corridor, char const * const refSeq, char const * const qrySeq, float & result, void * extData) {
	if (!device_checks()) {
#ifdef CVX_IN_NGMLR_TREE
		if (!cpu) cpu = new StrippedSW();
		return cpu->SingleScore(mode, corridor, refSeq, qrySeq, result, extData);
#else
		(void) mode; (void) corridor; (void) extData;
		throw "SharedScorer: CVX_CHECK_SCORER=0 needs the reference's StrippedSW (ngmlr tree only)";
#endif
	}
	result = scorer_of(device)->Score(refSeq, qrySeq, site);
	return 1;
}

int SharedScorer::BatchScore(int const mode, int const batchSize, char const * const * const refSeqList,
		char const * const * const qrySeqList, float * const results, void * extData) {
	for (int i = 0; i < batchSize; ++i) SingleScore(mode, 0, refSeqList[i], qrySeqList[i], results[i], extData);
	return batchSize;
}

BatchingScorer::Stats SharedScorer::DeviceStats(int device) {
	BatchingScorer * s = 0;
	{
		std::lock_guard<std::mutex> g(g_devMtx);
		if (device >= 0 && device < kMaxLogicalDevices) s = g_scorer[device];
	}
	if (s) return s->GetStats();
	BatchingScorer::Stats z = BatchingScorer::Stats();
	return z;
}

}  // namespace Convex
