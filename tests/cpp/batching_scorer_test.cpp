/*
 * batching_scorer_test.cpp -- Convex::BatchingScorer (ngmlr_amd/csrc/batching_scorer.{h,cpp}) with a host backend instead of
 * a device: the score of a pair is a deterministic function of its two strings, so every caller can check that it got its
 * own.  Covers the queue, parking on fibers (FiberApi::Park / Wake) and on plain threads (condition variable), shutdown
 * with requests still queued, and launches that fail (their callers, and only they, see an exception).
 *
 *   batching_scorer_test fibers <carriers> <fibers> <items>
 *   batching_scorer_test threads <threads> <items per thread>
 *   batching_scorer_test shutdown <threads>
 *   batching_scorer_test fail <threads> <items per thread>
 * Prints one line "ok: ..." and exits 0, or says what went wrong and exits 1.  A lost wake-up is a hang: the caller runs
 * this under a timeout.
 */
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "batching_scorer.h"
#include "cvx_fiber.h"

using namespace Convex;

namespace {

float expected(char const * a, char const * b) {
	unsigned h = 2166136261u;
	for (char const * p = a; *p; ++p) h = (h ^ (unsigned char) *p) * 16777619u;
	h = (h ^ 0xffu) * 16777619u;
	for (char const * p = b; *p; ++p) h = (h ^ (unsigned char) *p) * 16777619u;
	return (float) (h % 100003u);
}

/* the pair of item i: strings of varying length that are built on the caller's stack */
void make_pair(long i, std::string & ref, std::string & qry) {
	static char const acgt[] = "ACGT";
	ref.assign((size_t) (5 + i % 37), 'A');
	qry.assign((size_t) (1 + (i * 7) % 23), 'C');
	unsigned long x = (unsigned long) i * 2654435761ul + 1;
	for (char & c : ref) { x = x * 6364136223846793005ul + 1442695040888963407ul; c = acgt[(x >> 33) & 3]; }
	for (char & c : qry) { x = x * 6364136223846793005ul + 1442695040888963407ul; c = acgt[(x >> 33) & 3]; }
}

class HostBackend: public ScoreBackend {
public:
	std::atomic<long> submits{0}, waits{0}, largest{0}, failedReqs{0};
	int failEvery = 0;            /* every failEvery-th launch fails (alternately in Submit and in Wait) */
	int waitUs = 200;             /* how long a launch "runs" */
	struct L { std::vector<float> s; bool fail; };
	void * Submit(int n, char const * const * refs, char const * const * qrys) {
		const long k = ++submits;
		if (n > largest) largest = n;
		const bool fail = failEvery > 0 && k % failEvery == 0;
		if (fail) failedReqs += n;
		if (fail && (k / failEvery) % 2) return 0;
		L * l = new L();
		l->fail = fail;
		for (int i = 0; i < n; ++i) l->s.push_back(expected(refs[i], qrys[i]));
		return l;
	}
	bool Wait(void * launch, float * scores) {
		L * l = (L *) launch;
		std::this_thread::sleep_for(std::chrono::microseconds(waitUs));
		++waits;
		const bool ok = !l->fail;
		if (ok) for (size_t i = 0; i < l->s.size(); ++i) scores[i] = l->s[i];
		delete l;
		return ok;
	}
	double KernelMs() { return 0.01; }
};

int fail(char const * what) {
	printf("FAIL: %s\n", what);
	return 1;
}

struct FiberCtx {
	BatchingScorer * scorer;
	std::atomic<long> wrong{0}, thrown{0}, done{0};
};

void fiber_run(void * user, void ** slot, void * item) {
	FiberCtx * c = (FiberCtx *) user;
	if (!*slot) *slot = c;
	const long i = (long) (size_t) item;
	std::string ref, qry;
	make_pair(i, ref, qry);
	try {
		const float got = c->scorer->Score(ref.c_str(), qry.c_str(), (int) (i % 3));
		if (got != expected(ref.c_str(), qry.c_str())) ++c->wrong;
	} catch (...) {
		++c->thrown;
	}
	++c->done;
}
void fiber_destroy(void *, void *) {}

int run_fibers(int carriers, int fibers, long items) {
	HostBackend be;
	BatchingScorer * s = new BatchingScorer(&be, 512);
	FiberCtx ctx;
	ctx.scorer = s;
	FiberPool::Callbacks cb = { &ctx, fiber_run, fiber_destroy, 0, 0 };
	FiberPool pool(carriers, fibers, 64 * 1024, 4 * fibers, cb);
	for (long i = 0; i < items; ++i) pool.Submit((void *) (size_t) i);
	pool.CloseFeed();
	pool.DrainAndStop();
	const BatchingScorer::Stats st = s->GetStats();
	const FiberPool::Stats fs = pool.GetStats();
	delete s;
	if (ctx.wrong || ctx.thrown) { printf("wrong %ld thrown %ld\n", ctx.wrong.load(), ctx.thrown.load()); return fail("a fiber got another caller's score"); }
	if (ctx.done != items) return fail("not every item finished");
	if (st.pairs != items || st.checks[0] + st.checks[1] + st.checks[2] != items) return fail("pairs / checks do not add up");
	if (st.parks != items) return fail("not one park per request on fibers");
	if (fs.parks != items) { printf("pool parks %ld, items %ld\n", fs.parks, items); return fail("park and wake do not pair up"); }
	if (st.launches != be.waits || st.launches != be.submits) return fail("launch count");
	printf("ok: fibers %d carriers, %d fibers, %ld items, %ld launches, %.1f pairs per launch (largest %ld), max queued %ld\n",
			carriers, fibers, items, st.launches, (double) st.pairs / st.launches, be.largest.load(), st.maxQueued);
	return 0;
}

int run_threads(int threads, long per, int failEvery) {
	HostBackend be;
	be.failEvery = failEvery;
	BatchingScorer * s = new BatchingScorer(&be, 256);
	std::atomic<long> wrong(0), thrown(0), ok(0);
	std::vector<std::thread> th;
	for (int t = 0; t < threads; ++t)
		th.emplace_back([&, t] {
			for (long k = 0; k < per; ++k) {
				std::string ref, qry;
				make_pair(t * per + k, ref, qry);
				try {
					if (s->Score(ref.c_str(), qry.c_str(), BatchingScorer::kInterval) != expected(ref.c_str(), qry.c_str())) ++wrong;
					else ++ok;
				} catch (char const *) {
					++thrown;
				}
			}
		});
	for (auto & x : th) x.join();
	const BatchingScorer::Stats st = s->GetStats();
	delete s;
	if (wrong) return fail("a thread got another caller's score");
	if (ok + thrown != threads * per) return fail("requests lost");
	if (st.parks != 0) return fail("plain threads counted as fiber parks");
	if (failEvery == 0 && (thrown || st.failedLaunches)) return fail("exceptions without a failing backend");
	if (failEvery > 0) {
		if (!st.failedLaunches || !thrown) return fail("no launch failed although the backend fails some");
		/* a failed launch fails exactly its own requests: the callers that threw are those of the failed launches */
		if (thrown != be.failedReqs || st.pairs != ok) return fail("failed requests do not match the failed launches");
	}
	printf("ok: threads %d x %ld, %ld launches (%ld failed), %ld scores, %ld exceptions, %.1f pairs per launch\n", threads, per,
			st.launches + st.failedLaunches, st.failedLaunches, ok.load(), thrown.load(), st.launches ? (double) st.pairs / st.launches : 0.0);
	return 0;
}

int run_shutdown(int threads) {
	HostBackend be;
	be.waitUs = 20000;               /* launches take long: requests pile up behind the first */
	BatchingScorer * s = new BatchingScorer(&be, 8);
	std::atomic<long> wrong(0), ok(0), thrown(0);
	std::vector<std::thread> th;
	for (int t = 0; t < threads; ++t)
		th.emplace_back([&, t] {
			std::string ref, qry;
			make_pair(t, ref, qry);
			try {
				if (s->Score(ref.c_str(), qry.c_str(), BatchingScorer::kInversion) != expected(ref.c_str(), qry.c_str())) ++wrong;
				else ++ok;
			} catch (...) { ++thrown; }
		});
	/* every request has been queued (most still waiting: the first launch is "running"), then the scorer goes */
	for (;;) {
		BatchingScorer::Stats st = s->GetStats();
		if (st.checks[BatchingScorer::kInversion] == threads) break;
		std::this_thread::sleep_for(std::chrono::microseconds(100));
	}
	const long launchesBefore = s->GetStats().launches;
	delete s;                          /* must score what is queued, then stop */
	for (auto & x : th) x.join();
	if (wrong || thrown) return fail("a queued request was dropped or got a wrong score at shutdown");
	if (ok != threads) return fail("not every request was served");
	if (launchesBefore >= be.submits) return fail("nothing was pending at shutdown (the test did not test it)");
	printf("ok: shutdown with %ld of %d requests' launches still to come; all served\n", be.submits.load() - launchesBefore, threads);
	return 0;
}

}  // namespace

int main(int argc, char ** argv) {
	if (argc >= 5 && !strcmp(argv[1], "fibers")) return run_fibers(atoi(argv[2]), atoi(argv[3]), atol(argv[4]));
	if (argc >= 4 && !strcmp(argv[1], "threads")) return run_threads(atoi(argv[2]), atol(argv[3]), 0);
	if (argc >= 3 && !strcmp(argv[1], "shutdown")) return run_shutdown(atoi(argv[2]));
	if (argc >= 4 && !strcmp(argv[1], "fail")) return run_threads(atoi(argv[2]), atol(argv[3]), 5);
	fprintf(stderr, "usage: batching_scorer_test fibers C F N | threads T N | shutdown T | fail T N\n");
	return 2;
}
