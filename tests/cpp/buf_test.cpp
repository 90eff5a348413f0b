/*
 * buf_test.cpp -- the runtime's owning buffer (ngmlr_amd/csrc/cvx_buf.h) over a counting fake memory: the capacities its growth
 * rule reaches against the rule as DevBuf::ensure and PinBuf::ensure stated it before they became one template, the one
 * drain-and-retry, what a failed growth leaves behind, and who frees what.  Host only: plain g++, its own main
 * (tests/test_buf_cpu.py).
 */
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <set>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "cvx_buf.h"

namespace cvx {
thread_local std::string g_err;
void set_err(const char *fmt, ...) {
	char buf[512];
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(buf, sizeof(buf), fmt, ap);
	va_end(ap);
	g_err = buf;
}
}  // namespace cvx

static int g_failures = 0;
#define CHECK(cond, ...)                                                           \
	do {                                                                           \
		if (!(cond)) {                                                             \
			if (++g_failures <= 20) { printf("FAIL %s:%d: %s -- ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
		}                                                                          \
	} while (0)

/* hands out addresses nobody dereferences, and keeps the books: what lives, what is parked, every call */
template <size_t Slack>
struct FakeMem {
	static constexpr size_t kSlack = Slack;
	static constexpr const char *kName = "fakeAlloc";
	static inline std::set<void *> live, parked;
	static inline std::vector<size_t> asked_bytes;      /* of every alloc call, failed ones included */
	static inline long allocs = 0, frees = 0, parks = 0, drains = 0, bad_frees = 0;
	static inline long fail_from = 0, fail_count = 0;   /* alloc calls [fail_from, fail_from + fail_count) fail (counted from 1 after reset) */
	static inline uintptr_t serial = 0;

	static void reset() {
		live.clear(); parked.clear(); asked_bytes.clear();
		allocs = frees = parks = drains = bad_frees = 0;
		fail_from = fail_count = 0;
	}
	static const char *alloc(void **p, size_t bytes) {
		asked_bytes.push_back(bytes);
		const long call = (long) asked_bytes.size();
		if (call >= fail_from && call < fail_from + fail_count) return "out of fake memory";
		*p = reinterpret_cast<void *>(++serial << 12);
		live.insert(*p);
		++allocs;
		return nullptr;
	}
	static void free(void *p) {
		if (live.erase(p) != 1) ++bad_frees;
		++frees;
	}
	static void park(void *p) {
		if (live.erase(p) != 1) ++bad_frees;
		parked.insert(p);
		++parks;
	}
	static void drain() {
		++drains;
		frees += (long) parked.size();
		parked.clear();
	}
	static bool balanced() { return bad_frees == 0 && allocs == frees + (long) parked.size() + (long) live.size(); }
};

using DevLike = FakeMem<64>;       /* the device buffers' slack, in elements */
using PinLike = FakeMem<4096>;     /* the page-locked buffers', in bytes */

struct E12 { uint32_t a, b, c; };

/* ---- the rule as the two ensure() of cvx_rt.h stated it, copied out */

/* DevBuf<T>::ensure: cap and n in elements of sz bytes, *hwm in bytes */
static size_t dev_rule(size_t sz, size_t old, size_t n, const size_t *hwm) {
	const size_t asked = n + n / 8 + 64;
	size_t want = asked;
	if (want < 2 * old) want = 2 * old;
	if (hwm && want * sz < *hwm && *hwm / 16 <= asked * sz) want = (*hwm + sz - 1) / sz;
	return want;
}
/* PinBuf::ensure: everything in bytes */
static size_t pin_rule(size_t, size_t old, size_t bytes, const size_t *hwm) {
	const size_t asked = bytes + bytes / 8 + 4096;
	size_t want = asked;
	if (want < 2 * old) want = 2 * old;
	if (hwm && want < *hwm && *hwm / 16 <= asked) want = *hwm;
	return want;
}

/* (a) every old capacity x request x high-water mark: the capacity reached, the bytes asked of the allocator, the mark afterwards */
template <typename T, typename M>
static long sweep_capacities(size_t (*rule)(size_t, size_t, size_t, const size_t *), const char *name) {
	constexpr size_t sz = cvx::BufElem<T>::kBytes;
	long cases = 0;
	const size_t olds[] = {0, 1, 100, 1000000};
	for (size_t old : olds) {
		const size_t ns[] = {0, 1, old / 2, old ? old - 1 : 0, old, old + 1, old + old / 8 + 1, old + old / 2, 2 * old, 2 * old + 1, 3 * old + 7, 20 * old + 5, 1000, 123457};
		for (size_t n : ns) {
			const size_t asked = n + n / 8 + M::kSlack;
			const size_t plain = rule(sz, old, n, nullptr);          /* `want` before the mark has its say */
			/* no mark; marks below want; above want and within 16 x asked (whole elements and not, and the last that is within); beyond 16 x asked */
			const size_t marks[] = {0, 1, plain * sz / 2, plain * sz - 1, plain * sz, plain * sz + 1, plain * sz + sz + 5, 3 * plain * sz + 1,
			                        16 * asked * sz, 16 * asked * sz + 15, 16 * asked * sz + 16, 40 * asked * sz + 3};
			for (size_t mi = 0; mi < sizeof(marks) / sizeof(marks[0]); ++mi) {
				M::reset();
				size_t mark = marks[mi];
				const bool with_mark = mi > 0;
				const size_t mark_before = mark;
				{
					cvx::Buf<T, M> b;
					void *old_block = nullptr;
					if (old) {                                       /* a buffer that holds `old` elements */
						M::alloc(&old_block, old * sz);
						b.p = static_cast<T *>(old_block);
						b.cap = old;
					}
					if (with_mark) b.hwm = &mark;
					const size_t calls_before = M::asked_bytes.size();
					const int rc = b.ensure(n);
					++cases;
					CHECK(rc == CVX_OK, "%s old %zu n %zu mark %zu", name, old, n, mark_before);
					if (n <= old) {
						CHECK(b.cap == old && b.p == old_block && M::asked_bytes.size() == calls_before && M::parks == 0, "%s old %zu n %zu: a request that fits changed the buffer", name, old, n);
						CHECK(mark == mark_before, "%s old %zu n %zu: mark moved", name, old, n);
					} else {
						const size_t want = rule(sz, old, n, with_mark ? &mark_before : nullptr);
						CHECK(b.cap == want, "%s old %zu n %zu mark %zu: cap %zu, the rule gives %zu", name, old, n, mark_before, b.cap, want);
						CHECK(M::asked_bytes.size() == calls_before + 1 && M::asked_bytes.back() == want * sz, "%s old %zu n %zu mark %zu: allocator calls", name, old, n, mark_before);
						CHECK(b.p != nullptr && M::live.count(b.p) == 1, "%s old %zu n %zu: block", name, old, n);
						CHECK(M::parks == (old ? 1 : 0) && M::parked.count(old_block) == (old ? 1u : 0u), "%s old %zu n %zu: the old block is parked, nothing else", name, old, n);
						CHECK(M::drains == 0 && M::frees == 0, "%s old %zu n %zu: a growth that fits frees nothing", name, old, n);
						if (with_mark) CHECK(mark == (want * sz > mark_before ? want * sz : mark_before), "%s old %zu n %zu mark %zu: mark afterwards %zu", name, old, n, mark_before, mark);
					}
				}
				CHECK(M::live.empty() && M::balanced(), "%s old %zu n %zu: books after scope exit", name, old, n);
			}
		}
	}
	return cases;
}

/* (b) the generous size does not fit: one drain, one retry at what was asked for */
static void test_retry_after_drain() {
	using M = DevLike;
	M::reset();
	{
		cvx::Buf<uint32_t, M> b;
		CHECK(b.ensure(36) == CVX_OK && b.cap == 36 + 4 + 64, "first growth");       /* 104 */
		void *first = b.p;
		M::fail_from = 2; M::fail_count = 1;
		const int rc = b.ensure(105);      /* asked 105 + 13 + 64 = 182 < 2 x 104 */
		CHECK(rc == CVX_OK, "retry: rc %d (%s)", rc, cvx::g_err.c_str());
		CHECK(M::asked_bytes.size() == 3 && M::asked_bytes[1] == 208 * 4 && M::asked_bytes[2] == 182 * 4, "retry: the sizes tried");
		CHECK(M::drains == 1, "retry: %ld drains", M::drains);
		CHECK(b.cap == 182 && b.p && b.p != first, "retry: cap %zu", b.cap);
		CHECK(M::parked.empty() && M::frees == 1, "retry: the drain gave the outgrown block back");
	}
	CHECK(M::balanced() && M::live.empty() && M::frees == 2, "retry: books");
	/* ... and when what was asked for does not fit either */
	M::reset();
	{
		cvx::Buf<uint32_t, M> b;
		CHECK(b.ensure(36) == CVX_OK, "first growth");
		M::fail_from = 2; M::fail_count = 2;
		const int rc = b.ensure(105);
		CHECK(rc == CVX_ERR_OOM && b.p == nullptr && b.cap == 0, "retry fails: rc %d cap %zu", rc, b.cap);
		CHECK(M::drains == 1 && M::asked_bytes.size() == 3, "retry fails: one drain, one retry");
		CHECK(cvx::g_err == "fakeAlloc(728 bytes) failed: out of fake memory", "retry fails: message '%s'", cvx::g_err.c_str());
		M::fail_count = 0;
		CHECK(b.ensure(1) == CVX_OK && b.cap == 65, "the buffer grows again from empty: cap %zu", b.cap);
	}
	CHECK(M::balanced() && M::live.empty(), "retry fails: books");
}

/* (c) the size asked for is the generous size and does not fit: no drain, no retry, and the outgrown block stays parked.  (Today's
 * rule, pinned on purpose: a drain here might have made room.) */
template <typename T, typename M>
static void test_failure_without_retry(size_t bytes_expected) {
	constexpr size_t sz = cvx::BufElem<T>::kBytes;
	M::reset();
	{
		cvx::Buf<T, M> b;
		size_t mark = 0;
		b.hwm = &mark;
		CHECK(b.ensure(100) == CVX_OK, "first growth");
		void *first = b.p;
		const size_t cap1 = b.cap, mark1 = mark;
		M::fail_from = 2; M::fail_count = 1;
		const int rc = b.ensure(16 * cap1);      /* far beyond twice the capacity: want == asked */
		CHECK(rc == CVX_ERR_OOM, "no retry: rc %d", rc);
		CHECK(b.p == nullptr && b.cap == 0, "no retry: p %p cap %zu", (void *) b.p, b.cap);
		CHECK(M::drains == 0 && M::asked_bytes.size() == 2, "no retry: %ld drains, %zu allocator calls", M::drains, M::asked_bytes.size());
		CHECK(M::asked_bytes.back() == bytes_expected && bytes_expected == (16 * cap1 + 2 * cap1 + M::kSlack) * sz, "no retry: %zu bytes asked", M::asked_bytes.back());
		CHECK(M::parked.size() == 1 && M::parked.count(first) == 1 && M::frees == 0, "no retry: the outgrown block is still parked");
		CHECK(mark == mark1, "no retry: mark moved");
		char want_msg[128];
		snprintf(want_msg, sizeof(want_msg), "fakeAlloc(%zu bytes) failed: out of fake memory", bytes_expected);
		CHECK(cvx::g_err == want_msg, "no retry: message '%s'", cvx::g_err.c_str());
	}
	CHECK(M::live.empty() && M::parked.size() == 1 && M::frees == 0 && M::balanced(), "no retry: an empty buffer frees nothing as it goes");
}

/* (d) who frees what */
static void test_ownership() {
	using M = PinLike;
	using B = cvx::Buf<void, M>;
	M::reset();
	{
		B a;
		CHECK(a.ensure(10) == CVX_OK, "a");
		void *a1 = a.p;
		CHECK(a.ensure(a.cap + 1) == CVX_OK, "a grows");
		CHECK(M::parks == 1 && M::parked.size() == 1 && M::parked.count(a1) == 1 && M::frees == 0, "growth parks exactly the old block");
		void *a2 = a.p;
		const size_t a2cap = a.cap;

		B moved(std::move(a));      /* move construction */
		CHECK(a.p == nullptr && a.cap == 0, "move construction empties the source");
		CHECK(moved.p == a2 && moved.cap == a2cap && M::frees == 0, "move construction carries the block");

		size_t mark = 0;
		B t;
		t.hwm = &mark;
		CHECK(t.ensure(7) == CVX_OK, "t");
		void *t1 = t.p;
		t = std::move(moved);       /* move assignment */
		CHECK(moved.p == nullptr && moved.cap == 0, "move assignment empties the source");
		CHECK(t.p == a2 && t.cap == a2cap && t.hwm == &mark, "move assignment carries the block and keeps the target's mark");
		CHECK(M::frees == 1 && M::live.count(t1) == 0 && M::live.count(a2) == 1, "move assignment frees the target's old block, once, at once");

		B &same = t;
		t = std::move(same);        /* onto itself: nothing happens */
		CHECK(t.p == a2 && t.cap == a2cap && M::frees == 1, "self move");

		{
			B scoped;
			CHECK(scoped.ensure(1) == CVX_OK, "scoped");
		}
		CHECK(M::frees == 2 && M::parks == 1, "scope exit frees, and does not park");

		B early;
		CHECK(early.ensure(1) == CVX_OK, "early");
		early.release();
		CHECK(early.p == nullptr && early.cap == 0 && M::frees == 3, "release frees at once");
	}   /* a, moved, early: empty; t: a2 */
	CHECK(M::frees == 4 && M::live.empty() && M::bad_frees == 0, "every block freed exactly once: %ld frees, %ld bad", M::frees, M::bad_frees);
	CHECK(M::allocs == M::frees + (long) M::parked.size() && M::parked.size() == 1, "allocations = frees + parked: %ld = %ld + %zu", M::allocs, M::frees, M::parked.size());
	static_assert(!std::is_copy_constructible<B>::value && !std::is_copy_assignable<B>::value, "a buffer is not copied");
	static_assert(std::is_nothrow_move_constructible<B>::value && std::is_nothrow_move_assignable<B>::value, "a buffer moves");
}

int main() {
	long cases = 0;
	cases += sweep_capacities<uint8_t, DevLike>(dev_rule, "dev/1");
	cases += sweep_capacities<uint64_t, DevLike>(dev_rule, "dev/8");
	cases += sweep_capacities<E12, DevLike>(dev_rule, "dev/12");
	cases += sweep_capacities<void, PinLike>(pin_rule, "pin");
	test_retry_after_drain();
	test_failure_without_retry<E12, DevLike>((16 * 176 + 2 * 176 + 64) * 12);
	test_failure_without_retry<void, PinLike>(16 * 4208 + 2 * 4208 + 4096);
	test_ownership();
	if (g_failures) { printf("buf_test: %d FAILED\n", g_failures); return 1; }
	printf("buf_test: ok (%ld capacity cases)\n", cases);
	return 0;
}
