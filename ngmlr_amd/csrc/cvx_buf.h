/*
 * cvx_buf.h -- the runtime's one owning, grow-only buffer and its one growth rule.  Free of HIP: where the memory comes from is
 * the policy's business (cvx_rt.h: device and page-locked memory; tests/cpp/buf_test.cpp: a counting fake).
 *
 * A policy M supplies
 *   static const char *alloc(void **p, size_t bytes)   nullptr, or why not
 *   static void free(void *p)                          at once: waits for the device
 *   static void park(void *p)                          an outgrown block: given back later, when nothing waits for it
 *   static void drain()                                gives back what is parked
 *   static constexpr size_t kSlack                     elements added to every request
 *   static constexpr const char *kName                 the allocator, for the error text
 */
#ifndef CVX_BUF_H
#define CVX_BUF_H

#include <cstddef>

#include "cvx_rt_err.h"

namespace cvx {

template <typename T> struct BufElem { static constexpr size_t kBytes = sizeof(T); };
template <> struct BufElem<void> { static constexpr size_t kBytes = 1; };      /* untyped: counted in bytes */

template <typename T, typename M>
struct Buf {
	T *p = nullptr;
	size_t cap = 0;             /* elements */
	size_t *hwm = nullptr;      /* shared by the same buffer of every job slot of the handle (bytes) */

	Buf() = default;
	Buf(const Buf &) = delete;
	Buf &operator=(const Buf &) = delete;
	Buf(Buf &&o) noexcept : p(o.p), cap(o.cap), hwm(o.hwm) { o.p = nullptr; o.cap = 0; }
	Buf &operator=(Buf &&o) noexcept {      /* takes the block; the mark stays the target's (it belongs to the slot, not to the block) */
		if (this != &o) {
			release();
			p = o.p; cap = o.cap;
			o.p = nullptr; o.cap = 0;
		}
		return *this;
	}
	~Buf() { release(); }

	int ensure(size_t n) {
		if (n <= cap) return CVX_OK;
		constexpr size_t sz = BufElem<T>::kBytes;
		const size_t old = cap;
		if (p) {
			M::park(p);
			p = nullptr; cap = 0;
		}
		const size_t asked = n + n / 8 + M::kSlack;
		size_t want = asked;
		if (want < 2 * old) want = 2 * old;      /* a buffer that has to grow at least doubles; the first allocation stays close to what was asked for */
		if (hwm && want * sz < *hwm && *hwm / 16 <= asked * sz) want = (*hwm + sz - 1) / sz;      /* (never more than 16 x what was asked for) */
		void *q = nullptr;
		const char *why = M::alloc(&q, want * sz);
		if (why && want > asked) {      /* the generous size does not fit: give back what is parked, then what was asked for may */
			M::drain();
			want = asked;
			why = M::alloc(&q, want * sz);
		}
		if (why) {
			set_err("%s(%zu bytes) failed: %s", M::kName, want * sz, why);
			return CVX_ERR_OOM;
		}
		p = static_cast<T *>(q);
		cap = want;
		if (hwm && cap * sz > *hwm) *hwm = cap * sz;
		return CVX_OK;
	}
	void release() {      /* the destructor's work, for the few places that free early */
		if (p) M::free(p);
		p = nullptr;
		cap = 0;
	}
	template <typename U> U *as() const { return static_cast<U *>(p); }
};

}  // namespace cvx

#endif
