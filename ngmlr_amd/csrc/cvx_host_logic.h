/*
 * cvx_host_logic.h -- the device-independent half of the host runtime (cvx_rt_align.cpp):
 * how a batch of cvx_tile is laid out and packed for upload and which bytes travel to the device when
 * (build_upload_schedule: blocks that travel as they are, pieces, one record per transfer), and how the corridor plans that
 * come back from plan_kernel are turned into kernel classes, arena offsets and work lists, and
 * those into the compute stage's launch schedule (build_schedule: what is launched, in which order,
 * on which stream, and how each class is walked).
 * Header-only and free of HIP so that the CPU suite can exercise it (tests/cpp/host_logic_test.cpp).
 */
#ifndef CVX_HOST_LOGIC_H
#define CVX_HOST_LOGIC_H

#include <algorithm>
#include <atomic>
#include <cmath>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <mutex>
#include <system_error>
#include <thread>
#include <vector>

#include <pthread.h>

#include "cvx_align.h"
#include "cvx_types.h"

namespace cvx {

/* ------------------------------------------------------------------ kernel classes */

struct KernelClass {
	int m;                           /* slots per lane */
	int gang;                        /* waves per tile (1; 2 or 3: a gang of waves on one ring, float runs only) */
	int ring() const { return 64 * m * gang; }
};

/* fill_ring_kernel instantiations the runtime dispatches whole tiles to, smallest ring first.
 * Rings of more than 256 slots need so many registers (M = 6: 133, M = 8: 170 VGPRs) that only two
 * or three waves fit a SIMD; such tiles are chained instead (ONT mix, 60 000 tiles: 5 950 -> 7 180
 * Gbp/h when everything above M = 4 goes to 64-row blocks). */
/* Round 5: rings of 384 and 576 slots as GANGS of two / three M = 3 waves in one workgroup (the lane boundary between the
 * waves goes through LDS, cvx_kernels.hip): the retry loop's doubled corridors (257-576 live rows) are whole tiles again. */
static const KernelClass kClasses[] = { {1, 1}, {2, 1}, {3, 1}, {4, 1}, {3, 2}, {3, 3} };
static const int kNumClasses = (int) (sizeof(kClasses) / sizeof(kClasses[0]));

/* Corridors with more live rows than the widest single-wave ring are cut into row blocks that run
 * as a dependency chain (kFillChain).  Smaller blocks = more blocks of a tile in flight at once
 * (about need / rows-per-block): aim for 16 or more. */
static const int kChainClasses[] = {1, 2, 4};          /* M of the chain kernels: 64, 128, 256 rows per block */
static const int kNumChainClasses = 3;
/* A batch with fewer whole-tile waves than this cannot fill the device by tile parallelism alone:
 * its chains use the smallest blocks (a tile's time is then about (2 H + w) single-wave steps,
 * whatever its width), and its very long tiles are chained even if a ring would hold them. */
static const int kSmallBatchTiles = 2048;
static const int kLongTileSteps = 32768;
/* whole tiles of at least this many steps are filled by the exact-tracking instantiation right away (build_schedule),
 * as long as their class holds at most kExactDirectMaxTiles of them */
static const int kExactDirectSteps = 65536;
static const int kExactDirectMaxTiles = 4096;
/* streaming jobs smaller than this alternate between the runtime's two stream sets (cvx_rt_align.cpp, stage_compute) */
static const int kSmallJobTiles = 2048;
/* an upload whose host packing moves fewer bytes than this is not worth a thread (build_upload_schedule): one thread, one
 * piece; above it the batch is packed and copied in kUploadPieces pieces, each piece's copies under the packing of the next */
static const uint64_t kPackThreadBytes = 8ull << 20;
static const int kUploadPieces = 8;
inline int chain_class_for(int need, bool small_batch) {
	/* measured (C5 mix, 96 tiles): 64-row blocks 100 ms, 128-row 117 ms, 256-row 174 ms -- a tile's
	 * time is its block count times the lag between neighbouring blocks, and a step of a 64-row block
	 * is the shortest.  Batches that fill the device were tried with 128-row blocks (fewer instructions
	 * per cell): ONT mix, 60 000 tiles, 7 600-7 650 Gbp/h against 7 660-7 770 with 64-row blocks, and
	 * with the blocks at raised wave priority (FillArgs::chain_prio) 64 rows win clearly (8 320-8 450
	 * against 7 580-8 040).  The larger classes stay selectable (CVX_TUNE_CHAIN_M). */
	(void) need; (void) small_batch;
	return 0;
}

/* ------------------------------------------------------------------ host threads */

/* The process's pack threads: one persistent pool shared by every handle (eight handles on an 8-device node
 * used to spawn 24 fresh threads each per call -- 192 threads on a host that behaves like ~32 cores).  Size:
 * CVX_PACK_THREADS, else min(hardware threads, 16); the calling thread works too, so a pool of size 1 has no
 * worker threads at all.  Handles that pack at the same time share the workers task by task. */
class PackPool {
public:
	static PackPool &get() {
		static PackPool pool;
		return pool;
	}
	int size() const { return n_threads_; }
	/* runs fn(0) ... fn(n_tasks - 1), returns when all are done */
	void run(int n_tasks, const std::function<void(int)> &fn) {
		if (n_tasks <= 0) return;
		if (n_tasks == 1 || n_threads_ <= 1) { for (int i = 0; i < n_tasks; ++i) fn(i); return; }
		Group g;
		g.left = n_tasks;
		{
			std::lock_guard<std::mutex> lk(m_);
			for (int i = 0; i < n_tasks; ++i) q_.push_back(Task{&g, &fn, i});
		}
		cv_.notify_all();
		/* the caller takes tasks as well (its own or another caller's: whatever is at the front) */
		for (;;) {
			Task t;
			{
				std::unique_lock<std::mutex> lk(m_);
				if (g.left == 0) break;
				if (q_.empty()) { done_.wait(lk, [&] { return g.left == 0 || !q_.empty(); }); continue; }
				t = q_.front();
				q_.pop_front();
			}
			execute(t);
		}
	}
private:
	struct Group { int left = 0; };
	struct Task { Group *g; const std::function<void(int)> *fn; int i; };
	PackPool() {
		int hw = (int) std::thread::hardware_concurrency();
		n_threads_ = std::max(1, std::min(hw > 0 ? hw : 1, 16));
		if (const char *e = getenv("CVX_PACK_THREADS")) n_threads_ = std::max(1, atoi(e));
		/* (a worker that cannot be started is not an error: the callers of run take its tasks) */
		workers_.reserve((size_t) n_threads_ - 1);
		for (int i = 1; i < n_threads_; ++i) { try { workers_.emplace_back([this] { loop(); }); } catch (const std::system_error &) { break; } }
	}
	~PackPool() {
		{ std::lock_guard<std::mutex> lk(m_); stop_ = true; }
		cv_.notify_all();
		for (auto &t : workers_) t.join();
	}
	void execute(const Task &t) {
		(*t.fn)(t.i);
		bool last;
		{ std::lock_guard<std::mutex> lk(m_); last = (--t.g->left == 0); }
		if (last) done_.notify_all();
	}
	void loop() {
		pthread_setname_np(pthread_self(), "cvx-pack");
		for (;;) {
			Task t;
			{
				std::unique_lock<std::mutex> lk(m_);
				cv_.wait(lk, [&] { return stop_ || !q_.empty(); });
				if (stop_ && q_.empty()) return;
				t = q_.front();
				q_.pop_front();
			}
			execute(t);
			done_.notify_all();      /* a caller waiting for work to help with */
		}
	}
	std::mutex m_;
	std::condition_variable cv_, done_;
	std::deque<Task> q_;
	std::vector<std::thread> workers_;
	bool stop_ = false;
	int n_threads_ = 1;
};

/* fn(begin, end) over [0, n) in up to `threads` ranges balanced by the work prefix sums
 * (prefix[i] = work of items < i, n + 1 entries), on the process's pack threads */
template <typename F>
void parallel_ranges(int n, const std::vector<uint64_t> &prefix, int threads, F fn) {
	if (threads <= 1 || n < 2 * threads) { fn(0, n); return; }
	const uint64_t total = prefix[(size_t) n];
	std::vector<std::pair<int, int>> ranges;
	int begin = 0;
	for (int k = 1; k <= threads && begin < n; ++k) {
		int end = n;
		if (k < threads) {
			const uint64_t target = total / (uint64_t) threads * (uint64_t) k;
			end = (int) (std::upper_bound(prefix.begin(), prefix.begin() + n + 1, target) - prefix.begin());
			if (end <= begin) end = begin + 1;
			if (end > n) end = n;
		}
		ranges.emplace_back(begin, end);
		begin = end;
	}
	PackPool::get().run((int) ranges.size(), [&](int i) { fn(ranges[(size_t) i].first, ranges[(size_t) i].second); });
}

/* ------------------------------------------------------------------ upload layout + packing */

struct UploadLayout {
	uint64_t pad = 0;               /* defined bytes before the first, between the two blocks and after the last sequence (multiple of 256) */
	uint64_t seq_total = 0;         /* bytes of the seq arena: [pad][every read][pad][every reference][pad] */
	uint64_t qry_base = 0, qry_bytes = 0;   /* arena offset / size of the block of reads */
	uint64_t ref_base = 0, ref_bytes = 0;   /* ... of the block of references (ref_base is a multiple of 256) */
	uint64_t n_rows = 0;            /* read rows of all tiles */
	uint64_t arena_rows = 0;        /* entries of the rows arena: the rows of the tiles whose corridors came as arrays (closed forms own none) */
	uint64_t delta_total = 0;       /* bytes of the row-step stream (H bytes, 4-byte aligned, per tile whose rows come as arrays) */
	std::vector<RowSrc> rsrc;       /* per tile: where its rows come from (src_off = offset into the step stream until packed) */
	bool windows = false;           /* references decoded on the device from the resident genome: their block is not uploaded */
	bool segments = false;          /* queries written on the device from the call's read block (cvx_segments.h): their block is neither packed nor uploaded */
	/* the caller's reads (references) lie back to back in tile order: the block can travel as it is, without
	 * packing, when the runtime finds it in page-locked memory (cvx_host_alloc) */
	bool qry_contig = false, ref_contig = false;
	std::vector<uint64_t> wprefix;  /* packing work per tile (bytes moved if everything is packed), prefix sums */
};

enum { kLayoutOk = 0, kLayoutMalformed = 1, kLayoutTooLarge = 2 };

/* A closed form the device and the host evaluate alike: finite parameters, a positive finite slope, and every row's
 * offset ((float) y - d) / k - right inside the int32 range with room to spare -- the float -> int conversion of
 * affine_row_offset is undefined behaviour on the host and saturating on the device beyond it.  The
 * expression is monotone in y for k > 0, so rows 0 and H bound all of them. */
inline bool affine_form_ok(float k, float d, float right, int32_t H) {
	if (!(k > 0.0f && k < 3.0e38f) || !std::isfinite(d) || !std::isfinite(right)) return false;
	const double lo = (0.0 - (double) d) / (double) k - (double) right;
	const double hi = ((double) (H > 0 ? H : 0) - (double) d) / (double) k - (double) right;
	return std::fabs(lo) < 2.0e9 && std::fabs(hi) < 2.0e9;
}

/* Validates the tiles and assigns arena offsets (TileIn).  On kLayoutMalformed *bad is the
 * offending tile; kLayoutTooLarge: more than 4 GiB of bases (32-bit sequence offsets). */
inline int upload_layout(int n, const cvx_tile *tiles, std::vector<TileIn> &tin, UploadLayout &L, int *bad, bool windows = false, bool segments = false) {
	uint64_t ref_bytes = 0, n_rows = 0, qry_bytes = 0;
	int64_t max_hw = 0;
	bool qc = n > 0 && !segments, rc = n > 0 && !windows;
	for (int i = 0; i < n; ++i) {
		const cvx_tile &t = tiles[i];
		const bool rows_given = t.corridor_kind == CVX_CORRIDOR_ROWS;
		if (t.ref_len < 0 || t.qry_len < 0 || (t.ref_len > 0 && !t.ref && !windows) || (t.qry_len > 0 && !t.qry && !segments) ||
				(rows_given && t.qry_len > 0 && (!t.row_offset || !t.row_length)) ||
				(rows_given && ((t.row_stride_bytes & 3) || t.row_stride_bytes < 4)) ||
				t.corridor_kind < CVX_CORRIDOR_ROWS || t.corridor_kind > CVX_CORRIDOR_CONST ||
				(t.corridor_kind == CVX_CORRIDOR_AFFINE && !affine_form_ok(t.corridor_k, t.corridor_d, t.corridor_right, t.qry_len)) ||
				(!rows_given && t.corridor_width < 0)) {
			if (bad) *bad = i;
			return kLayoutMalformed;
		}
		if (i > 0) {
			if (!segments && tiles[i - 1].qry + tiles[i - 1].qry_len != t.qry) qc = false;
			if (!windows && tiles[i - 1].ref + tiles[i - 1].ref_len != t.ref) rc = false;
		}
		ref_bytes += (uint64_t) t.ref_len;
		qry_bytes += (uint64_t) t.qry_len;
		n_rows += (uint64_t) t.qry_len;
		max_hw = std::max<int64_t>(max_hw, (int64_t) t.ref_len + t.qry_len);
	}
	L.pad = ((uint64_t) max_hw + kRingMax + 256 + 255) / 256 * 256;
	L.qry_base = L.pad;
	L.qry_bytes = qry_bytes;
	L.ref_base = (L.qry_base + qry_bytes + L.pad + 255) / 256 * 256;
	L.ref_bytes = ref_bytes;
	L.seq_total = L.ref_base + ref_bytes + L.pad + 64;
	L.n_rows = n_rows;
	L.windows = windows;
	L.segments = segments;
	L.qry_contig = qc;
	L.ref_contig = rc;
	if (L.seq_total >= 0xFFFF0000ull) return kLayoutTooLarge;
	tin.resize((size_t) n);
	L.rsrc.assign((size_t) n, RowSrc());
	L.wprefix.assign((size_t) n + 1, 0);
	uint64_t qo = L.qry_base, ro = 0, dof = 0, rso = L.ref_base;
	for (int i = 0; i < n; ++i) {
		const cvx_tile &t = tiles[i];
		TileIn &ti = tin[(size_t) i];
		ti.ref_off = (uint32_t) rso;
		rso += (uint64_t) t.ref_len;
		ti.qry_off = (uint32_t) qo;
		qo += (uint64_t) t.qry_len;
		ti.W = t.ref_len;
		ti.H = t.qry_len;
		ti.row_off = 0;
		ti.reserved = 0;
		RowSrc &rs = L.rsrc[(size_t) i];
		memset(&rs, 0, sizeof(rs));
		uint64_t row_work = 0;
		if (t.corridor_kind == CVX_CORRIDOR_AFFINE) {
			rs.fmt = kRowsAffine; rs.width = t.corridor_width; rs.k = t.corridor_k; rs.d = t.corridor_d; rs.right = t.corridor_right;
		} else if (t.corridor_kind == CVX_CORRIDOR_CONST) {
			rs.fmt = kRowsConst; rs.width = t.corridor_width; rs.off0 = t.corridor_offset;
		} else {
			rs.src_off = dof; rs.fmt = kRowsDelta8;
			ti.row_off = ro;                       /* only corridors that came as arrays own a slice of the rows arena */
			ro += (uint64_t) t.qry_len;
			dof += ((uint64_t) t.qry_len + 3) / 4 * 4;
			row_work = 9ull * (uint64_t) t.qry_len;
		}
		L.wprefix[(size_t) i + 1] = L.wprefix[(size_t) i] + (windows ? 0 : (uint64_t) t.ref_len) + (segments ? 0 : (uint64_t) t.qry_len) + row_work + 64;
	}
	L.delta_total = dof;
	L.arena_rows = ro;
	return kLayoutOk;
}

/* the kernels prefetch a little past either end of a tile: all three pads must be defined (host staging form) */
inline void upload_zero_pads(const UploadLayout &L, uint8_t *hseq) {
	if (!L.segments) {      /* (segments: block A never leaves the staging; the device clears the two pads itself) */
		memset(hseq, 0, (size_t) L.qry_base);
		memset(hseq + (size_t) (L.qry_base + L.qry_bytes), 0, (size_t) (L.ref_base - L.qry_base - L.qry_bytes));
	}
	if (!L.windows) memset(hseq + (size_t) (L.ref_base + L.ref_bytes), 0, (size_t) (L.seq_total - L.ref_base - L.ref_bytes));
}

/* Step bytes of rows [1, H) of a tile whose (offset, length) arrays are plain int32 arrays (stride 4), eight
 * rows per iteration.  Returns the first row it did not finish (H when all rows fit the one-byte form; a row
 * whose width differs or whose step is outside -128..127 stops it, and the scalar loop decides). */
#if defined(__x86_64__)
#include <immintrin.h>
__attribute__((target("avx2"))) inline int pack_steps_avx2(const int32_t *off, const int32_t *len, int H, int32_t w0, int8_t *dst) {
	const __m256i vw = _mm256_set1_epi32(w0);
	const __m256i lo = _mm256_set1_epi32(-129), hi = _mm256_set1_epi32(128);
	const __m256i big = _mm256_set1_epi32(1 << 30), nbig = _mm256_set1_epi32(-(1 << 30));
	const __m256i pick = _mm256_setr_epi8(0, 4, 8, 12, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
			0, 4, 8, 12, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1);
	int y = 1;
	for (; y + 8 <= H; y += 8) {
		const __m256i cur = _mm256_loadu_si256(reinterpret_cast<const __m256i *>(off + y));
		const __m256i prv = _mm256_loadu_si256(reinterpret_cast<const __m256i *>(off + y - 1));
		const __m256i l = _mm256_loadu_si256(reinterpret_cast<const __m256i *>(len + y));
		/* with both offsets inside (-2^30, 2^30) the 32-bit difference cannot wrap (anything else: scalar loop) */
		const __m256i d = _mm256_sub_epi32(cur, prv);
		const __m256i inr = _mm256_and_si256(_mm256_and_si256(_mm256_cmpgt_epi32(cur, nbig), _mm256_cmpgt_epi32(big, cur)),
				_mm256_and_si256(_mm256_cmpgt_epi32(prv, nbig), _mm256_cmpgt_epi32(big, prv)));
		const __m256i ok = _mm256_and_si256(_mm256_and_si256(_mm256_and_si256(_mm256_cmpgt_epi32(d, lo), _mm256_cmpgt_epi32(hi, d)), _mm256_cmpeq_epi32(l, vw)), inr);
		if (_mm256_movemask_epi8(ok) != -1) break;
		const __m256i b = _mm256_shuffle_epi8(d, pick);
		const uint32_t b0 = (uint32_t) _mm256_extract_epi32(b, 0), b1 = (uint32_t) _mm256_extract_epi32(b, 4);
		memcpy(dst + y, &b0, 4);
		memcpy(dst + y + 4, &b1, 4);
	}
	return y;
}
#endif

/* Rows of the tiles that do not fit the one-byte form, collected by one packing thread. */
struct RowOverflow {
	std::vector<int32_t> tiles;        /* tile indices, in packing order */
	std::vector<RowDesc> rows;         /* their rows, back to back */
};

/* copies tiles [begin, end) into the staging arenas (callable from several threads at once).  Rows that
 * come as arrays go to the step stream `hdelta` (one byte per row: offset[y] - offset[y-1]; rsrc[i] gets row
 * 0's offset and the common width); a tile whose width changes or whose offset jumps by more than a byte is
 * marked kRowsExplicit and its rows are appended to `ovf` instead.  Closed-form corridors have nothing to
 * pack.  copy_qry / copy_ref = false: that block travels straight from the caller's page-locked memory. */
inline void upload_pack(int begin, int end, const cvx_tile *tiles, const std::vector<TileIn> &tin,
		uint8_t *hseq, uint8_t *hdelta, std::vector<RowSrc> &rsrc, RowOverflow &ovf, bool copy_qry = true, bool copy_ref = true) {
	for (int i = begin; i < end; ++i) {
		const cvx_tile &t = tiles[i];
		const TileIn &ti = tin[(size_t) i];
		if (t.ref_len && copy_ref) memcpy(hseq + ti.ref_off, t.ref, (size_t) t.ref_len);
		if (t.qry_len && copy_qry) memcpy(hseq + ti.qry_off, t.qry, (size_t) t.qry_len);
		RowSrc &rs = rsrc[(size_t) i];
		if (rs.fmt != kRowsDelta8) continue;       /* closed form: generated on the device */
		const char *po = (const char *) t.row_offset;
		const char *pl = (const char *) t.row_length;
		const size_t stride = (size_t) t.row_stride_bytes;
		const int H = t.qry_len;
		if (H <= 0) continue;
		int8_t *dst = reinterpret_cast<int8_t *>(hdelta + rs.src_off);
		int32_t prev, w0;
		memcpy(&prev, po, 4);
		memcpy(&w0, pl, 4);
		rs.off0 = prev;
		rs.width = w0;
		dst[0] = 0;
		bool fits = true;
		int y_from = 1;
#if defined(__x86_64__)
		/* plain int32 arrays with in-range first offset: eight rows per iteration (the scalar loop below finishes
		 * the tail and is the judge of any row the vector loop stopped at) */
		static const bool have_avx2 = __builtin_cpu_supports("avx2");
		if (have_avx2 && stride == 4 && H > 16) {
			y_from = pack_steps_avx2(reinterpret_cast<const int32_t *>(po), reinterpret_cast<const int32_t *>(pl), H, w0, dst);
			if (y_from > 1) memcpy(&prev, po + (size_t) (y_from - 1) * stride, 4);
		}
#endif
		for (int y = y_from; y < H; ++y) {
			int32_t o, l;
			memcpy(&o, po + (size_t) y * stride, 4);
			memcpy(&l, pl + (size_t) y * stride, 4);
			const int64_t d = (int64_t) o - (int64_t) prev;
			if (l != w0 || d < -128 || d > 127) { fits = false; break; }
			dst[y] = (int8_t) d;
			prev = o;
		}
		if (!fits) {
			rs.fmt = kRowsExplicit;
			ovf.tiles.push_back(i);
			const size_t at = ovf.rows.size();
			ovf.rows.resize(at + (size_t) H);
			for (int y = 0; y < H; ++y) {
				RowDesc rd;
				memcpy(&rd.off, po + (size_t) y * stride, 4);
				memcpy(&rd.len, pl + (size_t) y * stride, 4);
				ovf.rows[at + (size_t) y] = rd;
			}
		}
	}
}

/* what expand_rows_kernel does on the device, for the host's own needs (chain planning, tests):
 * the (offset, length) rows of tile i.  hrowsx: the explicit-rows buffer (rsrc[i].src_off indexes it). */
inline void expand_rows_host(const RowSrc &rs, int H, const uint8_t *hdelta, const RowDesc *hrowsx, RowDesc *out) {
	if (rs.fmt == kRowsExplicit) {
		if (H > 0) memcpy(out, hrowsx + rs.src_off, (size_t) H * sizeof(RowDesc));
		return;
	}
	if (rs.fmt == kRowsAffine || rs.fmt == kRowsConst) {
		for (int y = 0; y < H; ++y) {
			out[y].off = rs.fmt == kRowsConst ? rs.off0 : affine_row_offset(y, rs.d, rs.k, rs.right);
			out[y].len = rs.width;
		}
		return;
	}
	const int8_t *d = reinterpret_cast<const int8_t *>(hdelta + rs.src_off);
	int32_t o = rs.off0;
	for (int y = 0; y < H; ++y) {
		if (y > 0) o += (int32_t) d[y];
		out[y].off = o;
		out[y].len = rs.width;
	}
}

/* The misfits' rows (none in any corridor the reference builds) behind the packing: the lists of all packing ranges, back
 * to back, are the explicit-rows buffer.  misfit_rows: its entries; place_misfits fills hx (room for that many) and points
 * every kRowsExplicit tile's src_off -- the tile's step-stream offset until here -- at its rows in it. */
inline uint64_t misfit_rows(const std::vector<RowOverflow> &overflow) {
	uint64_t n_x = 0;
	for (const RowOverflow &o : overflow) n_x += o.rows.size();
	return n_x;
}
inline void place_misfits(const std::vector<RowOverflow> &overflow, const std::vector<TileIn> &tin, std::vector<RowSrc> &rsrc, RowDesc *hx) {
	uint64_t at = 0;
	for (const RowOverflow &o : overflow) {
		uint64_t r = 0;
		for (int32_t ti : o.tiles) {
			rsrc[(size_t) ti].src_off = at + r;
			r += (uint64_t) tin[(size_t) ti].H;
		}
		if (!o.rows.empty()) memcpy(hx + at, o.rows.data(), o.rows.size() * sizeof(RowDesc));
		at += o.rows.size();
	}
}

/* ------------------------------------------------------------------ upload schedule */

/* What stage_upload (cvx_rt_align.cpp) moves to the device for a laid-out batch, decided here so that the CPU suite can
 * check it: which blocks travel as they are, how the batch is cut into pieces, and one record per transfer in issue order.
 * The stage itself packs a piece, then issues that piece's records. */

enum UploadDst { kToSeq = 0, kToDelta = 1, kToReads = 2 };      /* the sequence arena, the step-stream arena, the job's read block (segments) */
/* the job's sequence / step staging, the page-locked block of zeros, the caller's block of reads / of references;
 * kClearOnDevice: no source, the destination is cleared by the device itself; segments: the caller's read block as it
 * lies in page-locked memory, or the job's staging of it (copied there piece by piece, each piece in front of its record) */
enum UploadSrc { kFromSeqStaging = 0, kFromDeltaStaging = 1, kFromZeros = 2, kFromQryBlock = 3, kFromRefBlock = 4, kClearOnDevice = 5,
	kFromReadBlock = 6, kFromReadStaging = 7 };
/* a read block that goes through the staging travels in pieces of this many bytes: a piece's DMA runs under the host's copy of the next */
static const uint64_t kReadPieceBytes = 4ull << 20;

struct UploadCopy {
	int dst = kToSeq, src = kFromSeqStaging;
	uint64_t dst_off = 0, src_off = 0, len = 0;
};

struct UploadPiece {
	int t0 = 0, t1 = 0;              /* tiles packed for this piece */
	size_t rec0 = 0, rec1 = 0;       /* copies[rec0, rec1): issued once they are packed */
};

struct UploadSchedule {
	bool zc_qry = false, zc_ref = false;   /* the block of reads / of references travels straight from the caller's page-locked arena */
	bool pack_seq = true;                  /* anything left for the host to copy into the sequence staging? */
	uint64_t zero_copy_bytes = 0;
	uint64_t pack_work = 0;                /* bytes the host still moves */
	int threads = 1;                       /* pack threads per piece */
	uint64_t zero_bytes = 0;               /* size the block of zeros must have (0: not needed) */
	std::vector<UploadCopy> copies;        /* [0, n_leading): before any packing; then the pieces' ranges; [n_staged, size()): behind the whole upload */
	size_t n_leading = 0, n_staged = 0;
	std::vector<UploadPiece> pieces;
	/* segments mode: the read block, a destination of its own, in issue order in front of everything else (kToReads; one
	 * record from the caller's arena, or one per piece of the staging); the stage kernel runs behind copies[n_staged, size()) */
	bool zc_reads = false;
	int read_threads = 1;                  /* > 1: the staging's pieces are copied side by side on the pack threads, then issued; 1: piece by piece, each DMA under the copy of the next */
	std::vector<UploadCopy> read_copies;
};

/* L, tin: of upload_layout, L.rsrc not yet packed (the step-stream cut-offs read src_off); qry_pinned / ref_pinned: the
 * caller's block of reads / references (qry_bytes + 4 / ref_bytes + 4 bytes from the first tile's pointer) lies inside one
 * page-locked block; threads_on_offer: pack threads the handle may use. */
inline void build_upload_schedule(const UploadLayout &L, const std::vector<TileIn> &tin, int n, bool qry_pinned, bool ref_pinned,
		int threads_on_offer, UploadSchedule &s, uint64_t thread_bytes = kPackThreadBytes, uint64_t read_bytes = 0, bool reads_pinned = false) {
	const bool windows = L.windows, segments = L.segments;
	/* a block of sequences that already lies back to back in page-locked memory is not packed: the
	 * device pulls it out of the caller's arena (the job's staging then holds only what the host wrote) */
	s.zc_qry = n > 0 && !segments && L.qry_contig && L.qry_bytes > 0 && qry_pinned;
	s.zc_ref = n > 0 && !windows && L.ref_contig && L.ref_bytes > 0 && ref_pinned;
	s.zero_copy_bytes = (s.zc_qry ? L.qry_bytes : 0) + (s.zc_ref ? L.ref_bytes : 0);
	s.pack_seq = !((s.zc_qry || segments) && (s.zc_ref || windows));      /* off when neither block travels from the staging */
	s.copies.clear(); s.pieces.clear();
	/* segments: the read block (read_bytes bytes, read_bytes + 4 of them inside one page-locked block when reads_pinned) as it
	 * is, or through the job's staging; every record a whole number of dwords (the last piece rounds up into the staging's /
	 * the block's slack), every boundary a multiple of 256 */
	s.read_copies.clear();
	s.zc_reads = segments && n > 0 && read_bytes > 0 && reads_pinned;
	if (segments && n > 0 && read_bytes > 0) {
		const uint64_t total = (read_bytes + 3) / 4 * 4;
		if (s.zc_reads) {
			s.read_copies.push_back(UploadCopy{kToReads, kFromReadBlock, 0, 0, total});
			s.zero_copy_bytes += read_bytes;
		} else {
			for (uint64_t at = 0; at < total; at += kReadPieceBytes)
				s.read_copies.push_back(UploadCopy{kToReads, kFromReadStaging, at, at, std::min<uint64_t>(kReadPieceBytes, total - at)});
		}
	}
	s.read_threads = (!s.read_copies.empty() && !s.zc_reads && read_bytes >= thread_bytes) ? std::max(1, threads_on_offer) : 1;      /* (the rule of the packing: not worth a thread below ~8 MB) */
	auto add = [&](int dst, int src, uint64_t dst_off, uint64_t src_off, uint64_t len) { s.copies.push_back(UploadCopy{dst, src, dst_off, src_off, len}); };
	/* the three pads: uploaded with the packed blocks (upload_zero_pads wrote them into the staging), or copied from zeros
	 * around the blocks that travel as they are (queued in front of those copies: a copy rounded up to whole dwords may
	 * spill a few bytes into the pad that follows) */
	s.zero_bytes = 0;
	if (s.zc_qry || s.zc_ref) {
		/* Pads around blocks that travel as they are: copied from a page-locked block of zeros, whole 256-byte
		 * units (SDMA engines; a memset would be a kernel that has to find wave slots beside the fill), queued
		 * BEFORE the blocks, which then overwrite the few bytes of overlap.  A block's own copy is rounded up to
		 * whole dwords: up to three bytes of whatever follows it in the caller's arena land in the pad behind it --
		 * pads only have to be readable (every cell outside a tile is forced to the empty element), not zero. */
		const uint64_t zmax = L.pad + 1024;
		s.zero_bytes = zmax;
		auto zero_range = [&](uint64_t lo, uint64_t hi) {      /* [lo, hi) widened to 256-byte units, inside the arena */
			lo = lo / 256 * 256;
			hi = std::min<uint64_t>((hi + 255) / 256 * 256, (L.seq_total + 255) / 256 * 256);
			for (uint64_t at = lo; at < hi; at += zmax / 256 * 256)
				add(kToSeq, kFromZeros, at, 0, std::min<uint64_t>(hi - at, zmax / 256 * 256));
		};
		if (s.zc_qry) {
			zero_range(0, L.qry_base);
			zero_range(L.qry_base + L.qry_bytes, L.ref_base);
			add(kToSeq, kFromQryBlock, L.qry_base, 0, (L.qry_bytes + 3) / 4 * 4);
		}
		if (s.zc_ref) {
			zero_range(L.ref_base + L.ref_bytes, L.seq_total);
			add(kToSeq, kFromRefBlock, L.ref_base, 0, (L.ref_bytes + 3) / 4 * 4);
		}
	}
	s.n_leading = s.copies.size();
	/* what the host still moves per tile decides whether packing is worth threads and pieces */
	s.pack_work = L.delta_total * 9ull;
	if (!s.zc_qry && !segments) s.pack_work += L.qry_bytes;
	if (!s.zc_ref && !windows) s.pack_work += L.ref_bytes;
	s.threads = std::max(1, threads_on_offer);
	if (s.pack_work < thread_bytes) s.threads = 1;      /* not worth a thread below ~8 MB */
	const int pieces = s.threads > 1 ? kUploadPieces : 1;
	const std::vector<uint64_t> &wprefix = L.wprefix;
	int t0 = 0;
	/* bytes of the two blocks of the sequence staging / of the step staging already on their way (block A = [pad][reads][pad], block B = [references][pad]) */
	uint64_t a_done = 0, b_done = L.ref_base, delta_done = 0;
	const uint64_t a_end_all = L.ref_base, b_end_all = (L.seq_total + 255) / 256 * 256;
	for (int pc = 1; pc <= pieces; ++pc) {
		int t1 = n;
		if (pc < pieces) {
			const uint64_t target = wprefix[(size_t) n] / (uint64_t) pieces * (uint64_t) pc;
			t1 = (int) (std::upper_bound(wprefix.begin(), wprefix.end(), target) - wprefix.begin());
			t1 = std::min(std::max(t1, t0), n);
		}
		const size_t rec0 = s.copies.size();
		/* Copy boundaries are multiples of 256 bytes: a host-to-device copy whose address or size is
		 * not dword-aligned is not handed to the SDMA engines but to a blit kernel that pulls the bytes
		 * over PCIe with compute units the fill needs.  The bytes below the rounded-down end are all
		 * packed (tiles are laid out in order inside either block); the remainder travels with the next
		 * piece, the last piece runs to the aligned end. */
		if (!s.zc_qry && !segments) {
			const uint64_t a_end = (t1 == n) ? a_end_all : (uint64_t) tin[(size_t) t1].qry_off / 256 * 256;
			if (a_end > a_done) add(kToSeq, kFromSeqStaging, a_done, a_done, a_end - a_done);
			a_done = std::max(a_done, a_end);
		}
		if (!s.zc_ref && !windows) {
			const uint64_t b_end = (t1 == n) ? b_end_all : (uint64_t) tin[(size_t) t1].ref_off / 256 * 256;
			if (b_end > b_done) add(kToSeq, kFromSeqStaging, b_done, b_done, b_end - b_done);
			b_done = std::max(b_done, b_end);
		}
		if (L.delta_total) {
			uint64_t del_end = L.delta_total;
			if (t1 < n) {        /* first tile at or after t1 whose rows travel as steps (src_off = step-stream offset until the misfits are renumbered, place_misfits) */
				int q = t1;
				while (q < n && L.rsrc[(size_t) q].fmt != kRowsDelta8 && L.rsrc[(size_t) q].fmt != kRowsExplicit) q++;
				if (q < n) del_end = L.rsrc[(size_t) q].src_off;
			}
			del_end = (t1 == n) ? (del_end + 255) / 256 * 256 : del_end / 256 * 256;
			if (del_end > delta_done) add(kToDelta, kFromDeltaStaging, delta_done, delta_done, del_end - delta_done);
			delta_done = std::max(delta_done, del_end);
		}
		s.pieces.push_back(UploadPiece{t0, t1, rec0, s.copies.size()});
		t0 = t1;
	}
	s.n_staged = s.copies.size();
	/* windows: the references are decoded on the device straight into the arena, and the pad behind them is cleared there */
	if (windows && n) add(kToSeq, kClearOnDevice, L.ref_base + L.ref_bytes, 0, L.seq_total - L.ref_base - L.ref_bytes);
	/* segments: the queries are written on the device straight into the arena, and the two pads upload_zero_pads would have
	 * written around their block are cleared there */
	if (segments && n) {
		add(kToSeq, kClearOnDevice, 0, 0, L.qry_base);
		add(kToSeq, kClearOnDevice, L.qry_base + L.qry_bytes, 0, L.ref_base - L.qry_base - L.qry_bytes);
	}
}

/* Packs one piece of the schedule into the staging arenas on the schedule's pack threads (upload_pack per range);
 * every packing range of the piece collects the rows of its misfits in its own list, appended to `overflow`. */
inline void upload_pack_piece(const UploadSchedule &s, const UploadPiece &p, const cvx_tile *tiles, const std::vector<TileIn> &tin,
		UploadLayout &L, uint8_t *hseq, uint8_t *hdelta, std::vector<RowOverflow> &overflow) {
	if (p.t1 <= p.t0 || s.pack_work == 0) return;
	std::vector<uint64_t> wp((size_t) (p.t1 - p.t0) + 1);
	for (int i = p.t0; i <= p.t1; ++i) wp[(size_t) (i - p.t0)] = L.wprefix[(size_t) i] - L.wprefix[(size_t) p.t0];
	const int base = p.t0;
	const size_t first = overflow.size();
	overflow.resize(first + (size_t) s.threads + 1);
	std::atomic<int> slot(0);
	parallel_ranges(p.t1 - p.t0, wp, s.threads, [&](int bg, int en) {
		upload_pack(base + bg, base + en, tiles, tin, hseq, hdelta, L.rsrc, overflow[first + (size_t) slot.fetch_add(1)], !s.zc_qry && !L.segments, !s.zc_ref && !L.windows);
	});
}

/* ------------------------------------------------------------------ host planning */

struct HostPlan {
	std::vector<TileRun> trun;
	std::vector<TileOut> tout;
	std::vector<std::vector<int32_t>> cls;   /* work list per kernel class x {float runs, int16 runs} */
	std::vector<int32_t> generic;            /* tiles of the catch-all kernel */
	/* chained tiles (row blocks): per chain class x {float runs, int16 runs} the tasks in launch
	 * order, the tiles, and the per-block tables shared by all classes */
	std::vector<std::vector<ChainTask>> chain_tasks;
	std::vector<std::vector<int32_t>> chain_tiles;
	std::vector<ChainBlk> chain_blk;
	uint64_t bnd_recs = 0;                   /* BoundaryRec entries */
	uint64_t dir_dwords = 0, ops_ints = 0, cells = 0, active = 0;
	int n_fast = 0;                          /* tiles taken whole by one wave */
	int n_chained = 0;
};

/* Row blocks of one chained tile: fills hp.chain_blk and returns the tile's tasks (block order).
 * rows = the tile's (offset, length) rows as uploaded. */
inline void plan_chain_tile(int tile, int m, const TilePlan &p, const TileIn &in, const RowDesc *rows,
		HostPlan &hp, TileRun &r, std::vector<ChainTask> &out) {
	const int N = 64 * m, H = in.H, W = in.W;
	const int nblk = (H + N - 1) / N;
	r.ring = N;
	r.r0 = p.r0;
	r.nsteps = p.rend - p.r0;
	r.dir_off = 0;
	r.mnw = m;
	r.chain_blk0 = (int32_t) hp.chain_blk.size();
	r.chain_nblk = nblk;
	auto span = [&](int y, long long &lo, long long &hi) {
		lo = rows[y].off > 0 ? rows[y].off : 0;
		hi = (long long) rows[y].off + (long long) rows[y].len;
		if (hi > W) hi = W;
		if (hi < lo) hi = lo;
	};
	uint64_t prev_out = 0;
	for (int g = 0; g < nblk; ++g) {
		const int y0 = g * N, y1 = std::min(H, y0 + N);
		long long gs_min = 0x7fffffff, ge_max = -0x7fffffff;
		for (int y = y0; y < y1; ++y) {
			long long lo, hi;
			span(y, lo, hi);
			if (hi > lo) { gs_min = std::min(gs_min, lo + y); ge_max = std::max(ge_max, hi + y); }
		}
		ChainTask t;
		memset(&t, 0, sizeof(t));
		t.tile = tile;
		t.y0 = y0;
		t.rows = y1 - y0;
		if (ge_max > gs_min) {
			/* planes of all blocks share the tile's bit phase: a block begins on a multiple of 32 steps behind the tile's first.
			 * A block below another begins at least ONE step before its first cell: the diagonal input of that cell -- the score
			 * of the row above one column to the left -- reaches the slot as the `up` score of the step before (round 5: a block
			 * whose first cell fell exactly on such a multiple took 0 for it; one block in 32, and visible only where the best
			 * path runs down the corridor's first column, i.e. in tiles validPath rejects -- found on the C5 mix, where the raw
			 * fill score of 6 of 4 096 chained tiles differed from the ring kernels' and the reference's) */
			const long long lead = g > 0 ? 1 : 0;
			t.r0 = p.r0 + (int) ((gs_min - lead - p.r0) & ~31ll);
			t.nsteps = (int) (ge_max - t.r0);
		} else {
			t.r0 = p.r0;
			t.nsteps = 0;
		}
		t.blk = r.chain_blk0 + g;
		t.prev = g > 0 ? t.blk - 1 : -1;
		if (g > 0) {
			long long lo, hi;
			span(y0 - 1, lo, hi);
			t.bnd_lo = (int32_t) lo;
			t.bnd_len = (int32_t) (hi - lo);
			t.bnd_in_off = prev_out;
		}
		t.has_next = (g + 1 < nblk) ? 1 : 0;
		{
			long long lo, hi;
			span(y1 - 1, lo, hi);
			t.bnd_out_off = hp.bnd_recs;
			prev_out = hp.bnd_recs;
			if (t.has_next) hp.bnd_recs += (uint64_t) (hi - lo);
		}
		const uint64_t nblk32 = (uint64_t) ((t.nsteps + 31) / 32);
		t.dir_off = hp.dir_dwords;
		ChainBlk cb;
		cb.dir_off = hp.dir_dwords / 2;
		cb.tblk0 = (t.r0 - p.r0) >> 5;
		cb.nblk32 = (int32_t) std::max<uint64_t>(nblk32, 1);
		hp.dir_dwords += std::max<uint64_t>(nblk32, 1) * (uint64_t) N * 2ull;
		hp.chain_blk.push_back(cb);
		out.push_back(t);
	}
}

/* Longest processing time first (most cells first, index as tie-break): the persistent waves
 * pull from the front.  Sorted as packed 64-bit keys when they fit (always, below a million
 * tiles of less than 2^43 cells), several times faster than comparing through the plan array. */
inline void lpt_sort(std::vector<int32_t> &v, const TilePlan *plan) {
	bool packed = v.size() < (1u << 20);
	if (packed) {
		std::vector<uint64_t> keys(v.size());
		for (size_t q = 0; q < v.size() && packed; ++q) {
			const uint64_t a = plan[(size_t) v[q]].active;
			if (a >= (1ull << 43) || (uint32_t) v[q] >= (1u << 20)) packed = false;
			keys[q] = (((1ull << 43) - 1 - a) << 20) | (uint64_t) (uint32_t) v[q];
		}
		if (packed) {
			std::sort(keys.begin(), keys.end());
			for (size_t q = 0; q < v.size(); ++q) v[q] = (int32_t) (keys[q] & ((1u << 20) - 1));
			return;
		}
	}
	std::sort(v.begin(), v.end(), [&](int32_t x, int32_t y) {
		const uint64_t ax = plan[(size_t) x].active, ay = plan[(size_t) y].active;
		return ax != ay ? ax > ay : x < y;
	});
}

/* Which forward fill a handle's scoring gets (cvx_create_ex).  The ring kernels implement the scalar recurrence and use its sign
 * structure: match > 0 > every penalty, extension never dearer than its floor (ring_signs).  A default handle must reproduce the
 * reference's SSE path, which equals that recurrence only while opening a gap directly off the other gap type can never win --
 * gap_open + gap_ext_min < mismatch (the 0.25 keeps float rounding out of the argument); any other scoring
 * goes to the catch-all kernel's SSE-variant instantiation.  A scalar-twin handle (CVX_CREATE_SCALAR_TWIN) reproduces
 * Convex::ConvexAlign, which runs the scalar recurrence for ANY scoring: it never takes the SSE variant; where the sign structure
 * holds it uses the rings' twin instantiations, otherwise the catch-all kernel with scalar rules.  Twin handles build no gang
 * classes (the twin form of the gang kernels is not instantiated): their corridors of 257-576 live rows are chained. */
struct FillSemantics {
	bool ring_signs;       /* the sign structure the ring kernels rely on holds */
	bool sse_variant;      /* every tile to fill_generic_kernel<SSE = true> */
	bool force_generic;    /* every tile to the catch-all kernel (either instantiation) */
	bool no_gangs;         /* the handle builds no gang classes, whatever CVX_TUNE_GANGS says */
	bool matrix_cap;       /* max_matrix_mb applies (the twin's AlignmentMatrix::prepare allocates whatever is asked) */
};
inline FillSemantics fill_semantics(const float match, const float mismatch, const float gap_open, const float gap_extend,
		const float gap_extend_min, const float gap_decay, const bool scalar_twin) {
	FillSemantics f;
	f.ring_signs = match > 0.0f && mismatch < 0.0f && gap_open < 0.0f && gap_extend < 0.0f && gap_extend_min < 0.0f &&
			gap_decay >= 0.0f && gap_extend <= gap_extend_min;
	const bool fast_regime = f.ring_signs && (gap_open + gap_extend_min) < mismatch - 0.25f;
	f.sse_variant = !scalar_twin && !fast_regime;
	f.force_generic = scalar_twin ? !f.ring_signs : !fast_regime;
	f.no_gangs = scalar_twin;
	f.matrix_cap = !scalar_twin;
	return f;
}
/* the twin's mismatch against an 'x' of the reference window: ONE binary32 multiply (src/ConvexAlign.cpp:513; the files that
 * include this are compiled with -ffp-contract=off and for a target that evaluates float expressions in binary32) */
inline float twin_mismatch_x(const float mismatch) {
	volatile float m = mismatch;
	volatile float r = m * 100.0f;
	return r;
}

/* The FAST ring fill (cvx_fill_ring.inc) runs on scores scaled by kScoreScale = 2^-64 so that the clamp bit of v_max3_f32 is the
 * zero clamp of a cell's maximum.  Scaling by a power of two commutes with binary32 +, max, negation and compares as long as
 * nothing overflows, underflows or goes subnormal.  That holds when every nonzero value the fill adds -- match, mismatch, the
 * twin's 'x' mismatch (pass 0 for a default handle), gap open and the kPenPairs penalties of the table -- is finite with a binary
 * exponent in [-kScoreExpMax, kScoreExpMax]: every score is then a multiple of 2^-43 (induction over the adds; rounding only
 * coarsens the grid), so a nonzero scaled score is at least 2^-107 in magnitude, which is normal, and the largest score, 2^20 a row
 * over 2^31 rows, scales to 2^-13 <= 1.  The penalties are computed with the operations of cvx_create's table check.  A scoring
 * that fails runs the arithmetic form (tune_pen_table = 0), which is unscaled. */
inline bool score_scale_value_ok(const float v) {
	if (v == 0.0f) return true;
	if (!std::isfinite(v)) return false;
	const int e = std::ilogb(v);      /* (a subnormal's is below -126) */
	return e >= -kScoreExpMax && e <= kScoreExpMax;
}
inline bool score_scale_exact(const float match, const float mismatch, const float mismatch_x, const float gap_open,
                              const float gap_extend, const float gap_extend_min, const float gap_decay) {
	if (!score_scale_value_ok(match) || !score_scale_value_ok(mismatch) || !score_scale_value_ok(mismatch_x) || !score_scale_value_ok(gap_open)) return false;
	for (int run = 0; run < kPenPairs; ++run) {
		volatile float prod = (float) run * gap_decay;
		volatile float sum = gap_extend + prod;
		volatile float pen = std::fmin(gap_extend_min, (float) sum);
		if (!score_scale_value_ok(pen)) return false;
	}
	return true;
}

/* Kernel class, arena offsets and (sorted) work lists of every tile from its corridor plan.
 * tune: the CVX_TUNE_* knobs of the runtime. */
/* tuning / test knobs of the runtime (CVX_TUNE_* environment variables; all 0 = off) */
struct PlanTuning {
	int min_slots = 0;     /* smallest M a whole tile may use */
	int max_slots = 0;     /* largest M a whole tile may use (wider tiles are chained) */
	int force_wrap = 0;    /* route every tile to the int16-run kernels */
	int chain_m = 0;       /* 1, 2 or 4: force the row-block height class of chained tiles */
	int force_generic = 0; /* every tile to the catch-all kernel (scoring that needs its SSE-variant instantiation) */
	int long_steps = 0;    /* > 0: replaces kLongTileSteps (a tile of a small batch with at least this many steps is chained) */
	int small_batch = 0;   /* > 0: replaces kSmallBatchTiles */
	int long_need = 0;     /* > 0: replaces the 128 live rows from which a very long tile of a small batch is chained */
	int no_gangs = 0;      /* != 0: no gang classes (corridors with more than 256 live rows are chained, as before round 5) */
};

/* rows_of(i, tmp) -> the (offset, length) rows of tile i (may fill and return tmp), or an empty function /
 * nullptr result when the host has none (then nothing is chained). */
template <typename RowsOf>
inline void host_plan_rows(int n, const TilePlan *plan, const TileIn *tin, RowsOf rows_of, bool have_rows, const PlanTuning &tune, HostPlan &hp);

inline void host_plan(int n, const TilePlan *plan, const TileIn *tin, const RowDesc *rows, const PlanTuning &tune, HostPlan &hp) {
	/* rows: one arena indexed by TileIn::row_off (tests), or NULL */
	host_plan_rows(n, plan, tin, [&](int i, std::vector<RowDesc> &) { return rows + tin[(size_t) i].row_off; }, rows != nullptr, tune, hp);
}

template <typename RowsOf>
inline void host_plan_rows(int n, const TilePlan *plan, const TileIn *tin, RowsOf rows_of, bool have_rows, const PlanTuning &tune, HostPlan &hp) {
	const int tune_min_slots = tune.min_slots, tune_force_wrap = tune.force_wrap;
	hp.trun.assign((size_t) n, TileRun());
	hp.tout.assign((size_t) n, TileOut());
	hp.cls.assign((size_t) kNumClasses * 2, std::vector<int32_t>());
	hp.generic.clear();
	hp.chain_tasks.assign((size_t) kNumChainClasses * 2, std::vector<ChainTask>());
	hp.chain_tiles.assign((size_t) kNumChainClasses * 2, std::vector<int32_t>());
	hp.chain_blk.clear();
	hp.bnd_recs = 0;
	hp.dir_dwords = hp.ops_ints = hp.cells = hp.active = 0;
	hp.n_fast = 0;
	hp.n_chained = 0;
	std::vector<std::vector<std::vector<ChainTask>>> per_tile((size_t) kNumChainClasses * 2);
	int n_work = 0;
	for (int i = 0; i < n; ++i) if (!(plan[(size_t) i].flags & (kPlanTooLarge | kPlanEmpty))) n_work++;
	const bool small_batch = n_work < (tune.small_batch > 0 ? tune.small_batch : kSmallBatchTiles);
	for (int i = 0; i < n; ++i) {
		const TilePlan &p = plan[(size_t) i];
		TileRun &r = hp.trun[(size_t) i];
		TileOut &o = hp.tout[(size_t) i];
		memset(&r, 0, sizeof(r));
		memset(&o, 0, sizeof(o));
		o.score = -1.0f;
		hp.cells += p.cells;
		r.skip = 1;
		if (p.flags & kPlanTooLarge) { o.status = CVX_TILE_TOO_LARGE; continue; }
		if (p.flags & kPlanEmpty) { o.status = CVX_TILE_EMPTY; continue; }
		const bool wrap = (p.flags & kPlanWrap16) || tune_force_wrap;
		const bool regular = !(p.flags & kPlanIrregular);
		int k = -1;
		if (regular && !tune.force_generic) {
			for (int c = 0; c < kNumClasses; ++c)
				if (kClasses[c].ring() >= p.need && kClasses[c].m >= tune_min_slots &&
						(tune.max_slots <= 0 || kClasses[c].m <= tune.max_slots) &&
						(kClasses[c].gang == 1 || (!wrap && !tune.no_gangs))) { k = c; break; }
		}
		r.skip = 0;
		r.chain_blk0 = -1;
		r.chain_nblk = 0;
		r.ops_cap = tin[(size_t) i].H + tin[(size_t) i].W + 8;
		r.ops_off = hp.ops_ints;
		hp.ops_ints += (uint64_t) r.ops_cap;
		hp.active += p.active;
		const bool long_tile = small_batch && p.need >= (tune.long_need > 0 ? tune.long_need : 128) && (p.rend - p.r0) >= (tune.long_steps > 0 ? tune.long_steps : kLongTileSteps);
		if ((k < 0 || long_tile) && regular && have_rows && tune_min_slots == 0 && !tune.force_generic) {
			/* more live rows than any ring (or one very long tile in a batch too small to fill the
			 * device with whole tiles): row blocks chained through boundary streams */
			int cc = chain_class_for(p.need, small_batch);
			for (int q = 0; q < kNumChainClasses; ++q) if (kChainClasses[q] == tune.chain_m) cc = q;
			const size_t slot = (size_t) cc * 2 + (wrap ? 1 : 0);
			per_tile[slot].emplace_back();
			std::vector<RowDesc> tmp_rows;
			plan_chain_tile(i, kChainClasses[cc], p, tin[(size_t) i], rows_of(i, tmp_rows), hp, r, per_tile[slot].back());
			hp.chain_tiles[slot].push_back(i);
			hp.n_chained++;
			continue;
		}
		int64_t ring;
		if (k < 0) {
			/* catch-all kernel, irregular row starts: one slot per row PLUS ONE: slot 0 reads its "up"
			 * neighbour from the last slot of the ring, which must therefore never hold a row -- with a
			 * ring of exactly H slots row 0 would see row H-1's live cells instead of the empty element
			 * (getElement(x, -1), src/AlignmentMatrixFast.h:74-111) */
			const int64_t want = regular ? (int64_t) p.need : (int64_t) tin[(size_t) i].H + 1;
			ring = ((want > 0 ? want : 1) + 63) / 64 * 64;
			const uint64_t dd = (uint64_t) ((p.rend - p.r0 + 31) / 32) * (uint64_t) ring * 2ull;
			if (ring > (1 << 30) || dd > (4ull << 30)) {     /* > 16 GiB of codes for one irregular tile */
				o.status = CVX_TILE_UNSUPPORTED;
				r.skip = 1;
				hp.active -= p.active;
				continue;
			}
		} else {
			ring = kClasses[k].ring();
		}
		r.ring = (int32_t) ring;
		r.r0 = p.r0;
		r.nsteps = p.rend - p.r0;
		r.dir_off = hp.dir_dwords;
		hp.dir_dwords += (uint64_t) ((r.nsteps + 31) / 32) * (uint64_t) r.ring * 2ull;
		r.mnw = k < 0 ? 0 : kClasses[k].m;
		if (k < 0) { hp.generic.push_back(i); continue; }
		hp.n_fast++;
		hp.cls[(size_t) k * 2 + (wrap ? 1 : 0)].push_back(i);
	}
	/* chain tasks in launch order: block index major, tile minor -- a wave takes tasks in this order,
	 * so all tiles advance together and the block above any task has always been taken before it */
	for (size_t slot = 0; slot < per_tile.size(); ++slot) {
		size_t deepest = 0;
		for (auto &v : per_tile[slot]) deepest = std::max(deepest, v.size());
		for (size_t g = 0; g < deepest; ++g)
			for (auto &v : per_tile[slot])
				if (g < v.size()) hp.chain_tasks[slot].push_back(v[g]);
	}
	for (auto &v : hp.cls) lpt_sort(v, plan);
}

/* ------------------------------------------------------------------ the compute stage's launch schedule */

/* What stage_compute (cvx_rt_align.cpp) queues for a planned batch, decided here so that the CPU suite can check it: the
 * contents of the work lists, one record per fill launch in launch order, the layout of the chain upload and the lanes of
 * every backtrack walk.  The stage itself only issues what the schedule says. */

/* the knobs of the handle that shape the schedule (cvx_context, CVX_TUNE_*) */
struct ScheduleTuning {
	int exact_steps = kExactDirectSteps;
	int bt_group = 0;
	bool bt_per_class = true;
	bool overlap_post = false;
	int wide_prio = 1, gang_prio = 0, chain_prio = -1, chain_lds_kb = 48;
	/* the tail split of a whole-tile class (tail_split below): 0 = none; N > 0 = the last N tiles of every whole-tile class with more
	 * than N two-phase tiles; kTailAuto = tail_rounds resident rounds of the class, where the class and the batch are large enough */
	int tail_tiles = 0;
	float tail_rounds = 1.0f;
	int tail_waves_per_simd[kNumClasses * 2] = {0};      /* kTailAuto: resident waves per SIMD of each class's two-phase fill (HostPlan::cls index; 0 = unknown, no split) */
};

enum { kTailAuto = -1 };
/* kTailAuto splits a class of at least this many resident rounds, in a batch that walks at least this many tiles (where the walk is issue-bound) */
static const int kTailMinRounds = 4;
static const int kTailMinWalk = 4096;

/* Tiles at the end of a whole-tile class's list (`two_phase` = count - n_direct entries behind its direct-exact prefix) that are filled
 * by a launch of their own on the handle's low-priority stream (stage_compute): the class's shortest tiles, the ones dispatched
 * last anyway.  One wave fills one tile, so from the moment a launch has nothing left to dispatch its resident waves retire over
 * the length of a tile and the device runs from full to empty; with the last round split off, the head of the class is walked in the
 * issue slots that the draining tail leaves free.  0 = no split: either part would be empty, the class is a gang, or -- kTailAuto --
 * the class would not fill the device kTailMinRounds times over or the batch's walk is not issue-bound. */
inline int tail_split(const ScheduleTuning &t, int cls, int gang, int two_phase, int n_walk, int num_cus) {
	if (t.tail_tiles == 0 || gang > 1 || t.overlap_post || !t.bt_per_class) return 0;
	int tail = t.tail_tiles;
	if (t.tail_tiles == kTailAuto) {
		const int64_t resident = (int64_t) num_cus * 4 * (int64_t) t.tail_waves_per_simd[cls];
		if (resident <= 0 || (int64_t) two_phase < kTailMinRounds * resident || n_walk < kTailMinWalk) return 0;
		tail = (int) ((double) t.tail_rounds * (double) resident + 0.5);
	}
	return (tail > 0 && tail < two_phase) ? tail : 0;
}

/* launch_fill's `mode` (= FillMode of cvx_kernels.hip) */
enum { kModeTwoPhase = 0, kModeExact = 1, kModeChain = 2 };

/* the streams a fill launch may ride on: the first side stream, `post`, `main`, the second side stream */
enum StreamSlot { kOnSide0 = 0, kOnPost = 1, kOnMain = 2, kOnSide1 = 3, kStreamSlots = 4 };

/* lanes of one backtrack walk: the first n_long tiles of the list at long_lanes per tile, the rest at bulk_lanes */
struct WalkPlan { int n_long = 0, long_lanes = 32, bulk_lanes = 64; };

/* the walk of list[0, count) (longest read first).  Few tiles in the batch: the walk is latency-bound and
 * 64 probing lanes per tile take the long diagonal runs in a quarter of the probes; many tiles: it is issue-bound and
 * several tiles share a wave -- eight for the bulk; the few reads much longer than the rest (a latency-bound tail, a
 * serial chain of H / 7 probes each) get 32 lanes per tile, beside the bulk on a side stream when the walk is one walk for the
 * whole batch, in front of it on the same stream otherwise (measured: PacBio 5.4 -> 4.9 ms with 8 lanes, ONT mix 8.2 -> 6.6 with 32).
 * bt_group: cvx_context::bt_group; n_walk: tiles of all walks of the batch; mean_h: mean read rows per tile of the batch. */
inline WalkPlan walk_plan(int count, int n_walk, int bt_group, uint64_t mean_h, const int32_t *list, const TileIn *tin) {
	/* Lanes per tile by the number of tiles walked together (round 5): a walk is a serial chain of probes per tile, and
	 * what hides a probe's latency is other waves -- so few tiles get many lanes each (a probe then covers 64 / 32 / 16
	 * path columns of a diagonal run instead of 8) until the walk has about six waves per SIMD, and only beyond that
	 * is it issue-bound and eight lanes per tile the cheapest.  Measured against round 4's rule (one wave per tile below
	 * 4 096 tiles, eight lanes from there on): C5 mix, 4 096 tiles of 100 kb, walk 39.5 ms at 8 lanes = 512 waves on 1 024
	 * SIMDs, 25.9 at 16, 21.6 at 32, 19.4 at 64; ONT mix at 49 152 tiles in one walk 7.6 ms at 8, 6.0 at 16; the PacBio
	 * bench (49 152 tiles): the walk alone 7.7 ms at 8 and 8.4 at 16, the pipelined step 114.4-114.9 against 113.9-114.1 ms
	 * (profiles/r05_ab_bt_group.txt). */
	const int auto_group = count <= 6144 ? 64 : count <= 12288 ? 32 : count <= 49152 ? 16 : 8;
	WalkPlan w;
	/*   bt_group   > 0: that many lanes for all        -1: 64 below 4 096 tiles in the batch, else 8        0: by count */
	w.bulk_lanes = bt_group > 0 ? bt_group : bt_group < 0 ? (n_walk < 4096 ? 64 : 8) : auto_group;
	/* a bulk at 8 or 16 lanes (never a forced group): the much-longer-than-average reads at its head at 32 */
	if (bt_group <= 0 && w.bulk_lanes <= 16)
		while (w.n_long < count && (uint64_t) tin[(size_t) list[w.n_long]].H > 3 * mean_h) w.n_long++;
	return w;
}

/* Dynamic LDS that caps the residency of a chained class: tasks are dispatched in order, long before their turn;
 * resident tasks beyond the ones that can actually run only poll.  Unused dynamic LDS caps the residency at ~1.5x
 * the blocks that are live at one time (`live` = need / rows-per-block per tile, + slack). */
inline size_t chain_pad_lds(uint64_t live, int num_cus, int chain_lds_kb, bool rings_beside) {
	const uint64_t resident = std::min<uint64_t>(8192, std::max<uint64_t>(768, live + live / 2 + 256));
	const size_t per_cu = (size_t) ((resident + (uint64_t) num_cus - 1) / (uint64_t) num_cus);
	size_t pad_lds = per_cu >= 32 ? 0 : (size_t) (160 * 1024) / per_cu - 4096;
	pad_lds = std::min<size_t>(pad_lds, 60 * 1024) / 256 * 256;
	/* The padding is LDS the ring classes of the same batch cannot use: a handful of chained retries among a thousand whole
	 * tiles (ngmlr's own launches: 10-40 chained tiles, resident = 768 tasks = 3 per CU at 50 KB each) held 150 of a CU's
	 * 160 KB for their 7 ms, and the M = 3 / M = 4 classes -- 4-5 KB per wave -- crawled until they were gone: a launch's
	 * fill was the SUM of the chained class and the widest ring class (18.6 = 7.0 + 11.7 ms, profiles/r06_e2e_launch_trace.txt).
	 * Beside ring classes the cap may hold chain_lds_kb per CU; more tasks than can run then sit in their back-off sleep. */
	if (rings_beside && chain_lds_kb > 0 && per_cu > 0 && per_cu < 32) {
		const size_t budget = (size_t) chain_lds_kb * 1024 / per_cu;
		const size_t capped = budget > 4096 ? (budget - 4096) / 256 * 256 : 0;
		pad_lds = std::min(pad_lds, capped);
	}
	return pad_lds;
}

/* one forward-fill launch: a chained class (row-block tasks + the per-tile reduction), a whole-tile class (the direct-exact
 * prefix, the two-phase pass, the exact redo pass) or the catch-all kernel */
struct FillLaunch {
	int kind = 0;                    /* CVX_LAUNCH_* */
	int m = 0, gang = 1, wrap = 0;   /* (the catch-all kernel: 0, 16, 1 -- what its cvx_launch_info has always said) */
	int slot = 0;                    /* index into HostPlan::chain_tasks (chained) or HostPlan::cls (whole tiles) */
	const std::vector<int32_t> *tiles = nullptr;   /* the launch's tiles (in the HostPlan) */
	size_t list_off = 0;             /* whole tiles, catch-all: lists[list_off, + count), the first n_direct straight to the exact fill */
	int n_direct = 0, count = 0;     /* (chained: count = row-block tasks) */
	size_t pad_lds = 0;              /* chained: chain_pad_lds */
	int prio = 0;                    /* FillArgs::chain_prio: the chain priority, the widest ring class's or the gangs' */
	int stream = kOnMain;            /* StreamSlot */
	/* whole tiles only, > 0: the launch is issued as two fills -- the head lists[list_off, + count - tail_count), which keeps the direct-exact
	 * prefix, on `stream`, and the tail, the last tail_count entries of the same list, on the handle's low-priority stream (tail_split) */
	int tail_count = 0;
	size_t bt_off = 0;               /* the launch's backtrack segment: lists[bt_off, + bt_count) */
	int bt_count = 0;
	int bt_tail_count = 0;           /* a split launch: the segment holds the head's tiles, then, from bt_count - bt_tail_count on, the tail's, each part longest read first */
	WalkPlan walk;                   /* of that segment, of its head part when the launch is split (per_class only) */
	WalkPlan walk_tail;              /* of the tail part */
	cvx_launch_info info;
};

struct ComputeSchedule {
	std::vector<FillLaunch> launches;      /* in launch order: chained classes, whole-tile classes from the widest ring down, the catch-all kernel */
	size_t n_listed = 0;                   /* entries of `lists`: fill lists, then the backtrack segments from bt_begin on */
	size_t bt_begin = 0;
	int n_walk = 0;                        /* tiles of all backtrack segments */
	bool per_class = false;                /* every launch walks its own segment behind its fill (always so when a launch is split); else one walk (`walk`) behind all fills */
	WalkPlan walk;
	/* chained tiles: tasks of every chain class, block table and tile lists in one upload */
	size_t chain_task_off[kNumChainClasses * 2] = {0}, chain_tile_off[kNumChainClasses * 2] = {0};
	size_t chain_blk_off = 0, chain_bytes = 0;
};

/* hp: of host_plan_rows (the direct-exact tiles move to the front of their class and get kPadRedo in hp.tout);
 * lists: room for 2 n entries; n_rows: read rows of all n tiles. */
inline void build_schedule(HostPlan &hp, const TilePlan *plan, const TileIn *tin, int n, uint64_t n_rows, int num_cus,
		const ScheduleTuning &t, int32_t *lists, ComputeSchedule &s) {
	size_t n_listed = 0;
	size_t cls_off[kNumClasses * 2];
	int n_direct[kNumClasses * 2];
	int ring_classes = 0;
	/* Very long tiles go straight to the exact-tracking instantiation.  The two-phase pass saves three half-rate ops per
	 * cell (~12 %) but a tile whose best cell is not in its last anti-diagonals -- a local alignment: an inverted segment,
	 * a read that does not reach its end -- is redone from step 0, and for a 100 kb tile that second pass is another
	 * ~100 ms on one wave behind everything else (C5 mix: 77 ms of a 200 ms fill).  Tiles of kExactDirectSteps steps and
	 * more are flagged kPadRedo up front and listed first; the exact launch over that prefix does them once.  Only while
	 * the class cannot fill the device several times over (then 12 % of throughput would cost more than the tail). */
	for (size_t c = 0; c < hp.cls.size(); ++c) {
		std::vector<int32_t> &v = hp.cls[c];      /* already in LPT order */
		cls_off[c] = n_listed;
		n_direct[c] = 0;
		if (v.empty()) continue;
		ring_classes++;
		auto direct = [&](int32_t ti) { return hp.trun[(size_t) ti].nsteps >= t.exact_steps; };
		const int nl = t.exact_steps > 0 ? (int) std::count_if(v.begin(), v.end(), direct) : 0;
		if (nl > 0 && nl <= kExactDirectMaxTiles) {
			std::stable_partition(v.begin(), v.end(), direct);
			for (int q = 0; q < nl; ++q) hp.tout[(size_t) v[(size_t) q]].pad = kPadRedo;
			n_direct[c] = nl;
		}
		memcpy(lists + n_listed, v.data(), v.size() * sizeof(int32_t));
		n_listed += v.size();
	}
	/* (every computed tile is walked: what the backtrack segments will hold) */
	int n_computed = 0;
	for (int i = 0; i < n; ++i) if (!hp.trun[(size_t) i].skip) n_computed++;
	const size_t generic_begin = n_listed;
	if (!hp.generic.empty()) memcpy(lists + n_listed, hp.generic.data(), hp.generic.size() * sizeof(int32_t));
	n_listed += hp.generic.size();

	/* forward fill: one launch per populated kernel class (+ its exact redo pass), classes run
	 * concurrently on separate streams (a sparsely populated class would otherwise serialise a
	 * whole tile latency behind the big one); widest rings first, they have the longest tiles */
	s.launches.clear();
	s.launches.reserve((size_t) (kNumChainClasses + kNumClasses) * 2 + 1);
	/* chained tiles first (their dependency chains are the longest thing in a batch): the row-block
	 * tasks of a class, then the per-tile reduction of the block results */
	for (size_t c = 0; c < hp.chain_tasks.size(); ++c) {
		if (hp.chain_tasks[c].empty()) continue;
		FillLaunch L;
		L.kind = CVX_LAUNCH_CHAINED;
		L.m = kChainClasses[c / 2]; L.wrap = (int) (c & 1); L.slot = (int) c;
		L.tiles = &hp.chain_tiles[c];
		L.count = (int) hp.chain_tasks[c].size();
		L.prio = t.chain_prio >= 0 ? t.chain_prio : 1;
		uint64_t live = 0;
		for (int32_t ti : hp.chain_tiles[c]) live += (uint64_t) plan[(size_t) ti].need / (uint64_t) (64 * L.m + kChainChunk) + 2;
		L.pad_lds = chain_pad_lds(live, num_cus, t.chain_lds_kb, ring_classes > 0);
		s.launches.push_back(L);
	}
	bool widest = true;
	for (int cc = (int) hp.cls.size() - 1; cc >= 0; --cc) {
		const size_t c = (size_t) cc;
		if (hp.cls[c].empty()) continue;
		const KernelClass &kc = kClasses[c / 2];
		FillLaunch L;
		L.kind = kc.gang > 1 ? CVX_LAUNCH_GANG : CVX_LAUNCH_WHOLE;
		L.m = kc.m; L.gang = kc.gang; L.wrap = (int) (c & 1); L.slot = cc;
		L.tiles = &hp.cls[c];
		L.list_off = cls_off[c]; L.n_direct = n_direct[c]; L.count = (int) hp.cls[c].size();
		/* (the widest ring class of a batch of several one priority notch up; gangs have a knob of their own) */
		L.prio = kc.gang > 1 ? t.gang_prio : (widest && ring_classes > 1) ? t.wide_prio : 0;
		widest = false;
		L.tail_count = tail_split(t, cc, kc.gang, L.count - L.n_direct, n_computed, num_cus);
		s.launches.push_back(L);
	}
	if (!hp.generic.empty()) {
		FillLaunch L;
		L.kind = CVX_LAUNCH_CATCH_ALL;
		L.m = 0; L.gang = 16; L.wrap = 1;
		L.tiles = &hp.generic;
		L.list_off = generic_begin; L.count = (int) hp.generic.size();
		s.launches.push_back(L);
	}

	/* fill launches go round-robin over the side streams, `post` and the main stream itself (which has
	 * nothing else to do until they are all done): classes side by side */
	/* (the `post` stream carries a fill class too unless the post-fill overlap experiment owns it) */
	/* (order: first side stream, post, main -- the assignment of rounds 2-4 for up to three classes -- and the second side stream
	 * only for a fourth class, i.e. with gangs.  Which class rides on which stream is not neutral: with the three whole-tile
	 * classes of the C5 mix on side / side / post instead of side / post / main the same batch takes 181 or 236 ms depending on the
	 * handle, on side / post / main 194 every time: profiles/r05_fill_stream_order.txt) */
	int order[kStreamSlots], n_order = 0;
	for (int sl = 0; sl < kStreamSlots; ++sl) if (sl != kOnPost || !t.overlap_post) order[n_order++] = sl;
	/* behind the fill lists: every computed tile once, longest read first (counting sort on H / 32) --
	 * the order in which the backtrack takes them, four to a wave: the walk of a tile is a serial
	 * chain of ~H / 7 probes, so the long ones must start first and share their wave with their like.
	 * One segment per fill launch, in launch order: a batch of several classes walks each class right behind its own fill,
	 * on that fill's stream, while the other classes still fill; a batch of one class has one segment = the whole list. */
	s.bt_begin = n_listed;
	constexpr int kBuckets = 4096;
	auto bucket = [&](int32_t ti) { const int k = tin[(size_t) ti].H >> 5; return kBuckets - 1 - (k < kBuckets ? k : kBuckets - 1); };
	std::vector<int32_t> count((size_t) kBuckets + 1);
	bool any_split = false;
	for (size_t i = 0; i < s.launches.size(); ++i) {
		FillLaunch &L = s.launches[i];
		L.stream = order[i % (size_t) n_order];
		memset(&L.info, 0, sizeof(L.info));
		L.info.slots_per_lane = L.m; L.info.wrap16 = L.wrap; L.info.n_tiles = (int) L.tiles->size(); L.info.kind = L.kind;
		L.info.waves = L.kind == CVX_LAUNCH_CHAINED ? L.count : L.gang;      /* row-block tasks / waves per tile (a gang's size) */
		for (int32_t ti : *L.tiles) {
			const TilePlan &p = plan[(size_t) ti];
			const TileIn &in = tin[(size_t) ti];
			L.info.cells += p.cells; L.info.active_cells += p.active;
			L.info.alg_bytes += p.cells + 6ull * (uint64_t) in.H + 2ull * (uint64_t) in.W;
			L.info.read_bases += (uint64_t) in.H;
		}
		L.bt_off = n_listed;
		/* (a split launch: the head's tiles, then the tail's -- the two parts are walked one after the other) */
		const size_t n_head = L.tiles->size() - (size_t) L.tail_count;
		for (int part = 0; part < (L.tail_count > 0 ? 2 : 1); ++part) {
			const int32_t *tb = L.tiles->data() + (part ? n_head : 0), *te = L.tiles->data() + (part ? L.tiles->size() : n_head);
			std::fill(count.begin(), count.end(), 0);
			for (const int32_t *q = tb; q < te; ++q) if (!hp.trun[(size_t) *q].skip) count[(size_t) bucket(*q) + 1]++;
			for (int k = 0; k < kBuckets; ++k) count[(size_t) k + 1] += count[(size_t) k];
			const int part_count = count[(size_t) kBuckets];
			/* (stable: inside a bucket of equally long reads the class's own order, most cells first) */
			for (const int32_t *q = tb; q < te; ++q) if (!hp.trun[(size_t) *q].skip) lists[n_listed + (size_t) count[(size_t) bucket(*q)]++] = *q;
			n_listed += (size_t) part_count;
			if (part) L.bt_tail_count = part_count;
		}
		L.bt_count = (int) (n_listed - L.bt_off);
		any_split = any_split || L.tail_count > 0;
	}
	s.n_listed = n_listed;
	s.n_walk = (int) (n_listed - s.bt_begin);

	/* Several fill classes (ONT mix: chained retries, M = 4, M = 3; C5): each class is walked right behind its own fill on
	 * that fill's stream.  The launch of such a batch lasts as long as its longest dependency chain, and while the last
	 * chains finish on a few waves the device has issue slots to spare: the other classes' walks run there instead of
	 * behind everything (CVX_TUNE_BT_PER_CLASS=0: one walk behind all fills, as a batch of one class has it anyway). */
	/* Only where the walk is issue-bound (>= 4096 tiles; measured, r04c: ONT mix 60 000 tiles 57.2 -> 56.0 ms, 24 000 tiles
	 * 35.3 -> 34.2, C5 mix 6 144 tiles 397 -> 369 ms); a small batch's one-wave-per-tile walks are latency-bound chains that
	 * gain nothing from starting early and cost the fills still running (C5 mix 2 048 tiles: 183.6 -> 187.2 ms). */
	/* A schedule with a split launch walks per launch whatever its size: the head of the split class behind the head's fill, the tail
	 * behind the tail's, each part with the lanes its own count gives it. */
	s.per_class = (t.bt_per_class && s.launches.size() > 1 && !t.overlap_post && s.n_walk >= 4096) || any_split;
	const uint64_t mean_h = n_rows / (uint64_t) std::max(n, 1);
	if (s.per_class) for (FillLaunch &L : s.launches) {
		const int n_head = L.bt_count - L.bt_tail_count;
		L.walk = walk_plan(n_head, s.n_walk, t.bt_group, mean_h, lists + L.bt_off, tin);
		if (L.bt_tail_count > 0) L.walk_tail = walk_plan(L.bt_tail_count, s.n_walk, t.bt_group, mean_h, lists + L.bt_off + (size_t) n_head, tin);
	}
	else s.walk = walk_plan(s.n_walk, s.n_walk, t.bt_group, mean_h, lists + s.bt_begin, tin);

	s.chain_blk_off = s.chain_bytes = 0;
	if (hp.n_chained) {
		for (size_t c = 0; c < hp.chain_tasks.size(); ++c) { s.chain_task_off[c] = s.chain_bytes; s.chain_bytes += hp.chain_tasks[c].size() * sizeof(ChainTask); }
		s.chain_blk_off = s.chain_bytes; s.chain_bytes += hp.chain_blk.size() * sizeof(ChainBlk);
		for (size_t c = 0; c < hp.chain_tiles.size(); ++c) { s.chain_tile_off[c] = s.chain_bytes; s.chain_bytes += (hp.chain_tiles[c].size() * sizeof(int32_t) + 7) / 8 * 8; }
	}
}

}  // namespace cvx

#endif
