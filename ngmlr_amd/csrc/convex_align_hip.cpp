/*
 * convex_align_hip.cpp -- see convex_align_hip.h.  Host-only C++; all device work is
 * behind include/cvx_align.h.  No CPU alignment path exists here: if the device
 * library reports an error the call throws, exactly like a hard error in the reference.
 */
#include "convex_align_hip.h"
#include "cvx_fiber.h"
#include "nm_regions_note.h"
#include "inv_checks_binding_logic.h"

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <unordered_map>

#ifdef CVX_IN_NGMLR_TREE
#include "IConfig.h"       /* Config.getMaxMatrixSizeMB(), as ConvexAlignFast's ctor reads it (src/ConvexAlignFast.cpp:49) */
#endif

namespace Convex {

namespace {
std::atomic<long> g_prepared(0), g_closedForm(0);
bool const g_fitCorridors = [] { const char * e = getenv("CVX_CORRIDOR_FIT"); return !(e && atoi(e) == 0); }();
}

/* ------------------------------------------------------------------ DeviceWindows */
namespace {
struct WindowNote { char const * buf; unsigned long long position; long length; };
thread_local WindowNote tl_window = { 0, 0, 0 };
void const * g_binRef = 0;
unsigned long long g_nNibbles = 0;
std::vector<uint64_t> g_startTable;
std::atomic<long> g_windowLaunches(0), g_windowTiles(0), g_mixedLaunches(0);
/* on wherever the binding announced a genome (DeviceWindows::SetGenome: only oracle/_ref/ngmlr_hip_all carries it); CVX_DEVICE_DECODE=0 keeps
 * the reference's decode on the worker's core */
bool const g_deviceDecode = [] { const char * e = getenv("CVX_DEVICE_DECODE"); return !(e && atoi(e) == 0); }();
}

bool DeviceWindows::Enabled() { return g_deviceDecode; }
bool DeviceWindows::HaveGenome() { return g_binRef != 0; }
bool DeviceWindows::Genome(void const * & binRef, unsigned long long & nNibbles, unsigned long long const * & startTable, int & nStarts) {
	if (g_binRef == 0) return false;
	binRef = g_binRef;
	nNibbles = g_nNibbles;
	startTable = (unsigned long long const *) g_startTable.data();
	nStarts = (int) g_startTable.size();
	return true;
}

void DeviceWindows::SetGenome(void const * binRef, unsigned long long nNibbles, unsigned long long const * startTable, int nStarts) {
	g_startTable.assign(startTable, startTable + (nStarts > 0 ? nStarts : 0));
	g_nNibbles = nNibbles;
	g_binRef = binRef;
}

void DeviceWindows::Placeholder(char * buf, unsigned long long position, int length) {
	memset(buf, 'x', (size_t) (length - 1));      /* what the reference's decode starts from (src/SequenceProvider.cpp:501) */
	buf[length - 1] = '\0';
	if (Fiber * const f = FiberApi::Current()) {
		/* slots 1-3 of the read's context (0 is the dispatcher: batching_aligner.cpp) */
		FiberApi::Local(f, 1) = buf;
		FiberApi::Local(f, 2) = reinterpret_cast<void *>((uintptr_t) position);
		FiberApi::Local(f, 3) = reinterpret_cast<void *>((uintptr_t) length);
	} else {
		tl_window.buf = buf; tl_window.position = position; tl_window.length = length;
	}
}

bool DeviceWindows::Lookup(char const * buf, unsigned long long & position, int & length) {
	if (buf == 0) return false;
	if (Fiber * const f = FiberApi::Current()) {
		if (FiberApi::Local(f, 1) != buf) return false;
		position = (unsigned long long) reinterpret_cast<uintptr_t>(FiberApi::Local(f, 2));
		length = (int) reinterpret_cast<uintptr_t>(FiberApi::Local(f, 3));
		return true;
	}
	if (tl_window.buf != buf) return false;
	position = tl_window.position;
	length = (int) tl_window.length;
	return true;
}

/* ------------------------------------------------------------------ DeviceReads */
namespace {
/* what lies behind a placeholder's NUL: the note itself.  The buffer describes itself -- no table, no calling context, nothing
 * that outlives the buffer or can be overwritten by a later note. */
struct ReadNote {
	uint64_t magic;
	char const * self;      /* the buffer the note was written into: a byte copy of it elsewhere is not a note */
	char const * seq;
	int32_t readLen, start, len, flags;
};
uint64_t const kReadNoteMagic = 0x43565852534547A5ull;
/* placeholder character k: bit 7 set (no read character has it), never NUL, different from its neighbours */
inline char noteChar(int k) { return (char) (0x80 | ((k * 37 + 11) & 0x7F)); }
std::atomic<long> g_notedLaunches(0), g_notedTiles(0), g_mixedReadLaunches(0);
bool const g_deviceReads = [] { const char * e = getenv("CVX_DEVICE_READS"); return !(e && atoi(e) == 0); }();
/* the bytes [off, off + n) of a note's string, the way extractReadSeq builds them (cvx_stage_segments_host) */
bool readString(char const * seq, int readLen, int start, int len, int flags, int off, int n, char * out) {
	uint64_t const offsets[2] = { 0, (uint64_t) readLen + 1 };      /* (Seq carries its NUL) */
	/* a piece of a forward string is a later piece of the read, a piece of a reverse-complemented one an earlier piece */
	cvx_read_segment const s = { 0, (flags & CVX_SEG_REVCOMP) ? start + len - off - n : start + off, flags, 0 };
	int32_t const l = n;
	uint64_t at = 0, used = 0;
	return cvx_stage_segments_host(1, (uint8_t const *) seq, offsets, 1, &s, &l, (uint8_t *) out, (uint64_t) n, &at, &used) == CVX_OK;
}
bool readNote(char const * buf, ReadNote & note) {
	if (buf == 0) return false;
	int k = 0;
	while (buf[k] != '\0') { if (buf[k] != noteChar(k)) return false; ++k; }      /* a string of anything else ends the walk at its first character */
	if (k == 0) return false;
	memcpy(&note, buf + k + 1, sizeof(note));
	return note.magic == kReadNoteMagic && note.self == buf && note.len == k;
}
}

bool DeviceReads::Enabled() { return g_deviceReads; }
int DeviceReads::BufferBytes(int length) { return length + 1 + (int) sizeof(ReadNote); }

void DeviceReads::Placeholder(char * buf, char const * readSeq, int readLength, int start, int length, int flags) {
	for (int k = 0; k < length; ++k) buf[k] = noteChar(k);
	buf[length] = '\0';
	ReadNote note;
	memset(&note, 0, sizeof(note));
	note.magic = kReadNoteMagic; note.self = buf; note.seq = readSeq;
	note.readLen = readLength; note.start = start; note.len = length; note.flags = flags;
	memcpy(buf + length + 1, &note, sizeof(note));
}

bool DeviceReads::Lookup(char const * buf, char const * & readSeq, int & readLength, int & start, int & length, int & flags) {
	ReadNote note;
	if (!readNote(buf, note)) return false;
	readSeq = note.seq; readLength = note.readLen; start = note.start; length = note.len; flags = note.flags;
	return true;
}

bool DeviceReads::Materialise(char * buf) {
	ReadNote note;
	if (!readNote(buf, note)) return false;
	if (!readString(note.seq, note.readLen, note.start, note.len, note.flags, 0, note.len, buf)) { fprintf(stderr, "ConvexAlignHip: %s\n", cvx_last_error()); throw 1; }
	return true;      /* the buffer holds characters now: Lookup no longer takes it for a placeholder */
}

void DeviceReads::CopyOut(char * dst, char const * src, int offset, int n) {
	ReadNote note;
	if (!readNote(src, note)) { strncpy(dst, src + offset, (size_t) n); return; }
	if (offset < 0 || n < 0 || offset + n > note.len || !readString(note.seq, note.readLen, note.start, note.len, note.flags, offset, n, dst)) {
		fprintf(stderr, "ConvexAlignHip: DeviceReads::CopyOut of [%d, %d) from a query of %d characters\n", offset, offset + n, note.len);
		throw 1;
	}
}

/* ------------------------------------------------------------------ DeviceRegions */
namespace {
std::atomic<bool> g_regionsAnnounced(false);
std::atomic<long> g_noteAlignments(0), g_noteRegions(0), g_profileAlignments(0);
bool const g_deviceRegions = [] { const char * e = getenv("CVX_DEVICE_REGIONS"); return !(e && atoi(e) == 0); }();
/* (DeviceInvChecks, below: on only where the regions are) */
bool const g_deviceInvChecks = [] { const char * e = getenv("CVX_DEVICE_INV_CHECKS"); return !(e && atoi(e) == 0); }();
bool const g_invChecksVerify = [] { const char * e = getenv("CVX_INV_CHECKS_VERIFY"); return e && atoi(e) != 0; }();
bool const g_jobText = [] { const char * e = getenv("CVX_JOB_TEXT"); return e && atoi(e) != 0; }();
std::atomic<long> g_textFromDevice(0), g_textOnHost(0);
}

void DeviceRegions::Announce() { g_regionsAnnounced.store(true); }
bool DeviceRegions::Enabled() { return g_deviceRegions && g_regionsAnnounced.load(); }
bool DeviceRegions::JobText() { return g_jobText && Enabled(); }
void DeviceRegions::CountNote(int regions) {
	g_noteAlignments.fetch_add(1, std::memory_order_relaxed);
	g_noteRegions.fetch_add(regions, std::memory_order_relaxed);
}
void DeviceRegions::CountProfile() { g_profileAlignments.fetch_add(1, std::memory_order_relaxed); }
void DeviceRegions::Stats(long & noteAlignments, long & noteRegions, long & profileAlignments) {
	noteAlignments = g_noteAlignments.load();
	noteRegions = g_noteRegions.load();
	profileAlignments = g_profileAlignments.load();
}

/* ------------------------------------------------------------------ DeviceInvChecks */
namespace {
static_assert((int) kInvCheckScored == (int) CVX_CHECK_SCORED && (int) kInvCheckTooShort == (int) CVX_CHECK_TOO_SHORT &&
		(int) kInvCheckNoRead == (int) CVX_CHECK_NO_READ && (int) kInvCheckNoWindow == (int) CVX_CHECK_NO_WINDOW, "the binding's logic reads cvx_inv_check's status");
static_assert(sizeof(NmRegionsNote::Check) == sizeof(cvx_inv_check), "a checks note holds cvx_inv_check records");
std::atomic<bool> g_invChecksAnnounced(false);
std::atomic<long> g_invScored(0), g_invNoRead(0), g_invOwn[3], g_invVerified(0), g_invDisagreements(0), g_invRegionsOnly(0);
/* the binding's exit line: once per process, from the copy of this file whose Announce was called */
struct InvChecksExitLine {
	~InvChecksExitLine() {
		if (!g_invChecksAnnounced.load()) return;
		DeviceInvChecks::Counts const c = DeviceInvChecks::Stats();
		fprintf(stderr, "DeviceInvChecks: %ld checks taken from the job (%ld scored, %ld without a read part), %ld through checkForSV's own scoring "
				"(%ld no window, %ld inconsistent record, %ld note without checks), %ld verified, %ld disagreements\n",
				c.scored + c.noRead, c.scored, c.noRead, c.noWindow + c.inconsistent + c.noteWithoutChecks, c.noWindow, c.inconsistent, c.noteWithoutChecks,
				c.verified, c.disagreements);
	}
} g_invChecksExitLine;
}

void DeviceInvChecks::Announce() { g_invChecksAnnounced.store(true); }
bool DeviceInvChecks::Enabled() { return g_deviceInvChecks && g_invChecksAnnounced.load() && DeviceRegions::Enabled(); }
bool DeviceInvChecks::Verify() { return g_invChecksVerify; }
void DeviceInvChecks::CountTaken(bool scored) { (scored ? g_invScored : g_invNoRead).fetch_add(1, std::memory_order_relaxed); }
void DeviceInvChecks::CountOwn(Own why) { g_invOwn[(int) why].fetch_add(1, std::memory_order_relaxed); }
void DeviceInvChecks::CountVerified(bool agrees) {
	g_invVerified.fetch_add(1, std::memory_order_relaxed);
	if (!agrees) g_invDisagreements.fetch_add(1, std::memory_order_relaxed);
}
void DeviceInvChecks::CountRegionsOnly() { g_invRegionsOnly.fetch_add(1, std::memory_order_relaxed); }
DeviceInvChecks::Counts DeviceInvChecks::Stats() {
	Counts c;
	c.scored = g_invScored.load(); c.noRead = g_invNoRead.load();
	c.noWindow = g_invOwn[kNoWindow].load(); c.inconsistent = g_invOwn[kInconsistent].load(); c.noteWithoutChecks = g_invOwn[kNoteWithoutChecks].load();
	c.verified = g_invVerified.load(); c.disagreements = g_invDisagreements.load();
	c.regionsOnlyAlignments = g_invRegionsOnly.load();
	return c;
}

void ConvexAlignHip::ReadStats(long & notedLaunches, long & notedTiles, long & mixedLaunches) {
	notedLaunches = g_notedLaunches.load();
	notedTiles = g_notedTiles.load();
	mixedLaunches = g_mixedReadLaunches.load();
}

void ConvexAlignHip::WindowStats(long & windowLaunches, long & windowTiles, long & mixedLaunches) {
	windowLaunches = g_windowLaunches.load();
	windowTiles = g_windowTiles.load();
	mixedLaunches = g_mixedLaunches.load();
}

void ConvexAlignHip::JobTextStats(long & fromDevice, long & onHost) {
	fromDevice = g_textFromDevice.load();
	onHost = g_textOnHost.load();
}

void ConvexAlignHip::CorridorStats(long & prepared, long & closedForm) {
	prepared = g_prepared.load();
	closedForm = g_closedForm.load();
}

ConvexAlignHip::ConvexAlignHip(int const stdOutMode, float const match, float const mismatch,
		float const gapOpen, float const gapExtend, float const gapExtendMin, float const gapDecay,
		int const deviceId, unsigned long const maxMatrixSizeMB, bool const scalarTwin, bool const nmRegions, bool const jobText_, bool const invChecks_) : handle(0), twin(scalarTwin), regions(nmRegions), jobText(jobText_),
		invChecks(invChecks_ && nmRegions), genome(0) {
	(void) stdOutMode;
	cvx_params p;
	p.match = match; p.mismatch = mismatch; p.gap_open = gapOpen;
	p.gap_extend = gapExtend; p.gap_extend_min = gapExtendMin; p.gap_decay = gapDecay;
	maxMatrixMB = maxMatrixSizeMB;
#ifdef CVX_IN_NGMLR_TREE
	if (maxMatrixMB == 0) maxMatrixMB = (unsigned long) Config.getMaxMatrixSizeMB();
#endif
	if (maxMatrixMB == 0) maxMatrixMB = 10000;      /* IConfig's default (src/IConfig.h:47) */
	uint32_t const flags = (twin ? (uint32_t) CVX_CREATE_SCALAR_TWIN : 0u) | (regions ? (uint32_t) CVX_CREATE_NM_REGIONS : 0u) |
			(jobText ? (uint32_t) CVX_CREATE_JOB_TEXT : 0u) | (invChecks ? (uint32_t) CVX_CREATE_INV_CHECKS : 0u);
	if (cvx_create_ex(deviceId, &p, (uint64_t) maxMatrixMB, flags, &handle) != CVX_OK) {
		fprintf(stderr, "ConvexAlignHip: %s\n", cvx_last_error());
		throw "ConvexAlignHip: no usable MI355X / unsupported scoring";
	}
}

ConvexAlignHip::~ConvexAlignHip() {
	if (genome) cvx_genome_free(handle, genome);
	genome = 0;
	cvx_destroy(handle);
	handle = 0;
}

/* the reference's convex aligners answer 0 to both (src/ConvexAlignFast.cpp:434-439) */
int ConvexAlignHip::GetScoreBatchSize() const { return 0; }
int ConvexAlignHip::GetAlignBatchSize() const { return 0; }

int ConvexAlignHip::BatchScore(int const, int const, char const * const * const,
		char const * const * const, float * const, void *) {
	throw "Not implemented";
}

int ConvexAlignHip::BatchAlign(int const, int const, char const * const * const,
		char const * const * const, Align * const, void *) {
	throw "Not implemented";   /* no corridor in this signature; use AlignTiles() */
}

int ConvexAlignHip::SingleAlign(int const, int const, char const * const, char const * const,
		Align &, void *) {
	fprintf(stderr, "SingleAlign not implemented");
	throw "Not implemented";
}

int ConvexAlignHip::SingleAlign(int const mode, CorridorLine * corridor, int const corridorHeight,
		char const * const refSeq, char const * const qrySeq, Align & result,
		int const externalQStart, int const externalQEnd, void * extData) {
	(void) mode; (void) extData;
	Tile t;
	t.corridor = corridor; t.corridorHeight = corridorHeight;
	t.refSeq = refSeq; t.qrySeq = qrySeq; t.result = &result;
	t.externalQStart = externalQStart; t.externalQEnd = externalQEnd; t.ret = -1; t.failed = false;
	AlignTiles(&t, 1);
	if (t.failed) throw 1;
	return t.ret;
}

/* what the two strings of a request stand for: themselves, or -- a binding's placeholders -- a window of the resident genome and a
 * segment of a read; refLen / qryLen either way */
void ConvexAlignHip::resolveSequences(Tile & t) {
	t.window = false;
	t.refPosition = 0;
	int windowLength = 0;
	if (g_deviceDecode && g_binRef != 0 && DeviceWindows::Lookup(t.refSeq, t.refPosition, windowLength)) {
		t.window = true;                        /* the binding's placeholder: the string DecodeRefSequenceExact leaves has windowLength - 1 characters */
		t.refLen = windowLength - 1;
	} else {
		t.refLen = (int) strlen(t.refSeq);
	}
	t.segment = false;
	t.readSeq = 0;
	t.readLen = t.segStart = t.segFlags = 0;
	int segLength = 0;
	if (g_deviceReads && DeviceReads::Lookup(t.qrySeq, t.readSeq, t.readLen, t.segStart, segLength, t.segFlags)) {
		t.segment = true;                       /* the binding's placeholder: the string extractReadSeq leaves has segLength characters */
		t.qryLen = segLength;
	} else {
		t.qryLen = (int) strlen(t.qrySeq);
	}
}

void ConvexAlignHip::Prepare(Tile & t, bool const scalarTwin) {
	Align & a = *t.result;
	if (!scalarTwin) a.svType = 0;      /* ConvexAlignFast reads it as a debug id, then clears it; the scalar twin only reads it */
	a.Score = -1.0f;
	t.ret = -1;
	t.failed = false;
	resolveSequences(t);
	if (t.corridorHeight != t.qryLen) {
		/* every reference caller passes corridorHeight == strlen(qry); anything else
		 * indexes the corridor out of bounds in the reference itself */
		fprintf(stderr, "ConvexAlignHip: corridorHeight %d != read length %d\n", t.corridorHeight, t.qryLen);
		throw 1;
	}
	/* caller-visible side effect of AlignmentMatrixFast::prepare (src/AlignmentMatrixFast.cpp:39-44) */
	unsigned long acc = 0;
	for (int y = 0; y < t.corridorHeight; ++y) {
		t.corridor[y].offsetInMatrix = acc;
		acc += (unsigned long) (long) t.corridor[y].length;
	}
	/* The rows came out of one of ngmlr's corridor builders (src/AlignmentBuffer.cpp:68-197): recover its closed form -- in
	 * the caller's thread, every row verified against the expression the device evaluates -- so that the launch carries
	 * 32 bytes for this tile instead of 8 per read row through the pack threads, PCIe and the rows arena */
	t.corridorKind = CVX_CORRIDOR_ROWS;
	t.corridorK = t.corridorD = t.corridorRight = 0.0f;
	t.corridorOffset = t.corridorWidth = 0;
	g_prepared.fetch_add(1, std::memory_order_relaxed);
	if (g_fitCorridors && t.corridorHeight > 0) {
		cvx_tile form;
		if (cvx_corridor_fit(&t.corridor[0].offset, &t.corridor[0].length, (int32_t) sizeof(CorridorLine), t.corridorHeight, t.refLen, t.qryLen, &form) == CVX_OK
				&& form.corridor_kind != CVX_CORRIDOR_ROWS) {
			t.corridorKind = form.corridor_kind;
			t.corridorK = form.corridor_k; t.corridorD = form.corridor_d; t.corridorRight = form.corridor_right;
			t.corridorOffset = form.corridor_offset; t.corridorWidth = form.corridor_width;
			g_closedForm.fetch_add(1, std::memory_order_relaxed);
		}
	}
}

cvx_job ConvexAlignHip::Submit(Tile const * tiles, int n) {
	packed.resize((size_t) (n > 0 ? n : 1));
	for (int i = 0; i < n; ++i) {
		Tile const & t = tiles[i];
		cvx_tile & c = packed[(size_t) i];
		c.ref = t.refSeq;
		c.qry = t.qrySeq;
		c.ref_len = t.refLen;
		c.qry_len = t.qryLen;
		c.row_offset = &t.corridor[0].offset;
		c.row_length = &t.corridor[0].length;
		c.row_stride_bytes = (int32_t) sizeof(CorridorLine);
		/* ngmlr hands over the rows its corridor builders produced (src/AlignmentBuffer.cpp:68-197); Prepare() has recovered
		 * the builder's closed form where there is one (the arrays are then ignored by the library) */
		c.corridor_kind = t.corridorKind;
		c.corridor_k = t.corridorK; c.corridor_d = t.corridorD; c.corridor_right = t.corridorRight;
		c.corridor_offset = t.corridorOffset; c.corridor_width = t.corridorWidth;
		c.reserved = 0;
	}
	return submitPacked(tiles, n, 0);
}

/* packed[0 .. n) hold the tiles' strings, lengths and corridors: the launch in the form its sequences allow -- every reference a
 * window of the resident genome, every query a segment of a read, or characters -- as an ordinary job, or (ladders given) as a
 * ladder job whose tiles carry ladders[i] in place of packed[i]'s corridor */
cvx_job ConvexAlignHip::submitPacked(Tile const * tiles, int n, cvx_ladder const * ladders) {
	int nWindows = 0, nSegments = 0;
	for (int i = 0; i < n; ++i) { nWindows += tiles[i].window ? 1 : 0; nSegments += tiles[i].segment ? 1 : 0; }
	cvx_job job = 0;
	int rc;
	bool const noted = nSegments == n && n > 0;
	if (noted) {
		/* every query of the launch is a segment of a read: the launch's DISTINCT reads, as they lie in MappedRead::Seq, once
		 * each -- the widening retries and the left / right / inverted tiles of one read share its bytes -- and 16 bytes per tile
		 * (the reference: src/AlignmentBuffer.cpp:1515-1549 on the worker's core, then the string over PCIe once per tile) */
		std::unordered_map<char const *, int32_t> index;
		readArena.clear();
		readOffsets.assign(1, 0);
		segments.resize((size_t) n);
		for (int i = 0; i < n; ++i) {
			Tile const & t = tiles[i];
			std::pair<std::unordered_map<char const *, int32_t>::iterator, bool> const at = index.insert(std::make_pair(t.readSeq, (int32_t) index.size()));
			if (at.second) {
				readArena.insert(readArena.end(), (uint8_t const *) t.readSeq, (uint8_t const *) t.readSeq + t.readLen);
				readArena.push_back(0);
				readOffsets.push_back(readArena.size());
			}
			cvx_read_segment & s = segments[(size_t) i];
			s.read = at.first->second; s.start = t.segStart; s.flags = t.segFlags; s.reserved = 0;
			packed[(size_t) i].qry = 0;
		}
		g_notedLaunches.fetch_add(1, std::memory_order_relaxed);
		g_notedTiles.fetch_add(n, std::memory_order_relaxed);
	} else if (nSegments > 0) {
		materialiseReads(tiles, n);      /* a launch that mixes both forms */
	}
	if (nWindows > 0 && genome == 0) {
		if (cvx_genome_upload(handle, (uint8_t const *) g_binRef, g_nNibbles, g_startTable.data(), (int32_t) g_startTable.size(), &genome) != CVX_OK) {
			fprintf(stderr, "ConvexAlignHip: %s\n", cvx_last_error());
			throw 1;
		}
	}
	if (nWindows == n && n > 0) {
		/* every reference of the launch is a window of the resident genome: (position, length) per tile, decoded on the device
		 * straight into the launch's sequence arena (the reference: src/AlignmentBuffer.cpp:199-223 on the worker's core) */
		positions.resize((size_t) n);
		for (int i = 0; i < n; ++i) { positions[(size_t) i] = tiles[i].refPosition; packed[(size_t) i].ref = 0; }
		if (ladders) rc = cvx_submit_ladder_ex(handle, genome, n, packed.data(), (uint64_t const *) positions.data(), ladders, noted ? (int32_t) readOffsets.size() - 1 : 0,
				noted ? readArena.data() : 0, noted ? readOffsets.data() : 0, noted ? segments.data() : 0, &job);
		else if (noted) rc = cvx_submit_segments(handle, genome, n, packed.data(), (uint64_t const *) positions.data(), (int32_t) readOffsets.size() - 1,
				readArena.data(), readOffsets.data(), segments.data(), &job);
		else rc = cvx_submit_windows(handle, genome, n, packed.data(), (uint64_t const *) positions.data(), &job);
		g_windowLaunches.fetch_add(1, std::memory_order_relaxed);
		g_windowTiles.fetch_add(n, std::memory_order_relaxed);
	} else {
		if (nWindows > 0) materialiseWindows(tiles, n);      /* a launch that mixes both forms (no ngmlr path builds one) */
		/* (a plain aligner's ladders of plain strings go where they always went) */
		if (ladders && !noted && !regions && !jobText) rc = cvx_submit_ladder(handle, 0, n, packed.data(), 0, ladders, &job);
		else if (ladders) rc = cvx_submit_ladder_ex(handle, 0, n, packed.data(), 0, ladders, noted ? (int32_t) readOffsets.size() - 1 : 0,
				noted ? readArena.data() : 0, noted ? readOffsets.data() : 0, noted ? segments.data() : 0, &job);
		else if (noted) rc = cvx_submit_segments(handle, 0, n, packed.data(), 0, (int32_t) readOffsets.size() - 1, readArena.data(), readOffsets.data(), segments.data(), &job);
		else rc = cvx_submit(handle, n, packed.data(), &job);
	}
	if (rc != CVX_OK) {
		fprintf(stderr, "ConvexAlignHip: %s\n", cvx_last_error());
		throw 1;
	}
	return job;
}

/* the windows among the tiles decoded into their callers' placeholder buffers (which extractReferenceSequenceForAlignment
 * allocated writable, window length + 100 bytes), so that the launch can travel as characters */
void ConvexAlignHip::materialiseWindows(Tile const * tiles, int n) {
	std::vector<uint64_t> pos, off;
	std::vector<int32_t> len;
	std::vector<int> who;
	uint64_t total = 0;
	for (int i = 0; i < n; ++i) if (tiles[i].window) {
		who.push_back(i);
		pos.push_back(tiles[i].refPosition);
		len.push_back(tiles[i].refLen + 1);
		off.push_back(total);
		total += (uint64_t) tiles[i].refLen + 1;
	}
	std::vector<char> out((size_t) total + 8);
	if (cvx_genome_decode(handle, genome, (int32_t) who.size(), pos.data(), len.data(), off.data(), out.data()) != CVX_OK) {
		fprintf(stderr, "ConvexAlignHip: %s\n", cvx_last_error());
		throw 1;
	}
	for (size_t k = 0; k < who.size(); ++k) memcpy(const_cast<char *>(tiles[who[k]].refSeq), out.data() + off[k], (size_t) len[k]);
	g_mixedLaunches.fetch_add(1, std::memory_order_relaxed);
}

/* the noted queries among the tiles built on the host in their callers' placeholder buffers (which the binding allocated
 * writable, length + 1 bytes), so that the launch can travel as characters */
void ConvexAlignHip::materialiseReads(Tile const * tiles, int n) {
	for (int i = 0; i < n; ++i) if (tiles[i].segment) {
		Tile const & t = tiles[i];
		if (!readString(t.readSeq, t.readLen, t.segStart, t.qryLen, t.segFlags, 0, t.qryLen, const_cast<char *>(t.qrySeq))) {
			fprintf(stderr, "ConvexAlignHip: %s\n", cvx_last_error());
			throw 1;
		}
	}
	g_mixedReadLaunches.fetch_add(1, std::memory_order_relaxed);
}

bool ConvexAlignHip::Poll(cvx_job job) {
	int32_t done = 0;
	if (cvx_job_poll(handle, job, &done) != CVX_OK) return true;      /* let Wait report it */
	return done != 0;
}

void ConvexAlignHip::Wait(cvx_job job, cvx_result const ** results, uint32_t const ** ops) {
	uint64_t nOps = 0;
	if (cvx_wait(handle, job, results, ops, &nOps) != CVX_OK) {
		fprintf(stderr, "ConvexAlignHip: %s\n", cvx_last_error());
		throw 1;
	}
}

bool ConvexAlignHip::Regions(cvx_job job, JobRegions & jr) {
	jr.off = 0; jr.regions = 0; jr.checks = 0;
	if (!regions) return false;
	if (cvx_job_regions(handle, job, &jr.off, &jr.regions, 0) != CVX_OK) {
		/* a request must never be answered with nothing: fail the launch like any other error of it */
		fprintf(stderr, "ConvexAlignHip: %s\n", cvx_last_error());
		throw 1;
	}
	/* the checks came back with the regions (no device call); NULL for a launch without the genome or without a region */
	if (invChecks && cvx_job_checks(handle, job, &jr.checks) != CVX_OK) {
		fprintf(stderr, "ConvexAlignHip: %s\n", cvx_last_error());
		throw 1;
	}
	return true;
}

bool ConvexAlignHip::JobTexts(cvx_job job, JobTextView & jx) {
	jx.recs = 0; jx.off = 0; jx.text = 0;
	if (!jobText) return false;
	if (cvx_job_texts(handle, job, &jx.recs, &jx.off, &jx.text) != CVX_OK) {
		fprintf(stderr, "ConvexAlignHip: %s\n", cvx_last_error());
		throw 1;
	}
	return true;
}

bool ConvexAlignHip::WindowRefs(cvx_job job, Tile * const * tiles, int n) {
	int nWindows = 0;
	for (int i = 0; i < n; ++i) nWindows += tiles[i]->window ? 1 : 0;
	if (nWindows == 0 || n <= 0) return false;
	if (nWindows < n) return false;      /* a mixed launch travelled as characters: its windows were materialised in the callers' buffers (Submit) */
	std::vector<char const *> refs((size_t) n);
	if (cvx_job_window_refs(handle, job, refs.data()) != CVX_OK) {
		/* the placeholders must never reach the text stage: fail the launch like any other error of it */
		fprintf(stderr, "ConvexAlignHip: %s\n", cvx_last_error());
		throw 1;
	}
	for (int i = 0; i < n; ++i) tiles[i]->refSeq = refs[(size_t) i];
	return true;
}

void ConvexAlignHip::Trace(cvx_job job, int nTiles, double serviceMs, double waitedMs) const {
	cvx_timing t;
	if (cvx_job_timing(job, &t) != CVX_OK) return;
	char cls[256];
	int at = 0;
	cls[0] = '\0';
	for (int i = 0; i < t.n_fill_launches && at < 200; ++i) {
		cvx_launch_info li;
		if (cvx_job_launch_info(job, i, &li) != CVX_OK) break;
		at += snprintf(cls + at, sizeof(cls) - (size_t) at, " M%d%s x%d %.2f ms", li.slots_per_lane, li.kind == CVX_LAUNCH_CHAINED ? "c" : (li.kind == CVX_LAUNCH_GANG ? "g" : (li.kind == CVX_LAUNCH_CATCH_ALL ? "x" : "")), li.n_tiles, li.ms);
	}
	fprintf(stderr, "cvx launch: %d tiles, %.1f M cells, oldest request waited %.1f ms, in flight %.1f ms: plan %.2f fill %.2f walk %.2f device total %.2f ms;%s%s\n",
			nTiles, (double) t.cells * 1e-6, waitedMs, serviceMs, t.plan_ms, t.fill_ms, t.backtrack_ms, t.total_ms, cls, t.n_tiles_redone ? " (redo)" : "");
}

void ConvexAlignHip::Release(cvx_job job) {
	cvx_job_release(handle, job);
}

void ConvexAlignHip::AlignTiles(Tile * tiles, int n) {
	if (n <= 0) return;
	for (int i = 0; i < n; ++i) Prepare(tiles[i], twin);
	cvx_job job = Submit(tiles, n);
	cvx_result const * res = 0;
	uint32_t const * ops = 0;
	try {
		Wait(job, &res, &ops);
	} catch (...) {
		Release(job);
		throw;
	}
	/* windows decoded on the device: the host text stage reads the characters that came back with the results */
	std::vector<char const *> callers((size_t) n);
	std::vector<Tile *> ptrs((size_t) n);
	for (int i = 0; i < n; ++i) { callers[(size_t) i] = tiles[i].refSeq; ptrs[(size_t) i] = &tiles[i]; }
	JobRegions jr;
	JobTextView jx;
	bool haveRegions = false, haveTexts = false;
	try {
		(void) WindowRefs(job, ptrs.data(), n);
		haveRegions = Regions(job, jr);
		haveTexts = JobTexts(job, jx);
	} catch (...) {
		Release(job);
		throw;
	}
	for (int i = 0; i < n; ++i) {
		try {
			Finish(tiles[i], res[i], ops, haveRegions ? &jr : 0, i, haveTexts ? &jx : 0);
		} catch (...) {
			/* this tile's own hard error: the caller drops this alignment and no other (src/AlignmentBuffer.cpp:454-463) */
			tiles[i].failed = true;
			tiles[i].ret = -1;
			tiles[i].result->Score = -1.0f;
		}
	}
	for (int i = 0; i < n; ++i) tiles[i].refSeq = callers[(size_t) i];
	Release(job);
}

/* the request as a Tile without a corridor: the strings resolved the way Prepare resolves them (windows and read placeholders of a
 * binding included), in the calling context, so that the launch takes Submit's forms and the tile finishes the way Finish
 * finishes any */
void ConvexAlignHip::PrepareLadder(LadderTile & lt) {
	lt.ret = -1; lt.failed = false; lt.rung = lt.attempts = lt.width = 0;
	if (lt.refSeq == 0 || lt.qrySeq == 0 || lt.result == 0) {
		fprintf(stderr, "ConvexAlignHip: a ladder request without its strings or its Align\n");
		throw 1;
	}
	Tile & t = lt.resolved;
	memset(&t, 0, sizeof(t));
	t.refSeq = lt.refSeq; t.qrySeq = lt.qrySeq; t.result = lt.result;
	t.externalQStart = lt.externalQStart; t.externalQEnd = lt.externalQEnd;
	t.ret = -1;
	resolveSequences(t);
	t.corridorHeight = t.qryLen;
	/* what cvx_submit_ladder would refuse for the whole launch (an unknown flag, a negative corridor, left / right out of range)
	 * is this caller's error alone */
	cvx_tile probe, form;
	memset(&probe, 0, sizeof(probe));
	memset(&form, 0, sizeof(form));
	probe.ref_len = t.refLen; probe.qry_len = t.qryLen;
	if (cvx_ladder_rung(&probe, &lt.ladder, 1, &form) < 0) {
		fprintf(stderr, "ConvexAlignHip: %s\n", cvx_last_error());
		throw 1;
	}
}

cvx_job ConvexAlignHip::SubmitLadders(LadderTile const * tiles, int n) {
	std::vector<Tile> ts((size_t) (n > 0 ? n : 0));
	std::vector<cvx_ladder> lad((size_t) (n > 0 ? n : 0));
	packed.resize((size_t) (n > 0 ? n : 1));
	for (int i = 0; i < n; ++i) {
		Tile const & t = ts[(size_t) i] = tiles[i].resolved;
		cvx_tile & c = packed[(size_t) i];
		memset(&c, 0, sizeof(c));
		c.ref = t.refSeq; c.qry = t.qrySeq;
		c.ref_len = t.refLen; c.qry_len = t.qryLen;
		c.row_stride_bytes = 4;
		lad[(size_t) i] = tiles[i].ladder;
	}
	return submitPacked(ts.data(), n, lad.data());
}

void ConvexAlignHip::Ladders(cvx_job job, cvx_ladder_result const ** out) {
	if (cvx_job_ladder(handle, job, out) != CVX_OK) {
		fprintf(stderr, "ConvexAlignHip: %s\n", cvx_last_error());
		throw 1;
	}
}

void ConvexAlignHip::FinishLadder(LadderTile & lt, cvx_result const & r, uint32_t const * ops, cvx_ladder_result const & lr, JobRegions const * jr, int index, JobTextView const * jx) const {
	lt.rung = lr.rung; lt.attempts = lr.attempts; lt.width = lr.width;
	Finish(lt.resolved, r, ops, jr, index, jx);
	lt.ret = lt.resolved.ret;
}

void ConvexAlignHip::AlignLadders(LadderTile * tiles, int n) {
	if (n <= 0) return;
	for (int i = 0; i < n; ++i) PrepareLadder(tiles[i]);
	cvx_job job = SubmitLadders(tiles, n);
	cvx_result const * res = 0;
	uint32_t const * ops = 0;
	cvx_ladder_result const * lr = 0;
	std::vector<Tile *> ptrs((size_t) n);
	for (int i = 0; i < n; ++i) ptrs[(size_t) i] = &tiles[i].resolved;
	JobRegions jr;
	JobTextView jx;
	bool haveRegions = false, haveTexts = false;
	try {
		Wait(job, &res, &ops);
		Ladders(job, &lr);
		(void) WindowRefs(job, ptrs.data(), n);      /* windows decoded on the device: the host text stage reads what came back */
		haveRegions = Regions(job, jr);
		haveTexts = JobTexts(job, jx);
	} catch (...) {
		Release(job);
		throw;
	}
	for (int i = 0; i < n; ++i) {
		try {
			FinishLadder(tiles[i], res[i], ops, lr[i], haveRegions ? &jr : 0, i, haveTexts ? &jx : 0);
		} catch (...) {
			tiles[i].failed = true;
			tiles[i].ret = -1;
			tiles[i].result->Score = -1.0f;
		}
	}
	Release(job);
}

/* convertCigar + flags into the caller's Align (src/ConvexAlignFast.cpp:488-539) */
void ConvexAlignHip::Finish(Tile & t, cvx_result const & r, uint32_t const * ops, JobRegions const * jr, int index, JobTextView const * jx) const {
	Align & a = *t.result;
	int const refLen = t.refLen, qryLen = t.qryLen;
	if (noAlignment(t, r)) return;      /* (a request stays where it is for the caller's retry) */
	/* nm_regions_note.h: the caller asked for regions.  With the job's regions at hand the text is formatted without a profile
	 * (nm_triples = NULL counts the entries and writes none) and the note goes where the profile would have gone; without them
	 * the request -- or the note an earlier call left -- is cleared and the profile is written as always */
	bool const asNote = jr != 0 && jr->off != 0 && NmRegionsNote::Begin(a.nmPerPosition, a.nmPerPostionLength, true);
	if (asNote && jx != 0 && jx->recs != 0) {      /* the launch brought this tile's text: nothing walks its ops */
		g_textFromDevice.fetch_add(1, std::memory_order_relaxed);
		FinishJobText(t, *jx, *jr, index);
		return;
	}
	g_textOnHost.fetch_add(1, std::memory_order_relaxed);
	/* (the request's buffer is a few dozen rows, and the finder's loop scans alignmentLength rows of a profile: the buffer becomes
	 * the one the caller allocates when it does not ask, and covers alignmentLength below) */
	bool const fromRequest = !asNote && NmRegionsNote::BeginProfile(a.nmPerPosition, a.nmPerPostionLength, qryLen);
	cvx_alignment_text txt;
	for (;;) {
		int rc = cvx_format_alignment_ex(&r, ops, t.refSeq, refLen, qryLen, t.externalQStart,
				t.externalQEnd, a.pBuffer1, a.maxBufferLength, a.pBuffer2, a.maxMdBufferLength,
				asNote ? (int32_t *) 0 : (int32_t *) a.nmPerPosition, asNote ? 0 : a.nmPerPostionLength, twin ? (uint32_t) CVX_FORMAT_SCALAR_TWIN : 0u, &txt);
		if (rc != CVX_OK) throw 1;
		bool again = false;
		if (txt.md_len >= a.maxMdBufferLength) {       /* checkMdBufferLength: grow with new[] */
			int cap = a.maxMdBufferLength > 0 ? a.maxMdBufferLength : 64;
			while (cap <= txt.md_len) cap *= 2;
			delete[] a.pBuffer2;
			a.pBuffer2 = new char[cap];
			a.maxMdBufferLength = cap;
			again = true;
		}
		if (!asNote && txt.nm_count > a.nmPerPostionLength) {      /* addPosition: grow with new[] */
			int cap = a.nmPerPostionLength > 0 ? a.nmPerPostionLength : 64;
			while (cap < txt.nm_count) cap *= 2;
			delete[] a.nmPerPosition;
			a.nmPerPosition = new PositionNM[cap];
			a.nmPerPostionLength = cap;
			again = true;
		}
		if (!again) break;
	}
	if (fromRequest) NmRegionsNote::CoverScan(a.nmPerPosition, a.nmPerPostionLength, txt.nm_count, txt.alignment_length);
	if (asNote) putNote(a, *jr, index);
	if (txt.cigar_len > a.maxBufferLength) {
		fprintf(stderr, "CIGAR/MD buffer not long enough (%d %d > %d %d). Please report this!\n",
				txt.cigar_len, txt.md_len, a.maxBufferLength, a.maxMdBufferLength);
		throw 1;
	}
	fillAlign(t, txt);
}

void ConvexAlignHip::FinishJobText(Tile & t, JobTextView const & jx, JobRegions const & jr, int index) const {
	Align & a = *t.result;
	cvx_alignment_text const & rec = jx.recs[index];
	char const * src = jx.text + jx.off[index];
	if (rec.md_len >= a.maxMdBufferLength) {       /* checkMdBufferLength: grow with new[] */
		int cap = a.maxMdBufferLength > 0 ? a.maxMdBufferLength : 64;
		while (cap <= rec.md_len) cap *= 2;
		delete[] a.pBuffer2;
		a.pBuffer2 = new char[cap];
		a.maxMdBufferLength = cap;
	}
	cvx_alignment_text txt;
	if (cvx_text_reclip(&rec, src, t.externalQStart, t.externalQEnd, a.pBuffer1, a.maxBufferLength, &txt) != CVX_OK) {
		fprintf(stderr, "ConvexAlignHip: %s\n", cvx_last_error());
		throw 1;
	}
	memcpy(a.pBuffer2, src + rec.cigar_len + 1, (size_t) rec.md_len + 1);
	putNote(a, jr, index);
	if (txt.cigar_len > a.maxBufferLength) {
		fprintf(stderr, "CIGAR/MD buffer not long enough (%d %d > %d %d). Please report this!\n",
				txt.cigar_len, txt.md_len, a.maxBufferLength, a.maxMdBufferLength);
		throw 1;
	}
	fillAlign(t, txt);
}

/* the answer to a request: the tile's regions, and -- where the binding reads them and the job brought them -- their check records
 * behind them; a job without checks (its windows were materialised on the host) answers with the regions-only note */
void ConvexAlignHip::putNote(Align & a, JobRegions const & jr, int index) const {
	static_assert(sizeof(NmRegionsNote::Region) == sizeof(cvx_nm_region), "a note holds cvx_nm_region records");
	int const count = (int) (jr.off[index + 1] - jr.off[index]);
	NmRegionsNote::Region const * mine = count > 0 ? reinterpret_cast<NmRegionsNote::Region const *>(jr.regions + jr.off[index]) : 0;
	if (jr.checks != 0 && DeviceInvChecks::Enabled()) {
		NmRegionsNote::PutChecks(a.nmPerPosition, a.nmPerPostionLength, mine, reinterpret_cast<NmRegionsNote::Check const *>(jr.checks + jr.off[index]), count);
		return;
	}
	if (count > 0 && invChecks && DeviceInvChecks::Enabled()) DeviceInvChecks::CountRegionsOnly();
	NmRegionsNote::Put(a.nmPerPosition, a.nmPerPostionLength, mine, count);
}

void ConvexAlignHip::fillAlign(Tile & t, cvx_alignment_text const & txt) const {
	Align & a = *t.result;
	a.QStart = txt.qstart;
	a.QEnd = txt.qend;
	a.firstPosition.refPosition = txt.first_ref;
	a.firstPosition.readPosition = txt.first_read;
	a.lastPosition.refPosition = txt.last_ref;
	a.lastPosition.readPosition = txt.last_read;
	a.Identity = txt.identity;
	a.NM = txt.nm;
	a.alignmentLength = txt.alignment_length;
	a.PositionOffset = txt.position_offset;
	a.Score = txt.score;
	if (!twin) {                /* the scalar twin writes neither (both come back as CVX_NOT_WRITTEN): the caller's values stay */
		a.cigarOpCount = txt.cigar_op_count;
		a.svType = txt.sv_type;
	}
	t.ret = txt.ret;
}

/* true: the tile has no alignment and the Align says so already (the cases Finish handles before it formats anything) */
bool ConvexAlignHip::noAlignment(Tile & t, cvx_result const & r) const {
	Align & a = *t.result;
	if (r.status == CVX_TILE_UNSUPPORTED) {
		fprintf(stderr, "ConvexAlignHip: corridor shape not covered by any device kernel\n");
		throw 1;
	}
	if (r.status == CVX_TILE_OK) return false;
	if (r.status == CVX_TILE_TOO_LARGE) {
		/* the reference's message (src/AlignmentMatrixFast.cpp:56), same float arithmetic for the size */
		fprintf(stderr, "Warning: Couldn't allocate alignment matrix. Required memory (%llu) > max matrix size (%lu)\n\n",
				(long long) ((float) r.cells / 1000.0f / 1000.0f), maxMatrixMB);
	} else if (a.pBuffer2 != 0) {
		a.pBuffer2[0] = '\0';
	}
	a.Score = -1.0f;
	t.ret = -1;
	return true;
}

void ConvexAlignHip::Text(cvx_job job, Tile const * const * tiles, int n, JobText & jt) {
	size_t const n1 = (size_t) (n > 0 ? n : 0);
	jt.out.resize(n1 + 1);
	jt.textOff.resize(n1 + 1);
	jt.nmOff.assign(n1 + 1, 0);
	jt.text = "";
	if (n <= 0) return;
	std::vector<int32_t> ext(2 * n1);
	for (size_t i = 0; i < n1; ++i) { ext[i] = tiles[i]->externalQStart; ext[n1 + i] = tiles[i]->externalQEnd; }
	uint64_t bytes = 0;
	jt.nm = 0;
	int const rc = cvx_job_text_all(handle, job, ext.data(), ext.data() + n1, jt.out.data(), jt.textOff.data(), &jt.text, &bytes, jt.nmOff.data(), &jt.nm);
	if (rc != CVX_OK) {
		fprintf(stderr, "ConvexAlignHip: %s\n", cvx_last_error());
		throw 1;
	}
}

/* what Finish leaves in the caller's Align, copied out of the job's device-made text (same growth rules for pBuffer2 and
 * nmPerPosition, same hard error for a CIGAR beyond the caller's buffer) */
void ConvexAlignHip::FinishText(Tile & t, cvx_result const & r, JobText const & jt, int index) const {
	if (noAlignment(t, r)) return;
	Align & a = *t.result;
	/* this path has no regions: a request ends as the profile, in a buffer as long as the caller's own would have been */
	bool const fromRequest = NmRegionsNote::BeginProfile(a.nmPerPosition, a.nmPerPostionLength, t.qryLen);
	cvx_alignment_text const & txt = jt.out[(size_t) index];
	if (txt.md_len >= a.maxMdBufferLength) {       /* checkMdBufferLength: grow with new[] */
		int cap = a.maxMdBufferLength > 0 ? a.maxMdBufferLength : 64;
		while (cap <= txt.md_len) cap *= 2;
		delete[] a.pBuffer2;
		a.pBuffer2 = new char[cap];
		a.maxMdBufferLength = cap;
	}
	if (txt.nm_count > a.nmPerPostionLength) {      /* addPosition: grow with new[] */
		int cap = a.nmPerPostionLength > 0 ? a.nmPerPostionLength : 64;
		while (cap < txt.nm_count) cap *= 2;
		delete[] a.nmPerPosition;
		a.nmPerPosition = new PositionNM[cap];
		a.nmPerPostionLength = cap;
	}
	if (txt.cigar_len > a.maxBufferLength) {
		fprintf(stderr, "CIGAR/MD buffer not long enough (%d %d > %d %d). Please report this!\n",
				txt.cigar_len, txt.md_len, a.maxBufferLength, a.maxMdBufferLength);
		throw 1;
	}
	char const * src = jt.text + jt.textOff[(size_t) index];
	memcpy(a.pBuffer1, src, (size_t) (txt.cigar_len + 1 <= a.maxBufferLength ? txt.cigar_len + 1 : a.maxBufferLength));
	memcpy(a.pBuffer2, src + txt.cigar_len + 1, (size_t) txt.md_len + 1);
	uint64_t const e0 = jt.nmOff[(size_t) index], e1 = jt.nmOff[(size_t) index + 1];
	if ((uint64_t) txt.nm_count != e1 - e0) {
		fprintf(stderr, "ConvexAlignHip: nmPerPosition count of the device (%llu) differs from the text stage's (%d)\n", (unsigned long long) (e1 - e0), txt.nm_count);
		throw 1;
	}
	if (e1 > e0) memcpy((void *) a.nmPerPosition, jt.nm + 3 * e0, (size_t) (e1 - e0) * 3 * sizeof(int32_t));
	if (fromRequest) NmRegionsNote::CoverScan(a.nmPerPosition, a.nmPerPostionLength, txt.nm_count, txt.alignment_length);
	fillAlign(t, txt);
}

}  // namespace Convex
