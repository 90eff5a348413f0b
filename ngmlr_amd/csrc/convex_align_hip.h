/*
 * convex_align_hip.h -- the drop-in: an IAlignment implementation that runs ngmlr's
 * convex-gap alignment on an MI355X through the C ABI of include/cvx_align.h.
 *
 * It takes the place of Convex::ConvexAlignFast at the one construction site
 * (reference src/AlignmentBuffer.h:355-363) and keeps its contract:
 *   - same constructor arguments (stdOutMode + six scoring floats), plus a device id;
 *   - SingleAlign(mode, CorridorLine*, ...) has the same argument meaning, side effects
 *     (offsetInMatrix written into the caller's lines, pBuffer2 / nmPerPosition possibly
 *     re-allocated with new[], align.svType consumed as read id then reset) and the same
 *     error convention: -1 / Score -1.0f for "no valid alignment", `throw 1` for hard
 *     errors (reference src/ConvexAlignFast.cpp:452-559);
 *   - BatchScore / corridor-less SingleAlign throw like the reference's do.
 * Extra: AlignTiles() -- many corridor alignments in one launch (the shape the
 * reference's BatchAlign slot lacks a corridor argument for) -- and its split form
 * Submit() / Wait() / Finish() / Release(), which keeps several launches in flight
 * (batching_aligner.h drives it from one dispatcher thread per device).
 */
#ifndef CONVEX_ALIGN_HIP_H
#define CONVEX_ALIGN_HIP_H

#include <stdint.h>
#include <vector>

#include "ngmlr_abi.h"
#include "cvx_align.h"

namespace Convex {

class ConvexAlignHip: public IAlignment {
public:
	ConvexAlignHip(int const stdOutMode, float const match, float const mismatch, float const gapOpen,
			float const gapExtend, float const gapExtendMin, float const gapDecay, int const deviceId = 0,
			unsigned long const maxMatrixSizeMB = 0 /* Config.getMaxMatrixSizeMB(); 0 = the reference's default 10000 */,
			bool const scalarTwin = false, bool const nmRegions = false, bool const jobText = false, bool const invChecks = false);
	/* invChecks: the handle is created with CVX_CREATE_INV_CHECKS (only together with nmRegions; alone it is ignored) -- every launch
	 * that travelled with the resident genome brings checkForSV's two scores per region back beside its regions (cvx_job_checks),
	 * and, where DeviceInvChecks::Enabled(), Finish answers a request with the checks form of the note (nm_regions_note.h).  A launch
	 * that materialised its windows on the host brings none: its requests get today's regions-only note. */
	bool InvChecks() const { return invChecks; }
	/* jobText: the handle is created with CVX_CREATE_JOB_TEXT -- every launch brings CIGAR, MD and the scalar fields of its tiles back
	 * with its results (external clips zero), and Finish copies them (FinishJobText) for every tile whose request it answers with a
	 * note instead of walking the tile's ops; a tile that wants its profile keeps the host form, in the same launch. */
	bool JobTextOn() const { return jobText; }
	/* nmRegions: the handle is created with CVX_CREATE_NM_REGIONS -- every launch brings the low-identity regions of its tiles back
	 * with its results, and Finish answers a request in Align::nmPerPosition (nm_regions_note.h) with a note of them instead of
	 * the profile.  Without it (and on the CVX_DEVICE_TEXT=1 path) a request ends as the full profile. */
	bool NmRegions() const { return regions; }
	/* scalarTwin: the drop-in takes the place of Convex::ConvexAlign, the scalar aligner ngmlr's --nosse binds at
	 * src/AlignmentBuffer.h:345-353, instead of ConvexAlignFast's (CVX_CREATE_SCALAR_TWIN, include/cvx_align.h).  In that mode
	 * SingleAlign / AlignTiles leave Align::svType and Align::cigarOpCount exactly as the caller passed them -- no clear at entry,
	 * no assignment at exit: the twin only reads svType (src/ConvexAlign.cpp:423), and ngmlr prints what it stored there
	 * (the read's id, src/AlignmentBuffer.cpp:362) as SV:i. */
	bool ScalarTwin() const { return twin; }
	virtual ~ConvexAlignHip();

	virtual int GetScoreBatchSize() const;
	virtual int GetAlignBatchSize() const;

	virtual int BatchScore(int const mode, int const batchSize, char const * const * const refSeqList,
			char const * const * const qrySeqList, float * const results, void * extData);
	virtual int BatchAlign(int const mode, int const batchSize, char const * const * const refSeqList,
			char const * const * const qrySeqList, Align * const results, void * extData);
	virtual int SingleAlign(int const mode, int const corridor, char const * const refSeq,
			char const * const qrySeq, Align & result, void * extData);
	virtual int SingleAlign(int const mode, CorridorLine * corridor, int const corridorHeight,
			char const * const refSeq, char const * const qrySeq, Align & result,
			int const externalQStart, int const externalQEnd, void * extData);

	/* One request of AlignTiles(): exactly the arguments of the corridor SingleAlign. */
	struct Tile {
		CorridorLine * corridor;
		int corridorHeight;
		char const * refSeq;
		char const * qrySeq;
		Align * result;
		int externalQStart;
		int externalQEnd;
		int ret;               /* out: what SingleAlign would have returned */
		bool failed;           /* out (AlignTiles): this tile hit a hard error -- the reference would have thrown for it alone */
		int refLen, qryLen;    /* filled by Prepare() */
		/* filled by Prepare(): the closed form behind `corridor` when cvx_corridor_fit finds one (every row verified), else
		 * CVX_CORRIDOR_ROWS -- Submit then sends 32 bytes instead of the tile's row arrays */
		int32_t corridorKind;
		float corridorK, corridorD, corridorRight;
		int32_t corridorOffset, corridorWidth;
		/* filled by Prepare(): refSeq is a placeholder for the window of the resident genome at refPosition (DeviceWindows
		 * below) -- the launch carries (position, length) and the device decodes; Finish needs WindowRefs() first */
		bool window;
		unsigned long long refPosition;
		/* filled by Prepare(): qrySeq is a placeholder for a segment of a read (DeviceReads below) -- the launch carries
		 * (read, start, flags) and the device writes the query; nothing on the host reads its characters afterwards (the text
		 * stage takes no query) */
		bool segment;
		char const * readSeq;
		int readLen, segStart, segFlags;
	};
	/* n independent corridor alignments in one device launch.  A hard error that belongs to one tile (a corridor no
	 * kernel covers, a CIGAR that does not fit the caller's buffer) marks that tile `failed` and leaves the others
	 * alone -- the reference's caller drops exactly one alignment in that case (src/AlignmentBuffer.cpp:454-463);
	 * a failure of the launch itself throws. */
	void AlignTiles(Tile * tiles, int n);

	struct JobRegions;
	struct JobTextView;
	/* One request of AlignLadders(): what AlignmentBuffer::computeAlignment's retry loop reads (src/AlignmentBuffer.cpp:259-425)
	 * in place of one CorridorLine[] -- see cvx_ladder, include/cvx_align.h. */
	struct LadderTile {
		char const * refSeq;
		char const * qrySeq;
		Align * result;
		int externalQStart;
		int externalQEnd;
		cvx_ladder ladder;     /* corridor as passed to computeAlignment; left / right of the anchors builder; CVX_LADDER_* flags */
		int ret;               /* out: the reference's cigarLength of the rung reported, or -1 */
		bool failed;           /* out: this tile hit a hard error */
		int rung, attempts, width;      /* out: the rung reported (1-based), the attempts made, that rung's corridor width */
		/* filled by PrepareLadder(): the request as a Tile without a corridor -- placeholders recognised, refLen / qryLen -- which
		 * SubmitLadders packs and FinishLadder finishes the way Finish finishes any tile */
		Tile resolved;
	};
	/* n retry ladders in one device job (cvx_submit_ladder; cvx_submit_ladder_ex on an aligner constructed with nmRegions and / or
	 * jobText, and for the placeholder forms below): every tile's corridor is rebuilt at multiplier 2, 3, ... and aligned again on
	 * the device while its attempt is invalid and a further rung exists; `result` is filled the way SingleAlign fills it for the
	 * rung reported -- on an aligner with nmRegions a request in Align::nmPerPosition is answered with a note of that rung's
	 * regions, with jobText such a tile takes its CIGAR and MD from the job's text (FinishJobText + cvx_text_reclip), every other
	 * tile the host form, exactly as AlignTiles finishes them.  The input forms are Submit's: every refSeq a DeviceWindows
	 * placeholder -- the genome form; every qrySeq a DeviceReads placeholder -- the segments form, distinct reads sent once; a
	 * mix is materialised on the host.  Hard errors as for AlignTiles. */
	void AlignLadders(LadderTile * tiles, int n);
	/* The same in stages, as AlignTiles has them (below), for a driver that gathers a launch from many calling contexts
	 * (batching_aligner.h).  Poll, Wait, Regions, JobTexts, WindowRefs (on &tile.resolved) and Release work on the job as on any.
	 *   PrepareLadder  any thread, the CALLER's: recognises the DeviceWindows / DeviceReads placeholders where a window's note
	 *                  lives and takes the lengths; throws 1 for a malformed call (no strings, no Align, a ladder cvx_ladder_rung
	 *                  refuses).  No corridor is fitted and no CorridorLine is touched: there is none
	 *   SubmitLadders  the device thread: one ladder job of n prepared tiles, in the input form Submit would choose
	 *   Ladders        after Wait: the job's cvx_job_ladder records, valid until Release
	 *   FinishLadder   any thread: one tile's Align out of the job's buffers as Finish leaves it for the rung reported, and
	 *                  ret / rung / attempts / width; throws 1 for that tile's hard errors */
	static void PrepareLadder(LadderTile & t);
	cvx_job SubmitLadders(LadderTile const * tiles, int n);
	void Ladders(cvx_job job, cvx_ladder_result const ** out);
	void FinishLadder(LadderTile & t, cvx_result const & r, uint32_t const * ops, cvx_ladder_result const & lr, JobRegions const * jr = 0, int index = 0, JobTextView const * jx = 0) const;

	/* The same in stages, for a driver that keeps launches in flight.  Prepare / Finish may run on any thread (they
	 * touch only the tile and the caller's Align); Submit / Wait / Release belong to the ONE thread that owns this
	 * aligner's device handle.
	 *   Prepare  strlen + height check + the caller-visible offsetInMatrix side effect (throws like SingleAlign) + the
	 *            corridor's closed form (cvx_corridor_fit; CVX_CORRIDOR_FIT=0 sends the rows as round 5 did)
	 *   Submit   queues a launch for n prepared tiles, returns its job (throws on a hard error of the launch)
	 *   Poll     non-blocking "is it done"; Wait  blocks until the job is done: result records and run-length ops, valid until Release
	 *   Finish   convertCigar + flags of ONE tile into its Align (throws 1 for that tile's hard errors)
	 *   Release  gives the job's buffers back */
	static void Prepare(Tile & t, bool scalarTwin = false);      /* scalarTwin: of the aligner the tile goes to (ScalarTwin()) */
	cvx_job Submit(Tile const * tiles, int n);
	bool Poll(cvx_job job);       /* true: Wait would not block (also keeps queued launches moving) */
	void Wait(cvx_job job, cvx_result const ** results, uint32_t const ** ops);
	/* the regions of a finished job (cvx_job_regions: the job's page-locked memory, valid until Release); tile i owns
	 * regions[off[i] .. off[i + 1]); checks (cvx_job_checks, the same memory and lifetime): the check record of every region, parallel
	 * to `regions` -- NULL where the handle delivers none, the job travelled without a genome, or the job has no region */
	struct JobRegions {
		uint64_t const * off;
		cvx_nm_region const * regions;
		cvx_inv_check const * checks = 0;
	};
	bool Regions(cvx_job job, JobRegions & jr);      /* after Wait.  false: the handle delivers none (throws 1 when one that should cannot) */
	/* jr / index: the launch's regions and the tile's place in it.  With them a request (or an earlier note) in
	 * Align::nmPerPosition is answered with a note and no profile is written; without them it ends as the profile */
	/* the records and strings of a finished job (cvx_job_texts: the job's page-locked memory, valid until Release); tile i's CIGAR
	 * is the string at text[off[i]], its MD follows that NUL */
	struct JobTextView {
		cvx_alignment_text const * recs;
		uint64_t const * off;
		char const * text;
	};
	bool JobTexts(cvx_job job, JobTextView & jx);      /* after Wait, once per launch.  false: the handle delivers none (throws 1 when one that should cannot) */
	/* jx: the launch's device-made text.  With it a tile that is answered with a note takes its CIGAR and MD from there
	 * (FinishJobText) and nothing walks its ops */
	void Finish(Tile & t, cvx_result const & r, uint32_t const * ops, JobRegions const * jr = 0, int index = 0, JobTextView const * jx = 0) const;
	/* what Finish leaves in the caller's Align for a tile it answers with a note, copied out of the job's text: cvx_text_reclip puts
	 * the tile's external clips on and writes pBuffer1, the MD is a memcpy; the same growth rule for pBuffer2 and the same hard
	 * error for a CIGAR beyond maxBufferLength as FinishText.  The caller has made sure of the alignment (r.status) and of the
	 * note (NmRegionsNote::Begin) */
	void FinishJobText(Tile & t, JobTextView const & jx, JobRegions const & jr, int index) const;
	/* alignments of this process that took their CIGAR and MD from the device, and alignments Finish formatted on the host */
	static void JobTextStats(long & fromDevice, long & onHost);
	void Release(cvx_job job);
	/* one line on stderr about a finished job: tiles, device stages, fill classes (CVX_LAUNCH_TRACE=1 in the dispatcher) */
	void Trace(cvx_job job, int nTiles, double serviceMs, double waitedMs) const;

	/* The text stage of a whole finished job on the device instead of one Finish per tile on the workers' cores
	 * (cvx_job_text + cvx_job_nm_profile: CIGAR, MD, the scalar fields and nmPerPosition from the ops and sequences
	 * still resident in HBM).  Text belongs to the device thread, after Wait and before Release; FinishText may run
	 * on any thread and only copies: the same Align, byte for byte, as Finish (tests/test_gpu_e2e.py, CVX_DEVICE_TEXT=1). */
	struct JobText {
		std::vector<cvx_alignment_text> out;
		std::vector<uint64_t> textOff, nmOff;
		int32_t const * nm;                /* (refPosition, readPosition, nm) triples of all tiles, in the job's page-locked memory */
		char const * text;                 /* the job's page-locked text buffer */
	};
	void Text(cvx_job job, Tile const * const * tiles, int n, JobText & jt);
	/* after Wait, for a launch that travelled through cvx_submit_windows: tiles[i]->refSeq is redirected to the characters
	 * the device decoded (cvx_job_window_refs: the job's page-locked memory, valid until Release), so that Finish -- the host
	 * text stage, which reads the reference base of every mismatch and deletion -- works on them.  false: not a window launch; throws 1 when a window launch cannot hand its characters back */
	bool WindowRefs(cvx_job job, Tile * const * tiles, int n);
	/* launches that travelled as windows of the resident genome (cvx_submit_windows), and launches that mixed windows with
	 * decoded references (their windows were materialised with cvx_genome_decode first) */
	static void WindowStats(long & windowLaunches, long & windowTiles, long & mixedLaunches);
	/* launches whose queries all travelled as segments of one read block (cvx_submit_segments), their tiles, and launches that
	 * mixed noted and plain queries (their noted ones were materialised on the host first) */
	static void ReadStats(long & notedLaunches, long & notedTiles, long & mixedLaunches);
	/* tiles Prepare() has seen in this process, and how many of them travelled as a closed form */
	static void CorridorStats(long & prepared, long & closedForm);
	void FinishText(Tile & t, cvx_result const & r, JobText const & jt, int index) const;

private:
	static void resolveSequences(Tile & t);      /* Prepare's first half: placeholders recognised, refLen / qryLen */
	cvx_job submitPacked(Tile const * tiles, int n, cvx_ladder const * ladders);      /* Submit's second half, shared with SubmitLadders */
	void fillAlign(Tile & t, cvx_alignment_text const & txt) const;
	bool noAlignment(Tile & t, cvx_result const & r) const;
	void putNote(Align & a, JobRegions const & jr, int index) const;      /* the note of tile `index`: with its checks where the job brought them */
	cvx_handle handle;
	bool twin;
	bool regions;
	bool jobText;
	bool invChecks;
	unsigned long maxMatrixMB;
	std::vector<cvx_tile> packed;
	cvx_genome genome;                     /* DeviceWindows' genome on this aligner's device (uploaded by the first launch that carries a window) */
	std::vector<unsigned long long> positions;
	std::vector<char const *> refPtrs;
	void materialiseWindows(Tile const * tiles, int n);
	/* DeviceReads: the read block of a noted launch -- every distinct read once -- and one segment per tile */
	std::vector<uint8_t> readArena;
	std::vector<uint64_t> readOffsets;
	std::vector<cvx_read_segment> segments;
	void materialiseReads(Tile const * tiles, int n);
};

/*
 * Reference windows decoded on the device inside ngmlr's worker flow (decode half).
 *
 * ngmlr expands the reference window of every alignment from its 4-bit genome on the worker's core
 * (extractReferenceSequenceForAlignment -> DecodeRefSequenceExact, reference src/AlignmentBuffer.cpp:199-223,
 * src/SequenceProvider.cpp:493-565) and hands SingleAlign the characters.  Between that call and SingleAlign the
 * caller only measures the string (strlen in the corridor builders, :112, :135).  Unless CVX_DEVICE_DECODE=0, the
 * binding (window_decode_binding.inc) allocates the same buffer, fills it with a placeholder of the same length and
 * notes (buffer, position, length) for the calling context; Prepare() recognises the buffer, the launch travels
 * through cvx_submit_windows, and the text stage -- on the host (default) or on the device (CVX_DEVICE_TEXT=1) -- reads
 * what the device decoded: the windows come back with the launch's results (cvx_job_window_refs, one byte per base) resp.
 * are read where the fill read them.  No core expands a window.  The note travels with the read:
 * fiber-local under the pool's user-level contexts, thread-local on a plain worker thread.
 */
struct DeviceWindows {
	static bool Enabled();                 /* unless CVX_DEVICE_DECODE=0 */
	/* ngmlr's encoded genome as _SequenceProvider::Init leaves it (binRef, binRefIndex nibbles, refStartPos with its upper
	 * bound): the pointers must stay valid; each aligner uploads it to its own device at its first window launch */
	static void SetGenome(void const * binRef, unsigned long long nNibbles, unsigned long long const * startTable, int nStarts);
	static bool HaveGenome();
	/* what SetGenome was given (false before it): StrippedSWHip::BatchScoreWindows uploads it once per logical device */
	static bool Genome(void const * & binRef, unsigned long long & nNibbles, unsigned long long const * & startTable, int & nStarts);
	/* buf[0 .. length) stands for DecodeRefSequenceExact(buf, position, length, 0): length - 1 characters and a NUL */
	static void Placeholder(char * buf, unsigned long long position, int length);
	static bool Lookup(char const * buf, unsigned long long & position, int & length);
};

/*
 * Alignment queries built on the device inside ngmlr's worker flow.
 *
 * ngmlr builds the query of every SingleAlign on the worker's core (AlignmentBuffer::extractReadSeq, reference
 * src/AlignmentBuffer.cpp:1515-1549: a strncpy, or computeReverseSeq's byte-at-a-time reverse complement) and between that call
 * and SingleAlign only measures the string (strlen in the corridor builders).  Unless CVX_DEVICE_READS=0, the binding
 * (read_segments_binding.inc) allocates a buffer of BufferBytes(length) and fills it with a placeholder of the same length that
 * DESCRIBES ITSELF: `length` characters no read holds (bit 7 set, a fixed sequence), the NUL, and behind the NUL the note --
 * (this buffer, the read's Seq, its length, start, length, flags).  Nothing is kept per calling context: any number of noted
 * buffers live side by side on a thread or fiber, a note ends with its buffer, and a plain string is never taken for a
 * placeholder (its first character ends the check).  Prepare() recognises the buffer, and a launch whose tiles are all noted
 * sends every distinct read once and goes through cvx_submit_segments.  flags = (isReverse != revComp), CVX_SEG_REVCOMP.
 */
struct DeviceReads {
	static bool Enabled();                 /* unless CVX_DEVICE_READS=0 */
	static int BufferBytes(int length);    /* what a buffer for a placeholder of `length` characters must hold */
	/* buf (BufferBytes(length) bytes) stands for extractReadSeq's string: length placeholder characters, a NUL, the note.
	 * readSeq (MappedRead::Seq, readLength bytes) must stay valid until the launch has been submitted. */
	static void Placeholder(char * buf, char const * readSeq, int readLength, int start, int length, int flags);
	static bool Lookup(char const * buf, char const * & readSeq, int & readLength, int & start, int & length, int & flags);
	/* the placeholder in buf replaced by the string itself, built on the host.  false: buf holds no placeholder (nothing is written) */
	static bool Materialise(char * buf);
	/* strncpy(dst, src + offset, n) for a caller that reads characters of a query after all (checkForSV,
	 * src/AlignmentBuffer.cpp:1202): from a placeholder, those n characters of the string it stands for, built on the host */
	static void CopyOut(char * dst, char const * src, int offset, int n);
};

/*
 * detectMisalignment on regions found by the device (nm_regions_note.h; CVX_CREATE_NM_REGIONS, include/cvx_align.h).
 *
 * Every alignment writes Align::nmPerPosition, 12 bytes per alignment column, for one reader: the peak finder at the top of
 * AlignmentBuffer::detectMisalignment (reference src/AlignmentBuffer.cpp:1316-1395), which keeps four or five regions.  A
 * binding that walks a note there announces itself (Announce) before the aligners are built; SharedAligner then creates its
 * handles with the flag, the binding's allocation site writes a request instead of allocating the profile, and Finish answers
 * it.  CVX_DEVICE_REGIONS=0 turns all of it off inside the same binary: plain handles, no requests, the reference's loop.
 */
/*
 * computeAlignment's retry ladder as ONE request (ladder_binding.inc, in front of the loop at src/AlignmentBuffer.cpp:292).
 *
 * The binding reaches an aligner that can take it through this interface, found with dynamic_cast on ngmlr's IAlignment *: the
 * IAlignment vtable stays as it is.  SingleLadder returns false, having done nothing, when the aligner cannot take ladders
 * right now -- the caller then runs the reference's loop; otherwise `result` is filled as SingleAlign fills it for the rung
 * reported, ret is that rung's return value (-1: its attempt failed), rung / attempts / width are cvx_job_ladder's record.
 * Hard errors throw like SingleAlign's.
 */
class LadderAligner {
public:
	virtual ~LadderAligner() {}
	virtual bool SingleLadder(char const * refSeq, char const * qrySeq, Align & result, int const externalQStart, int const externalQEnd,
			cvx_ladder const & ladder, int & ret, int & rung, int & attempts, int & width) = 0;
};

struct DeviceRegions {
	static void Announce();                /* the binding's finder site is compiled in */
	static bool Enabled();                 /* announced, unless CVX_DEVICE_REGIONS=0 */
	static bool JobText();                 /* Enabled() and CVX_JOB_TEXT=1 (default 0): the handles that deliver regions deliver CIGAR and MD too */
	/* the binding's finder site: an alignment walked `regions` regions of a note / scanned its profile */
	static void CountNote(int regions);
	static void CountProfile();
	static void Stats(long & noteAlignments, long & noteRegions, long & profileAlignments);
};

/*
 * checkForSV on the scores its job brought (inv_checks_binding.inc, inv_checks_binding_logic.h; CVX_CREATE_INV_CHECKS).
 *
 * Every region detectMisalignment keeps costs its read's context a window decode, a copy, a reverse complement and two
 * StrippedSW::SingleScore calls (reference src/AlignmentBuffer.cpp:1195-1225).  A job of a handle with the flag has scored them
 * already.  A binding whose checkForSV reads a record announces itself beside the regions binding; SharedAligner then creates its
 * handles with the flag, Finish writes the checks form of the note, the finder site offers region k's record to the checkForSV
 * call of region k.  CVX_DEVICE_INV_CHECKS=0 (or CVX_DEVICE_REGIONS=0) turns all of it off inside the same binary: handles without
 * the flag, regions-only notes, the reference's scoring.  CVX_INV_CHECKS_VERIFY=1 runs the reference's scoring beside every
 * record, compares and uses the reference's result.  One line on stderr when the process ends (announced binaries only).
 */
struct DeviceInvChecks {
	static void Announce();                /* the binding's checkForSV site is compiled in */
	static bool Enabled();                 /* announced, DeviceRegions::Enabled(), and not CVX_DEVICE_INV_CHECKS=0 */
	static bool Verify();                  /* CVX_INV_CHECKS_VERIFY=1 */
	/* checkForSV: a record was taken (scored: its two scores; else it said that no read part exists) */
	static void CountTaken(bool scored);
	/* checkForSV: the reference's own scoring ran although the binding is on */
	enum Own { kNoWindow = 0, kInconsistent = 1, kNoteWithoutChecks = 2 };
	static void CountOwn(Own why);
	static void CountVerified(bool agrees);
	/* the aligner: an alignment with regions whose launch brought no checks got a regions-only note while the binding is on */
	static void CountRegionsOnly();
	struct Counts { long scored, noRead, noWindow, inconsistent, noteWithoutChecks, verified, disagreements, regionsOnlyAlignments; };
	static Counts Stats();
};

}  // namespace Convex

#endif
