/*
 * inv_checks_binding_logic.h -- what AlignmentBuffer::checkForSV does with a check record its job brought (inv_checks_binding.inc,
 * included by tools/build_ngmlr_hip.sh), as plain functions: no HIP, no ngmlr, no library header -- tests/cpp/inv_note_test.cpp
 * holds them to hand-written cases and to the calls recorded from the unmodified reference (tests/golden/inv_checks_test_3.npz).
 *
 * The reference (src/AlignmentBuffer.cpp:1158-1265) decides three things before it scores anything, all of them cheap:
 *   inversionLength > 10                                                         else nothing happens: "too short" (:1174, :1259)
 *   50 <= inversionMidpointOnRead && inversionMidpointOnRead + 50 < strlen(read) else "Skipping", SV_NONE (:1201, :1238)
 * and only then decodes a window, copies and reverses the read part and scores twice.  A record (cvx_inv_check, include/cvx_align.h)
 * carries the status the device found by the same rule and, where it scored, the two scores.  The site states the rule ONCE more,
 * here, in the reference's own types, and takes a record only where both agree; everything else is scored by the reference's code
 * as it stands, and counted.
 */
#ifndef INV_CHECKS_BINDING_LOGIC_H
#define INV_CHECKS_BINDING_LOGIC_H

#include <stdint.h>

namespace Convex {

/* a record's status: the values of CVX_CHECK_* (convex_align_hip.cpp asserts that they are) */
enum { kInvCheckScored = 0, kInvCheckTooShort = 1, kInvCheckNoRead = 2, kInvCheckNoWindow = 3 };

int const kInvReadCheckLength = 50;       /* readCheckLength (:1164) */
int const kInvMinInversionLength = 10;    /* minInversionLength (:1170) */

/* The site's own cheap preconditions, in the reference's arithmetic: the midpoint is a uloc, the int constant and strlen's int are
 * converted to it (:1201).  -> what the reference is about to do: kInvCheckTooShort (nothing), kInvCheckNoRead (skip) or
 * kInvCheckScored (score). */
inline int inv_check_site_class(int const inversionLength, uint64_t const midpointOnRead, int const fullReadSeqLength) {
	if (!(inversionLength > kInvMinInversionLength)) return kInvCheckTooShort;
	uint64_t const half = (uint64_t) (int64_t) kInvReadCheckLength;
	if (half <= midpointOnRead && (midpointOnRead + half) < (uint64_t) (int64_t) fullReadSeqLength) return kInvCheckScored;
	return kInvCheckNoRead;
}

/* what checkForSV does with a record */
enum InvCheckOutcome {
	kInvOutcomeOutside = 0,         /* inversionLength <= 10: the branch is not entered, no record is looked at */
	kInvOutcomeTakeScores,          /* SCORED on both sides: the record's two scores, then the reference's decision */
	kInvOutcomeNoRead,              /* NO_READ on both sides: SV_NONE, as the reference's "Skipping" branch leaves it */
	kInvOutcomeOwnNoWindow,         /* the device's window did not decode: the reference's own path scores against its zeroed buffer */
	kInvOutcomeOwnInconsistent      /* the record disagrees with the site (TOO_SHORT inside the branch included): the reference's own path */
};

inline InvCheckOutcome inv_check_outcome(int const recordStatus, int const inversionLength, uint64_t const midpointOnRead, int const fullReadSeqLength) {
	int const site = inv_check_site_class(inversionLength, midpointOnRead, fullReadSeqLength);
	if (site == kInvCheckTooShort) return kInvOutcomeOutside;
	if (recordStatus == kInvCheckScored && site == kInvCheckScored) return kInvOutcomeTakeScores;
	if (recordStatus == kInvCheckNoRead && site == kInvCheckNoRead) return kInvOutcomeNoRead;
	if (recordStatus == kInvCheckNoWindow && site == kInvCheckScored) return kInvOutcomeOwnNoWindow;
	return kInvOutcomeOwnInconsistent;
}

/* What the finder site makes available to the checkForSV call of one region, as a member of the caller's AlignmentBuffer (each
 * read context owns its AlignmentBuffer; nothing is kept per thread -- a carrier thread runs many contexts). */
struct InvCheckSlot {
	enum State { kNone = 0,         /* the reference's loop, or the binding is off: checkForSV as it stands */
		kNoteWithoutChecks,             /* a regions-only note while the binding is on: the reference's path, counted */
		kRecord };                      /* the record of the region this call is about */
	int state;
	float scoreFwd, scoreRev;
	int32_t status;
	InvCheckSlot() : state(kNone), scoreFwd(0.0f), scoreRev(0.0f), status(kInvCheckTooShort) {}
};

/* makes a slot's content last exactly as long as one cvxRegionBody() call */
struct InvCheckOffer {
	InvCheckSlot & slot;
	InvCheckOffer(InvCheckSlot & s, float const scoreFwd, float const scoreRev, int32_t const status) : slot(s) {
		slot.state = InvCheckSlot::kRecord; slot.scoreFwd = scoreFwd; slot.scoreRev = scoreRev; slot.status = status;
	}
	explicit InvCheckOffer(InvCheckSlot & s) : slot(s) { slot.state = InvCheckSlot::kNoteWithoutChecks; }
	~InvCheckOffer() { slot = InvCheckSlot(); }
private:
	InvCheckOffer(InvCheckOffer const &);
	InvCheckOffer & operator=(InvCheckOffer const &);
};

/* verify mode: does the reference's own run of a call agree with what the record would have given?  ownScored: the reference
 * reached its two SingleScore calls; the scores are compared by their bits */
inline bool inv_check_agrees(InvCheckOutcome const outcome, int const svTypeFromRecord, float const recordFwd, float const recordRev,
		int const svTypeOwn, bool const ownScored, float const ownFwd, float const ownRev) {
	if (svTypeFromRecord != svTypeOwn) return false;
	if (outcome == kInvOutcomeNoRead) return !ownScored;
	if (outcome != kInvOutcomeTakeScores || !ownScored) return false;
	union { float f; uint32_t u; } a, b, c, d;
	a.f = recordFwd; b.f = ownFwd; c.f = recordRev; d.f = ownRev;
	return a.u == b.u && c.u == d.u;
}

}  // namespace Convex

#endif
