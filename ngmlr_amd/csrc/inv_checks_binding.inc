/*
 * inv_checks_binding.inc -- included twice by tools/build_ngmlr_hip.sh in AlignmentBuffer::checkForSV (reference
 * src/AlignmentBuffer.cpp:1158-1265), inside `if (inversionLength > minInversionLength)`.
 *
 * The script has moved the reference's decision (:1230-1236: SV_INVERSION, SV_TRANSLOCATION or nothing, from the two scores)
 * into the lambda cvxDecide in front of site 1, with `minScore` (:1221) in front of it, and calls it from the reference's own
 * path, whose scores it notes in cvxOwnFwd / cvxOwnRev.  cvxInvCheck is the member the script adds to AlignmentBuffer; the finder
 * site (nm_regions_finder_binding.inc) fills it for the one call it is about.
 *
 *   site 1, at the top of the branch.  With a record that agrees with the site's own preconditions (inv_checks_binding_logic.h):
 *           SCORED   the record's scores, the decision, return -- no buffer, no decode, no copy, no reverse complement, no scorer;
 *           NO_READ  SV_NONE, return (the reference's "Skipping" branch, without its decode).
 *           Everything else -- no window on the device, a record that disagrees, a note without checks -- falls through to the
 *           reference's path as it stands, counted.  CVX_INV_CHECKS_VERIFY=1: the record's result is kept aside and the
 *           reference's path runs as well.
 *   site 2, behind the reference's scoring (in front of its delete[]s): verify mode compares svType and the bits of both scores;
 *           the reference's result stands.
 *
 * What follows the branch's work in the reference (:1248-1258) only logs under pacbioDebug, and under pacbioDebug or --stdout 4 the
 * finder site offers no record.
 */
#if CVX_INV_CHECKS_SITE == 1
		bool cvxOwnScored = false, cvxVerifying = false;
		float cvxOwnFwd = 0.0f, cvxOwnRev = 0.0f;
		int cvxFromRecord = SV_NONE;
		Convex::InvCheckOutcome cvxOutcome = Convex::kInvOutcomeOutside;
		if (cvxInvCheck.state == Convex::InvCheckSlot::kNoteWithoutChecks) {
			Convex::DeviceInvChecks::CountOwn(Convex::DeviceInvChecks::kNoteWithoutChecks);
		} else if (cvxInvCheck.state == Convex::InvCheckSlot::kRecord) {
			cvxOutcome = Convex::inv_check_outcome(cvxInvCheck.status, inversionLength, (uint64_t) inversionMidpointOnRead, (int) strlen(fullReadSeq));
			if (cvxOutcome == Convex::kInvOutcomeTakeScores || cvxOutcome == Convex::kInvOutcomeNoRead) {
				if (cvxOutcome == Convex::kInvOutcomeTakeScores) cvxDecide(cvxInvCheck.scoreFwd, cvxInvCheck.scoreRev);
				Convex::DeviceInvChecks::CountTaken(cvxOutcome == Convex::kInvOutcomeTakeScores);
				if (!Convex::DeviceInvChecks::Verify()) return svType;
				cvxVerifying = true;
				cvxFromRecord = svType;
				svType = SV_NONE;
			} else {
				Convex::DeviceInvChecks::CountOwn(cvxOutcome == Convex::kInvOutcomeOwnNoWindow ? Convex::DeviceInvChecks::kNoWindow : Convex::DeviceInvChecks::kInconsistent);
			}
		}
#elif CVX_INV_CHECKS_SITE == 2
		if (cvxVerifying) {
			Convex::DeviceInvChecks::CountVerified(Convex::inv_check_agrees(cvxOutcome, cvxFromRecord, cvxInvCheck.scoreFwd, cvxInvCheck.scoreRev,
					svType, cvxOwnScored, cvxOwnFwd, cvxOwnRev));
		}
#endif
