/*
 * nm_regions_finder_binding.inc -- included by tools/build_ngmlr_hip.sh in AlignmentBuffer::detectMisalignment in front of the peak
 * finder's loop (reference src/AlignmentBuffer.cpp:1320-1395).
 *
 * The script has moved what the reference does per region -- the BED and debug prints, the midpoints, checkCount += 1, checkForSV,
 * bestResult (:1348-1383) -- into the lambda cvxRegionBody in front of this file, calls it from the reference's loop, and runs that
 * loop only when cvxNote is false.  When the aligner answered the request with a note (nm_regions_note.h), the regions are the
 * ones that loop would have found in the profile -- in its order, a run still open at the end dropped -- and the loop becomes a
 * walk over them: the four variables the body reads, then the body.  (inversionPositionShift is the reference's constant 0.)
 *
 * A binary whose checkForSV reads check records (CVX_INV_CHECKS_BINDING, inv_checks_binding.inc) offers region k's record -- from
 * the checks form of the note -- to the checkForSV call cvxRegionBody() makes for region k, through the AlignmentBuffer's own
 * cvxInvCheck, and withdraws it when the body returns (Convex::InvCheckOffer).  A regions-only note is offered as such; the
 * reference's loop offers nothing.  Nothing is offered under pacbioDebug and --stdout 4, whose output only the reference's
 * scoring path produces, or when the binding is off (CVX_DEVICE_INV_CHECKS=0).  A test binary without a device fills the record in
 * here, from the host rule (CVX_INV_CHECKS_CPU_SOURCE, tests/cpp/inv_checks_cpu_source.h).
 */
	int cvxNoteRegions = 0;
	bool const cvxNoteOnly = Convex::NmRegionsNote::IsNote(align->nmPerPosition, align->nmPerPostionLength, cvxNoteRegions);
	bool const cvxNoteChecks = !cvxNoteOnly && Convex::NmRegionsNote::IsChecksNote(align->nmPerPosition, align->nmPerPostionLength, cvxNoteRegions);
	bool const cvxNote = cvxNoteOnly || cvxNoteChecks;
	if (cvxNote) {
#ifdef CVX_INV_CHECKS_BINDING
		bool const cvxOffer = Convex::DeviceInvChecks::Enabled() && !pacbioDebug && !printInvCandidateFa;
#endif
		for (int k = 0; k < cvxNoteRegions; ++k) {
			Convex::NmRegionsNote::Region const region = Convex::NmRegionsNote::At(align->nmPerPosition, k);
			startInv = region.refStart - inversionPositionShift;
			stopInv = region.refStop - inversionPositionShift;
			startInvRead = region.readStart - inversionPositionShift;
			stopInvRead = region.readStop - inversionPositionShift;
#ifdef CVX_INV_CHECKS_BINDING
			if (cvxOffer) {
				bool cvxHaveCheck = cvxNoteChecks;
				Convex::NmRegionsNote::Check cvxCheck = { 0.0f, 0.0f, 0, 0 };
				if (cvxNoteChecks) cvxCheck = Convex::NmRegionsNote::CheckAt(align->nmPerPosition, cvxNoteRegions, k);
#ifdef CVX_INV_CHECKS_CPU_SOURCE
				else { cvxCheck = CVX_INV_CHECKS_CPU_SOURCE(region, readPartSeq, alignedInterval->onRefStart, align->PositionOffset); cvxHaveCheck = true; }
#endif
				if (cvxHaveCheck) {
					Convex::InvCheckOffer const cvxOffered(cvxInvCheck, cvxCheck.scoreFwd, cvxCheck.scoreRev, cvxCheck.status);
					cvxRegionBody();
				} else {
					Convex::InvCheckOffer const cvxOffered(cvxInvCheck);
					cvxRegionBody();
				}
			} else
#endif
			cvxRegionBody();
		}
		startInv = stopInv = startInvRead = stopInvRead = -1;
		Convex::DeviceRegions::CountNote(cvxNoteRegions);
	} else {
		Convex::DeviceRegions::CountProfile();
	}
