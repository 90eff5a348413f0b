/*
 * nm_regions_finder_binding.inc -- included by tools/build_ngmlr_hip.sh in AlignmentBuffer::detectMisalignment in front of the peak
 * finder's loop (reference src/AlignmentBuffer.cpp:1320-1395).
 *
 * The script has moved what the reference does per region -- the BED and debug prints, the midpoints, checkCount += 1, checkForSV,
 * bestResult (:1348-1383) -- into the lambda cvxRegionBody in front of this file, calls it from the reference's loop, and runs that
 * loop only when cvxNote is false.  When the aligner answered the request with a note (nm_regions_note.h), the regions are the
 * ones that loop would have found in the profile -- in its order, a run still open at the end dropped -- and the loop becomes a
 * walk over them: the four variables the body reads, then the body.  (inversionPositionShift is the reference's constant 0.)
 */
	int cvxNoteRegions = 0;
	bool const cvxNote = Convex::NmRegionsNote::IsNote(align->nmPerPosition, align->nmPerPostionLength, cvxNoteRegions);
	if (cvxNote) {
		for (int k = 0; k < cvxNoteRegions; ++k) {
			Convex::NmRegionsNote::Region const region = Convex::NmRegionsNote::At(align->nmPerPosition, k);
			startInv = region.refStart - inversionPositionShift;
			stopInv = region.refStop - inversionPositionShift;
			startInvRead = region.readStart - inversionPositionShift;
			stopInvRead = region.readStop - inversionPositionShift;
			cvxRegionBody();
		}
		startInv = stopInv = startInvRead = stopInvRead = -1;
		Convex::DeviceRegions::CountNote(cvxNoteRegions);
	} else {
		Convex::DeviceRegions::CountProfile();
	}
