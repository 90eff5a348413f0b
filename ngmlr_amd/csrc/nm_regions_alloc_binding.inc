/*
 * nm_regions_alloc_binding.inc -- included by tools/build_ngmlr_hip.sh in AlignmentBuffer::computeAlignment where the reference
 * allocates Align::nmPerPosition (src/AlignmentBuffer.cpp:277-278: new PositionNM[2 * (readLength + 1)], 240 kB per 10 kb read,
 * zeroed by its constructor), in front of those two lines, which the script keeps as the else branch.
 *
 * The profile has two readers, both in detectMisalignment: the peak finder (:1316-1395) and the --stdout 3 dump (:1304-1309).
 * Where the finder walks a note (nm_regions_finder_binding.inc) and the dump is off, the buffer is a header and some thirty
 * regions with a request in its first row (nm_regions_note.h); the aligner answers it with the regions of its job and grows the
 * buffer when a tile has more.  CVX_DEVICE_REGIONS=0, or --stdout 3: the reference's allocation.
 */
			if (Convex::DeviceRegions::Enabled() && !stdoutErrorProfile) {
				align->nmPerPostionLength = Convex::NmRegionsNote::RowsFor(32);
				align->nmPerPosition = new PositionNM[align->nmPerPostionLength];
				Convex::NmRegionsNote::Request(align->nmPerPosition);
			} else
