/*
 * score_windows_binding.inc -- the body tools/build_ngmlr_hip.sh inserts in front of the two preparation loops of ScoreBuffer
 * (variant ngmlr_hip_scorewin), with CVX_SCORE_WINDOWS_SITE saying which:
 *   1  ScoreBuffer::DoRun (reference src/ScoreBuffer.cpp:94-124): the loop that reverse-complements the sub-read
 *      (computeReverseSeq) and expands the window (DecodeRefSequence) of each of up to 1 024 pairs, and the BatchScore behind it;
 *   2  ScoreBuffer::scoreShortRead (:245-272): the same per candidate of a short read, each followed by a SingleScore -- here one
 *      call per read over all its candidates; the sort and computeMQ behind the loop stay as they are.
 * When the scorer is a StrippedSWHip and the genome has been announced (Convex::DeviceWindows::SetGenome), the pairs travel as
 * (position, buffer length, read, strand) over the distinct reads of the call and both strings are written on the device
 * (StrippedSWHip::BatchScoreWindows); neither computeReverseSeq nor DecodeRefSequence runs here.  Sets cvxWindows, which empties the
 * reference's loop (and, at site 1, its BatchScore).  A call with a pair whose window starts at or behind GetConcatRefLen() --
 * where DecodeRefSequence returns false and the reference scores a buffer of N -- is left alone: cvxWindows stays false and the
 * reference's untouched loop handles the whole call (counted in the scorer's exit line as pairs through the string path).
 * CVX_SCORE_WINDOWS=0: nothing of this runs.
 */
#if CVX_SCORE_WINDOWS_SITE == 1
	{
		StrippedSWHip * const cvxSw = cvxScoreWindowsOn() ? dynamic_cast<StrippedSWHip *>(aligner) : 0;
		if (cvxSw != 0 && Convex::DeviceWindows::HaveGenome()) {
			std::vector<unsigned char> cvxArena;
			std::vector<unsigned long long> cvxOffsets(1, 0ull);
			std::vector<cvx_score_window> cvxPairs((size_t) iScores);
			std::map<MappedRead *, int> cvxReads;
			bool cvxDecodes = true;
			for (int i = 0; i < iScores; ++i) {
				MappedRead * const cvxRead = scores[i].read;
				std::map<MappedRead *, int>::iterator cvxAt = cvxReads.find(cvxRead);
				if (cvxAt == cvxReads.end()) {
					cvxAt = cvxReads.insert(std::make_pair(cvxRead, (int) cvxReads.size())).first;
					cvxArena.insert(cvxArena.end(), (unsigned char const *) cvxRead->Seq, (unsigned char const *) cvxRead->Seq + cvxRead->length);
					cvxArena.push_back(0);
					cvxOffsets.push_back((unsigned long long) cvxArena.size());
				}
				SequenceLocation const cvxLoc = cvxRead->Scores[scores[i].scoreId].Location;
				cvxPairs[(size_t) i].position = (uint64_t) (cvxLoc.m_Location - (corridor >> 1));
				cvxPairs[(size_t) i].buffer_len = (int32_t) refMaxLen;
				cvxPairs[(size_t) i].read = cvxAt->second;
				cvxPairs[(size_t) i].reverse = cvxLoc.isReverse() ? 1 : 0;
				cvxDecodes = cvxDecodes && cvxPairs[(size_t) i].position < (uint64_t) SequenceProvider.GetConcatRefLen();
			}
			if (cvxDecodes) {
				cvxSw->BatchScoreWindows((int) cvxReads.size(), &cvxArena[0], &cvxOffsets[0], iScores, &cvxPairs[0], m_ScoreBuffer, 0);
				cvxWindows = true;
			} else {
				cvxSw->CountStringPath(iScores);
			}
		}
	}
#elif CVX_SCORE_WINDOWS_SITE == 2
	{
		StrippedSWHip * const cvxSw = cvxScoreWindowsOn() ? dynamic_cast<StrippedSWHip *>(this->aligner) : 0;
		int const cvxN = read->numScores();
		if (cvxSw != 0 && cvxN > 0 && Convex::DeviceWindows::HaveGenome()) {
			int const cvxCorridor = (int) (0.3 * (double) read->length + 256.0);      /* the corridor this function gives a read of that length (:246) */
			std::vector<unsigned char> cvxArena((unsigned char const *) read->Seq, (unsigned char const *) read->Seq + read->length);
			cvxArena.push_back(0);
			unsigned long long const cvxOffsets[2] = { 0ull, (unsigned long long) cvxArena.size() };
			std::vector<cvx_score_window> cvxPairs((size_t) cvxN);
			bool cvxDecodes = true;
			for (int i = 0; i < cvxN; ++i) {
				cvxPairs[(size_t) i].position = (uint64_t) (read->Scores[i].Location.m_Location - (cvxCorridor >> 1));
				cvxPairs[(size_t) i].buffer_len = (int32_t) (read->length + cvxCorridor);
				cvxPairs[(size_t) i].read = 0;
				cvxPairs[(size_t) i].reverse = read->Scores[i].Location.isReverse() ? 1 : 0;
				cvxDecodes = cvxDecodes && cvxPairs[(size_t) i].position < (uint64_t) SequenceProvider.GetConcatRefLen();
			}
			if (cvxDecodes) {
				std::vector<float> cvxScores((size_t) cvxN, -1.0f);
				cvxSw->BatchScoreWindows(1, &cvxArena[0], cvxOffsets, cvxN, &cvxPairs[0], &cvxScores[0], 0);
				for (int i = 0; i < cvxN; ++i) read->Scores[i].Score.f = cvxScores[(size_t) i];
				cvxWindows = true;
			} else {
				cvxSw->CountStringPath(cvxN);
			}
		}
	}
#else
#error "CVX_SCORE_WINDOWS_SITE: 1 (ScoreBuffer::DoRun) or 2 (ScoreBuffer::scoreShortRead)"
#endif
