/*
 * cs_feed_binding.inc -- the two pieces cs_search_binding.inc includes in CS::RunBatch when CVX_CS_FEED_BINDING is defined
 * (variant ngmlr_hip_feed = ngmlr_hip_scorewin + this; tools/build_ngmlr_hip.sh), with CVX_CS_FEED_SITE saying which:
 *   1  in front of the batch's search: when CVX_CS_FEED is not 0, a genome is announced (Convex::DeviceWindows::SetGenome), the
 *      thread's scorer is a StrippedSWHip and every read of the batch is a sub-read of a group (a short read has group == 0 and
 *      keeps scoreShortRead's own window rule), the batch is searched AND scored in one device call
 *      (CandidateSearchHip::SearchAndScore: buffer_len = refMaxLen, window_lead = corridor >> 1 as ScoreBuffer::DoRun has them,
 *      src/ScoreBuffer.h:65-72, ScoreBuffer.cpp:111; max_cmrs = Config.getMaxCMRs()).  Sets cvxFused; otherwise the batch takes
 *      Search and, later, the scorer's own call, and the reason is counted for the exit line.
 *   2  per read, behind AllocScores, in place of SendToBuffer: a read whose list was handed to AllocScores and whose every
 *      candidate was scored goes to ScoreBuffer::addScoredRead (added by the build script: the scores written, Calculated set,
 *      the reference's own completion block of src/ScoreBuffer.cpp:141-162 run -- moved into a method, not restated).  A read
 *      without scores (count 0: no list, or one of max_cmrs entries and more) and a read with a candidate whose window does not
 *      decode (sw_status 1: the reference scores a buffer of N there, and that stays its code) go to SendToBuffer as ever.
 */
#if CVX_CS_FEED_SITE == 1
	{
		int cvxWhy = -1;
		StrippedSWHip * const cvxSw = dynamic_cast<StrippedSWHip *>(sw->cvxAligner());
		int const cvxBufferLen = (int) sw->cvxRefMaxLen(), cvxMaxCmrs = Config.getMaxCMRs();
		if (!cvxCsFeedOn()) cvxWhy = Convex::CandidateSearchHip::kFeedOff;
		else if (!Convex::DeviceWindows::HaveGenome()) cvxWhy = Convex::CandidateSearchHip::kFeedNoGenome;
		else if (cvxSw == 0) cvxWhy = Convex::CandidateSearchHip::kFeedScorer;
		else if (cvxBufferLen < 3 || cvxBufferLen > 2048 || cvxMaxCmrs < 1) cvxWhy = Convex::CandidateSearchHip::kFeedShape;
		else for (size_t i = 0; i < cvxN; ++i) if (m_CurrentBatch[i]->group == 0 || m_CurrentBatch[i]->length > 511) cvxWhy = Convex::CandidateSearchHip::kFeedShape;
		if (cvxWhy < 0 && cvxN > 0) {
			cvxSearch->SearchAndScore(cvxBatch, m_CsSensitivity, (float) Config.getMinKmerHits(), Config.getBinSize(), cvxBits, cvxBufferLen,
					sw->cvxCorridor() >> 1, cvxMaxCmrs);
			cvxFused = true;
		} else if (cvxN > 0) {
			Convex::CandidateSearchHip::NoteTwoCallBatch(cvxWhy);
		}
	}
#elif CVX_CS_FEED_SITE == 2
	if (cvxFused && n > 0 && read->numScores() == n) {
		float const * const cvxScores = cvxBatch.swScores.data() + cvxBatch.begin[i];
		int32_t const * const cvxStatus = cvxBatch.swStatus.data() + cvxBatch.begin[i];
		bool cvxAll = true;
		for (int q = 0; q < n; ++q) cvxAll = cvxAll && cvxStatus[q] == 0;
		if (cvxAll) {
			sw->addScoredRead(read, cvxScores);
			cvxSent = true;
		}
	}
#else
#error "CVX_CS_FEED_SITE: 1 (the batch's search) or 2 (per read, in place of SendToBuffer)"
#endif
