/*
 * cs_search_binding.inc -- the body tools/build_ngmlr_hip.sh inserts at the top of CS::RunBatch (reference src/CS.cpp:400-410)
 * so that the k-mer vote of the thread's whole batch runs on the MI355X (Convex::CandidateSearchHip, candidate_search_hip.h)
 * instead of read by read in CS::RunRead (src/CS.cpp:324-398).  What follows the search is RunRead's and
 * CollectResultsStd's own code path, per read and in batch order: MappedRead::s = maxHitNumber and the kCount rule for the
 * mapping quality (src/CS.cpp:221-226), the LocationScore list in the reference's order handed to AllocScores unless it
 * reaches --max-cmrs (:263-265), the "too many candidates" message (:391-393), SendToBuffer (:396).  Members it uses: the
 * thread's tmp / tmpSize list buffer, m_CurrentBatch, m_CurrentSeq, m_CurrentReadLength, m_ProcessedReads, m_Fallback.
 * The vote table of the first attempt: the reference starts a CS thread at 2^16 entries (src/CS.cpp:516, or the user's
 * --search-table-length) and adapts the size per batch from the overflows it counted (:482-489): down to 2^8 while few first
 * attempts overflow, up -- for good -- when more than 1 % do.  The size only decides when an attempt runs out of its probe
 * budget; a successful attempt returns the same list at every size (tests/test_search_cpu.py, tests/test_gpu_search.py: every
 * recorded call at 2^16 and at the size the reference had adapted to).  Two things do depend on it.  (1) WHICH reads fail:
 * the retry ladder is first + 2, + 3, ... up to 2^20, so a thread that starts at 2^19 or 2^20 (adapted up on an overflow-heavy
 * genome, or set by the user) has no further rung and reports "too many candidates" where a thread climbing from 2^16 would
 * still find a list.  The binding therefore follows the thread's own size whenever it is ABOVE 2^16 or user-set, and counts
 * m_Overflows exactly as RunRead does (a read whose first attempt overflowed: cvx_search_last_attempts), so that
 * NGM.Stats->csOverflows and DoRun's upward adaptation mean what they mean in the reference (ADVICE r4).  Below 2^16 it keeps
 * 2^16: there every ladder ends at the same most permissive rung (2^20 at 0.777), the set of failing reads is the same, and
 * following the adaptation down to 2^8 would buy two to four device round trips per call for nothing.  (2) kCount, which the
 * reference sums over the failed attempts as well: with 2^16 fewer attempts fail, so a read can stay below the
 * 0.9 (length - k + 1) that zeroes its mapping quality where the reference's adapted run crossed it.  That value is overwritten
 * by ScoreBuffer::computeMQ for every sub-read that gets scores (src/ScoreBuffer.cpp:38-45) and sub-reads without scores are
 * not looked at again (src/AlignmentBuffer.cpp:2935-2940), so no output depends on it.  Genomes of more than one table unit
 * (> 4 Gbp) keep the reference's search.
 * CS::DoRun (src/CS.cpp:422) sizes the thread's own 2^24-entry vote table through cvxHostVoteTableLen (cs_search_binding.h):
 * one entry when the device takes the votes -- 320 MB per CS thread that were allocated and written at start-up.
 */
	{
		static Convex::CandidateSearchHip * const cvxSearch = [](IRefProvider const * rp) -> Convex::CandidateSearchHip * {
			TableUnit const * unit = cvxSearchableUnit(rp);      /* cs_search_binding.h */
			if (unit == 0) return 0;
			return Convex::CandidateSearchHip::Get(Config.getKmerLength(), unit->RefTableIndex, (uint32_t const *) unit->RefTable,
					unit->cRefTableLen, (uint64_t) unit->Offset);
		}(m_RefProvider);
		if (cvxSearch != 0 && !m_Fallback) {
			static thread_local Convex::CandidateSearchHip::Batch cvxBatch;
			size_t const cvxN = m_CurrentBatch.size();
			cvxBatch.seqs.resize(cvxN);
			cvxBatch.lens.resize(cvxN);
			for (size_t i = 0; i < cvxN; ++i) {
				cvxBatch.seqs[i] = m_CurrentBatch[i]->Seq;
				cvxBatch.lens[i] = m_CurrentBatch[i]->length;
			}
			/* the first attempt's table: the user's --search-table-length when given, else the size this thread has adapted to
			 * (src/CS.cpp:482-489) but never below the 2^16 it started with -- see the note above */
			int const cvxFirstBits = Config.getCsSearchTableLength() != 0 ? c_SrchTableBitLen : (c_SrchTableBitLen > 16 ? c_SrchTableBitLen : 16);
			/* the device's ladder ends at 2^20 (the reference's own last rung, src/CS.cpp:359-364); a user's --search-table-length beyond
			 * it runs as ONE attempt at 2^20 here, where the reference runs one attempt at the size given: said once, not silently (ADVICE r5) */
			static bool const cvxClampSaid = [](int bits) { if (bits > 20) Log.Message("CandidateSearchHip: --search-table-length %d runs as 2^20 on the device (one attempt, like the reference's single attempt at the user's size)", bits); return true; }(Config.getCsSearchTableLength() != 0 ? c_SrchTableBitLen : 0);
			(void) cvxClampSaid;
			int const cvxBits = cvxFirstBits < 8 ? 8 : (cvxFirstBits > 20 ? 20 : cvxFirstBits);
			bool cvxFused = false;      /* the batch was searched and scored in one call (cs_feed_binding.inc, variant ngmlr_hip_feed) */
#ifdef CVX_CS_FEED_BINDING
#define CVX_CS_FEED_SITE 1
#include "cs_feed_binding.inc"
#undef CVX_CS_FEED_SITE
#endif
			if (!cvxFused) cvxSearch->Search(cvxBatch, m_CsSensitivity, (float) Config.getMinKmerHits(), Config.getBinSize(), cvxBits);
			static int const cvxMaxScores = Config.getMaxCMRs();
			int cvxScoresSum = 0;
			for (size_t i = 0; i < cvxN; ++i) {
				MappedRead * read = m_CurrentBatch[i];
				m_CurrentSeq = read->ReadId;
				m_CurrentReadLength = read->length;
				++m_ProcessedReads;
				int const n = cvxBatch.nCand[i];
				if (cvxBatch.attempts[i] > 1 || n < 0) ++m_Overflows;      /* the first attempt ran out of its probe budget (src/CS.cpp:359-364) */
				if (n < 0) {
					Log.Message("Couldn't find candidate for read %s (too many candidates)", read->name);
				} else {
					int max = (read->length - CS::prefixBasecount + 1) * 0.9;
					if (cvxBatch.kmerMisses[i] > max)
						read->mappingQlty = 0;
					read->s = cvxBatch.maxHit[i];
					if (2 * n > tmpSize) {
						tmpSize = 2 * n * 1.5f;
						delete[] tmp;
						tmp = new LocationScore[tmpSize];
					}
					cvx_candidate const * c = cvxBatch.cands.data() + cvxBatch.begin[i];
					for (int q = 0; q < n; ++q) {
						LocationScore * toInsert = &tmp[q];
						toInsert->Score.f = c[q].score;
						toInsert->Location.m_Location = c[q].location;
						toInsert->Location.setReverse(c[q].reverse != 0);
					}
					if (n < cvxMaxScores)
						read->AllocScores(tmp, n);
					cvxScoresSum += n;
				}
				bool cvxSent = false;
#ifdef CVX_CS_FEED_BINDING
#define CVX_CS_FEED_SITE 2
#include "cs_feed_binding.inc"
#undef CVX_CS_FEED_SITE
#endif
				if (!cvxSent) SendToBuffer(read, sw, out);
			}
			return cvxScoresSum;
		}
	}
