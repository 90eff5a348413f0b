#!/bin/bash
# tools/build_ngmlr_hip.sh -- the drop-in, end to end: builds the reference's own ngmlr
# (its CMake, its sources, in a fresh /tmp copy) with exactly the change INTEGRATION.md
# describes -- Convex::ConvexAlignHip constructed instead of Convex::ConvexAlignFast at
# src/AlignmentBuffer.h:355, and in scalar-twin mode instead of Convex::ConvexAlign in the --nosse
# branch at :346 -- linked against this repository's libcvxalign.so.  The
# binary lands in oracle/_ref/ngmlr_hip (git-ignored build artefact, travels to the GPU
# box like the .so files); tests/test_gpu_e2e.py runs it on the reference's test data and
# compares the SAM with the unmodified reference's output (tests/golden/test_*.sam).
# Needs /root/reference, cmake, zlib (this container only).  No reference source enters
# the repository.
set -euo pipefail
HERE="$(cd "$(dirname "$0")" && pwd)"
REPO="$(dirname "$HERE")"
make -s -C "$REPO/ngmlr_amd/csrc"
WORK="$(mktemp -d /tmp/ngmlr_hip.XXXXXX)"
mkdir -p "$REPO/oracle/_ref"
# build_variant OUT_NAME ALIGNER_CLASS: the class constructed at src/AlignmentBuffer.h:355
#   ngmlr_hip          Convex::ConvexAlignHip  one private aligner per worker, one tile per launch
#   ngmlr_hip_batched  Convex::SharedAligner   all -t N workers share one BatchingAligner per device
#   ngmlr_hip_full     Convex::SharedAligner + StrippedSWHip at NGM::CreateAlignment (src/NGM.cpp:355): alignment AND
#                      sub-read scoring on the device
#                      and the SAM records through cvx_sam_record_text (src/SAMWriter.cpp:87)
#   ngmlr_sam          the reference's own CPU aligners; only SAMWriter::DoWriteReadGeneric goes through cvx_sam_record_text
#                      (runs without a GPU: tests/test_sam_cpu.py)
#   ngmlr_hip_pool     ngmlr_hip_full + Convex::AlignPool: processLongReadLIS / processShortRead run on K >> t alignment
#                      contexts instead of on the CS thread (align_pool.h; SURVEY 8 f1's second half), the main loop polls
#                      for the end of the run every 20 ms instead of every 2 s, SAM buffers flush at 256 kB instead of 10 MB (thousands of contexts each own one)
#   ngmlr_hip_all      ngmlr_hip_pool + the candidate search of every CS thread's batch on the device (Convex::CandidateSearchHip,
#                      cs_search_binding.inc at the top of CS::RunBatch, src/CS.cpp:400): alignment, sub-read scoring, k-mer vote
#                      and SAM records on the drop-ins (SURVEY 8 f1 + f2 + f3 + f4's search half)
#                      -- and the k-mer table itself built by cvx_index_build (index_build_binding.inc in CompactPrefixTable::CreateTable)
#   ngmlr_hip_checks   ngmlr_hip_all + the interval check (overlapCheckAligner, src/AlignmentBuffer.h:368) and the inversion check
#                      (lqCheckAligner, src/AlignmentBuffer.cpp:1217) scored on the device: Convex::SharedScorer proxies in place of
#                      their private StrippedSW, one BatchingScorer per device (batching_scorer.h); CVX_CHECK_SCORER=0 puts the
#                      reference's StrippedSW back at run time (tests/test_gpu_e2e_checks.py)
#   ngmlr_hip_scorewin ngmlr_hip_all + the scoring calls of ScoreBuffer::DoRun and scoreShortRead as windows of the resident genome
#                      (score_windows_binding.inc: StrippedSWHip::BatchScoreWindows, no computeReverseSeq / DecodeRefSequence on the CS
#                      thread); CVX_SCORE_WINDOWS=0 keeps the string path inside the same binary (tests/test_gpu_e2e_scorewin.py)
#   ngmlr_hip_feed     ngmlr_hip_scorewin + a CS batch of sub-reads searched AND scored in one device call (cs_feed_binding.inc inside
#                      cs_search_binding.inc: CandidateSearchHip::SearchAndScore, ScoreBuffer::addScoredRead over the reference's own
#                      completion block); CVX_CS_FEED=0 keeps the two calls inside the same binary (tests/test_gpu_e2e_feed.py)
#   ngmlr_hip_readseg  ngmlr_hip_all + the query of every alignment tile as a segment of the launch's read block, written on the device
#                      (read_segments_binding.inc at the top of the Interval overload of extractReadSeq, Convex::DeviceReads::CopyOut
#                      in checkForSV); CVX_DEVICE_READS=0 restores the reference's strings inside the same binary (tests/test_gpu_e2e_readseg.py)
#   ngmlr_index_cpu    the reference's CPU code with only that table builder bound: the table file it writes against the unmodified
#                      binary's, without a GPU (tests/test_index_cpu.py)
#   ngmlr_pool_cpu     the reference's CPU aligners + the same pool: the pool's own correctness without a GPU (tests/test_pool_cpu.py)
#   ngmlr_hip_regions  ngmlr_hip_all + detectMisalignment on the regions its job found: a request instead of the nmPerPosition profile where
#                      computeAlignment allocates it, the peak finder's loop as a walk over the aligner's note (nm_regions_*_binding.inc,
#                      ngmlr_amd/csrc/nm_regions_note.h; CVX_DEVICE_REGIONS=0 restores the profile inside the same binary)
#   ngmlr_regions_cpu  the same two insertions around the reference's CPU aligner (tests/cpp/regions_cpu_aligner.h), no GPU
#   ngmlr_hip_ladder   ngmlr_hip_regions + computeAlignment's retry loop as ONE request (ladder_binding.inc in front of the loop at
#                      src/AlignmentBuffer.cpp:292, which stays as the fallback; Convex::LadderAligner, found with dynamic_cast): the
#                      dispatcher gathers ladder launches, the device climbs; CVX_DEVICE_LADDER=0 restores ngmlr_hip_regions' behaviour
#                      inside the same binary (tests/test_gpu_e2e_ladder.py)
#   ngmlr_ladder_cpu   the same insertion around the reference's CPU aligner (tests/cpp/ladder_cpu_aligner.h), no GPU
#                      (tests/test_ladder_binding_cpu.py)
#   ngmlr_hip_invchecks ngmlr_hip_regions + checkForSV on the two scores its job brought: handles with CVX_CREATE_INV_CHECKS, the checks form of
#                      the note (nm_regions_note.h), region k's record offered by the finder's walk to the checkForSV call of region k
#                      (a member the script adds to AlignmentBuffer), and in checkForSV the record's scores in front of the reference's
#                      decision, which the script moves into a lambda both paths call (inv_checks_binding.inc, inv_checks_binding_logic.h);
#                      CVX_DEVICE_INV_CHECKS=0 restores ngmlr_hip_regions' behaviour inside the same binary, CVX_INV_CHECKS_VERIFY=1 runs the
#                      reference's scoring beside every record and compares (tests/test_gpu_e2e_invchecks.py).  Nobody's default.
#   ngmlr_invchecks_cpu ngmlr_regions_cpu + the same insertions, the records filled in at the finder site from the host rule
#                      (tests/cpp/inv_checks_cpu_source.h), no GPU (tests/test_inv_checks_binding_cpu.py)
#   ngmlr_pool_parked  the same with a park / wake of the read's user-level context in front of every SingleAlign
#                      (tests/cpp/parking_cpu_aligner.h): the fiber runtime under ngmlr's own long-read stage, no GPU
#   ngmlr_ref          (nothing changed)       the unmodified reference, for wall-clock comparison only
build_variant() {
local OUT_NAME=$1 CLASS=$2 SCORER=${3:-} SAM=${4:-} POOL=${5:-} SEARCH=${6:-} INDEX=${7:-} CHECKS=${8:-} SCOREWIN=${9:-} FEED=${10:-} READSEG=${11:-} REGIONS=${12:-} LADDER=${13:-} INVCHECKS=${14:-}
local T="$WORK/$OUT_NAME"
cp -r /root/reference "$T"
if [ "$CLASS" != "unmodified" ]; then
python3 - "$T" "$REPO" "$CLASS" "$SCORER" "$SAM" "$POOL" "$SEARCH" "$INDEX" "$CHECKS" "$SCOREWIN" "$FEED" "$READSEG" "$REGIONS" "$LADDER" "$INVCHECKS" <<'PY'
import re, sys
T, REPO, CLASS, SCORER, SAM, POOL, SEARCH, INDEX, CHECKS = sys.argv[1], sys.argv[2], sys.argv[3], sys.argv[4], sys.argv[5], sys.argv[6], sys.argv[7], sys.argv[8], sys.argv[9]
SCOREWIN = sys.argv[10]
FEED = sys.argv[11]
READSEG = sys.argv[12]
REGIONS = sys.argv[13]
LADDER = sys.argv[14]
INVCHECKS = sys.argv[15]
def sub1(s, old, new, what):
    assert s.count(old) == 1, (what, s.count(old))
    return s.replace(old, new, 1)
if CHECKS:
    # the interval and inversion checks through Convex::SharedScorer (ngmlr_amd/csrc/batching_scorer.h)
    p = T + '/src/AlignmentBuffer.h'
    s = open(p).read()
    s = sub1(s, '#include "StrippedSW.h"', '#include "StrippedSW.h"\n#include "batching_scorer.h"', 'AlignmentBuffer.h include (checks)')
    s = sub1(s, 'overlapCheckAligner = new StrippedSW();', 'overlapCheckAligner = new Convex::SharedScorer(Convex::SharedScorer::kIntervalCheck);', 'interval check')
    open(p, 'w').write(s)
    p = T + '/src/AlignmentBuffer.cpp'
    s = open(p).read()
    s = sub1(s, 'IAlignment * lqCheckAligner = new StrippedSW();', 'IAlignment * lqCheckAligner = new Convex::SharedScorer(Convex::SharedScorer::kInversionCheck);', 'inversion check')
    open(p, 'w').write(s)
if INDEX or (INVCHECKS and 'RegionsCpu' in CLASS):
    # (the accessor alone where only tests/cpp/inv_checks_cpu_source.h reads the genome)
    p = T + '/src/SequenceProvider.h'
    s = open(p).read()
    s = sub1(s, '\tChromosome getChrStart(uloc const position);\n', '\tChromosome getChrStart(uloc const position);\n\t/* the 4-bit genome as Init built it (read access for cvx_index_build) */\n'
             '\tchar const * cvxBinRef() const { return binRef; }\n', 'SequenceProvider.h accessor')
    open(p, 'w').write(s)
if INDEX:
    # the k-mer table built by cvx_index_build (ngmlr_amd/csrc/index_build_binding.inc at the top of CompactPrefixTable::CreateTable)
    p = T + '/src/PrefixTable.cpp'
    s = open(p).read()
    s = sub1(s, '#include "PrefixTable.h"', '#include "PrefixTable.h"\n#include <vector>\n#include <stdlib.h>\n#include <string.h>\n#include <stdint.h>\n#include "cvx_align.h"', 'PrefixTable.cpp includes')
    s = sub1(s, 'void CompactPrefixTable::CreateTable(uint const length) {\n', 'void CompactPrefixTable::CreateTable(uint const length) {\n#include "index_build_binding.inc"\n', 'CompactPrefixTable::CreateTable')
    open(p, 'w').write(s)
if INDEX and POOL:
    # the reference window of an alignment decoded on the device (CVX_DEVICE_DECODE=0 turns it off; ngmlr_amd/csrc/window_decode_binding.inc,
    # Convex::DeviceWindows in convex_align_hip.h): the encoded genome is announced where _SequenceProvider::Init has finished it
    p = T + '/src/SequenceProvider.cpp'
    s = open(p).read()
    s = sub1(s, '#include "SequenceProvider.h"', '#include "SequenceProvider.h"\n#include "convex_align_hip.h"', 'SequenceProvider.cpp include')
    s = sub1(s, '\trefStartPos[j] = refStartPos[j - 1] + SequenceProvider.GetRefLen(refCount - 1) + 1000;\n',
             '\trefStartPos[j] = refStartPos[j - 1] + SequenceProvider.GetRefLen(refCount - 1) + 1000;\n'
             '\tConvex::DeviceWindows::SetGenome(binRef, (unsigned long long) binRefIndex, refStartPos, j + 1);\n', 'SequenceProvider::Init genome')
    open(p, 'w').write(s)
    p = T + '/src/AlignmentBuffer.cpp'
    s = open(p).read()
    s = sub1(s, 'char const * const AlignmentBuffer::extractReferenceSequenceForAlignment(Interval const*& interval, int & refSeqLength) {\n',
             'char const * const AlignmentBuffer::extractReferenceSequenceForAlignment(Interval const*& interval, int & refSeqLength) {\n#include "window_decode_binding.inc"\n', 'extractReferenceSequenceForAlignment')
    open(p, 'w').write(s)
if READSEG:
    # the query of an alignment tile as a segment of the launch's read block (ngmlr_amd/csrc/read_segments_binding.inc,
    # Convex::DeviceReads in convex_align_hip.h, which AlignmentBuffer.h includes for every device variant)
    assert CLASS != 'cpu'
    p = T + '/src/AlignmentBuffer.cpp'
    s = open(p).read()
    s = sub1(s, '\t\tInterval const * interval, MappedRead* read,\n\t\tbool const revComp) {\n', '\t\tInterval const * interval, MappedRead* read,\n\t\tbool const revComp) {\n#include "read_segments_binding.inc"\n', 'extractReadSeq (Interval overload)')
    s = sub1(s, 'strncpy(readSeq, fullReadSeq + inversionMidpointOnRead - readCheckLength, readCheckLength * 2);',
             'Convex::DeviceReads::CopyOut(readSeq, fullReadSeq, inversionMidpointOnRead - readCheckLength, readCheckLength * 2);', 'checkForSV')
    open(p, 'w').write(s)
if REGIONS:
    # detectMisalignment on the regions the aligner found (ngmlr_amd/csrc/nm_regions_note.h, Convex::DeviceRegions in convex_align_hip.h;
    # CVX_DEVICE_REGIONS=0 turns it off): a request instead of the profile's buffer where computeAlignment allocates it
    # (nm_regions_alloc_binding.inc, the reference's two lines kept as its else branch), and the peak finder's loop as a walk over the
    # note (nm_regions_finder_binding.inc) -- what the reference does per region moved, as it stands, into a lambda both forms call
    assert CLASS != 'cpu'
    p = T + '/src/AlignmentBuffer.cpp'
    s = open(p).read()
    m = re.search(r'^([ \t]*)align->nmPerPostionLength = \(readLength \+ 1\) \* 2;\n[ \t]*align->nmPerPosition = new PositionNM\[align->nmPerPostionLength\];\n', s, re.M)
    assert m and len(re.findall(r'\balign->nmPerPosition = new PositionNM\[', s)) == 1, 'profile allocation'
    s = s[:m.start()] + '#include "nm_regions_alloc_binding.inc"\n' + m.group(1) + '{\n' + m.group(0) + m.group(1) + '}\n' + s[m.end():]
    first, last = 'if (stdoutInversionBed) {\n', 'bestInversionMidpointOnRead = inversionMidpointOnRead;\n'
    assert s.count(first) == 1 and s.count(last) == 1, 'region body'
    a = s.rindex('\n', 0, s.index(first)) + 1
    b = s.index('}\n', s.index(last)) + 2
    body = s[a:b]
    s = s[:a] + '\t\t\t\t\tcvxRegionBody();\n' + s[b:]
    s = sub1(s, '\tfor (int i = 0; i < align->alignmentLength /*&& result == SV_NONE*/; ++i) {\n',
             '\tauto cvxRegionBody = [&]() {\n' + body + '\t};\n#include "nm_regions_finder_binding.inc"\n'
             '\tfor (int i = 0; !cvxNote && i < align->alignmentLength /*&& result == SV_NONE*/; ++i) {\n', 'peak finder loop')
    open(p, 'w').write(s)
    # (the CPU wrapper stands only in the SSE branch: under --nosse the reference's own scalar aligner is constructed, which knows no
    # request, so nothing is announced there and the reference's allocation and loop run)
    p = T + '/src/AlignmentBuffer.h'
    s = open(p).read()
    s = sub1(s, '\t\tif (Config.getNoSSE()) {\n', ('\t\tif (%s) Convex::DeviceRegions::Announce();      /* cvx: this binary\'s detectMisalignment walks a note */\n\t\tif (Config.getNoSSE()) {\n'
             % ('!Config.getNoSSE()' if 'RegionsCpu' in CLASS else 'true')), 'AlignmentBuffer ctor (regions)')
    open(p, 'w').write(s)
if INVCHECKS:
    # checkForSV on the scores its job brought (ngmlr_amd/csrc/inv_checks_binding.inc and inv_checks_binding_logic.h, Convex::DeviceInvChecks in
    # convex_align_hip.h; CVX_DEVICE_INV_CHECKS=0 turns it off): the reference's decision (src/AlignmentBuffer.cpp:1230-1236) moved, as it
    # stands, into a lambda at the top of the branch -- with the constant it reads (:1221) -- which the reference's path calls where the
    # lines stood and the binding calls on a record's scores; the finder's walk (REGIONS, above) offers the records through a member
    assert REGIONS
    p = T + '/src/AlignmentBuffer.cpp'
    s = open(p).read()
    a = s.index('int AlignmentBuffer::checkForSV(')
    b = s.index('int AlignmentBuffer::detectMisalignment(')
    f = s[a:b]
    first, last = '\t\t\tif ((scoreRev / scoreFwd) > Config.getInvScoreRatio() && scoreRev > minScore) {\n', '\t\t\t\tsvType = SV_TRANSLOCATION;\n\t\t\t}\n'
    assert f.count(first) == 1 and f.count(last) == 1, 'checkForSV decision'
    d0, d1 = f.index(first), f.index(last) + len(last)
    assert d0 < d1
    decision = f[d0:d1]
    f = f[:d0] + '\t\t\tcvxOwnScored = true; cvxOwnFwd = scoreFwd; cvxOwnRev = scoreRev;\n\t\t\tcvxDecide(scoreFwd, scoreRev);\n' + f[d1:]
    m = re.search(r'^[ \t]*static const float minScore = [^;\n]*;\n', f, re.M)
    assert m and f.count('static const float minScore =') == 1, 'checkForSV minScore'
    min_score = m.group(0)
    f = f[:m.start()] + f[m.end():]
    f = sub1(f, '\tif (inversionLength > minInversionLength) {\n', '\tif (inversionLength > minInversionLength) {\n' + min_score +
             '\t\tauto cvxDecide = [&](float const scoreFwd, float const scoreRev) {\n' + decision + '\t\t};\n'
             '#define CVX_INV_CHECKS_SITE 1\n#include "inv_checks_binding.inc"\n#undef CVX_INV_CHECKS_SITE\n', 'checkForSV branch')
    f = sub1(f, '\t\tdelete[] refSeq;\n\t\trefSeq = 0;\n\t\tdelete[] readSeq;\n', '#define CVX_INV_CHECKS_SITE 2\n#include "inv_checks_binding.inc"\n#undef CVX_INV_CHECKS_SITE\n'
             '\t\tdelete[] refSeq;\n\t\trefSeq = 0;\n\t\tdelete[] readSeq;\n', 'checkForSV end of scoring')
    s = s[:a] + f + s[b:]
    open(p, 'w').write(s)
    p = T + '/src/AlignmentBuffer.h'
    s = open(p).read()
    m = re.search(r'^[ \t]*int checkForSV\([^;]*;\n', s, re.M)
    assert m and len(re.findall(r'\bint checkForSV\(', s)) == 1, 'checkForSV declaration'
    s = s[:m.end()] + '\t/* cvx (nm_regions_finder_binding.inc, inv_checks_binding.inc): the check record of the region the next checkForSV call is about */\n\tConvex::InvCheckSlot cvxInvCheck;\n' + s[m.end():]
    s = sub1(s, 'Convex::DeviceRegions::Announce();', 'Convex::DeviceRegions::Announce(), Convex::DeviceInvChecks::Announce();', 'AlignmentBuffer ctor (inversion checks)')
    open(p, 'w').write(s)
if LADDER:
    # computeAlignment's retry loop as one request to a Convex::LadderAligner (ngmlr_amd/csrc/ladder_binding.inc and
    # ladder_binding_logic.h): `corridor` kept as it was passed, in front of the clamp, and the binding in front of the loop, which
    # stays as it stands
    assert CLASS != 'cpu'
    p = T + '/src/AlignmentBuffer.cpp'
    s = open(p).read()
    s = sub1(s, '\t\t\tint const maxCorridorSize = refSeqLen * 2;\n', '\t\t\tint const cvxLadderCorridor = corridor;      /* cvx: before the clamp (ladder_binding.inc) */\n'
             '\t\t\tint const maxCorridorSize = refSeqLen * 2;\n', 'corridor clamp')
    s = sub1(s, '\t\t\tint corridorMultiplier = 1;\n\t\t\twhile (!validAlignment\n', '\t\t\tint corridorMultiplier = 1;\n#include "ladder_binding.inc"\n\t\t\twhile (!validAlignment\n', 'retry loop')
    open(p, 'w').write(s)
if SEARCH:
    # the k-mer vote of a CS thread's batch on the device (ngmlr_amd/csrc/candidate_search_hip.h, cs_search_binding.inc)
    p = T + '/src/PrefixTable.h'
    s = open(p).read()
    s = sub1(s, '\tstatic int maxPrefixFreq;\n', '\tstatic int maxPrefixFreq;\n\t/* read access to the table units for the device search (what GetRefEntry reads) */\n'
             '\tTableUnit const * cvxUnits(uint & count) const { count = m_UnitCount; return m_Units; }\n', 'PrefixTable.h accessor')
    open(p, 'w').write(s)
    p = T + '/src/CS.cpp'
    s = open(p).read()
    s = sub1(s, '#include "AlignmentBuffer.h"', '#include "AlignmentBuffer.h"\n#include "cs_search_binding.h"', 'CS include (search)')
    s = sub1(s, 'int x_SrchTableLen = (int) pow(2, x_SrchTableBitLen);', 'int x_SrchTableLen = cvxHostVoteTableLen(NGM.GetRefProvider(m_TID), (int) pow(2, x_SrchTableBitLen));', 'CS::DoRun vote table')
    s = sub1(s, '\tint nScoresSum = 0;\n\tfor (size_t i = 0; i < m_CurrentBatch.size(); ++i) {', '#include "cs_search_binding.inc"\n\tint nScoresSum = 0;\n\tfor (size_t i = 0; i < m_CurrentBatch.size(); ++i) {', 'CS::RunBatch')
    s = sub1(s, 'void CS::Cleanup() {', 'void CS::Cleanup() {\n\tConvex::CandidateSearchHip::Shutdown();', 'CS::Cleanup')
    # reads per CS batch = reads per device search / scoring call: the reference's 10 unless CVX_CS_BATCH says otherwise (a measurement knob)
    s = sub1(s, 'int const cBatchSize = 10;', 'int const cBatchSize = cvxCsBatchSize(10);', 'cBatchSize')
    # DoRun's downward adaptation of the vote-table size stops where the device's first attempt does (cs_search_binding.h)
    s = sub1(s, 'if (m_Overflows <= 5 && !up && c_SrchTableBitLen > 8) {', 'if (m_Overflows <= 5 && !up && c_SrchTableBitLen > cvxMinTableBits(m_RefProvider, 8)) {', 'DoRun adaptation floor')
    open(p, 'w').write(s)
if POOL:
    # reads in flight decoupled from the CS threads (ngmlr_amd/csrc/align_pool.h)
    p = T + '/src/CS.cpp'
    s = open(p).read()
    s = sub1(s, '#include "AlignmentBuffer.h"', '#include "AlignmentBuffer.h"\n#include "align_pool.h"', 'CS include')
    s = sub1(s, 'void CS::DoRun() {', 'void CS::DoRun() {\n\tConvex::AlignPool::Attach();', 'CS::DoRun entry')
    s = sub1(s, '\tdelete scoreBuffer;\n\tscoreBuffer = 0;', '\tConvex::AlignPool::Detach();\n\tdelete scoreBuffer;\n\tscoreBuffer = 0;', 'CS::DoRun exit')
    s = sub1(s, 'out->processLongReadLIS(read->group);', 'Convex::AlignPool::Submit(read->group);', 'CS.cpp:296')
    open(p, 'w').write(s)
    p = T + '/src/ScoreBuffer.cpp'
    s = open(p).read()
    s = sub1(s, '#include "AlignmentBuffer.h"', '#include "AlignmentBuffer.h"\n#include "align_pool.h"', 'ScoreBuffer include')
    s = sub1(s, 'out->processLongReadLIS(group);', 'Convex::AlignPool::Submit(group);', 'ScoreBuffer.cpp:155')
    s = sub1(s, 'out->processShortRead(cur_read);', 'Convex::AlignPool::SubmitShort(cur_read);', 'ScoreBuffer.cpp:159')
    s = sub1(s, 'out->processShortRead(read);', 'Convex::AlignPool::SubmitShort(read);', 'ScoreBuffer.cpp:283')
    open(p, 'w').write(s)
    p = T + '/src/NGM.cpp'
    s = open(p).read()
    s = sub1(s, 'Sleep(2000);', 'for (int cvxPoll = 0; cvxPoll < 100 && Running(); ++cvxPoll) Sleep(20);', 'NGM::MainLoop')
    # measurement only: how long the CS threads wait for / hold the lock under which reads are parsed and split (align_pool.h)
    s = sub1(s, 'std::vector<MappedRead*> _NGM::GetNextReadBatch(int desBatchSize) {\n\tNGMLock(&m_Mutex);', 'std::vector<MappedRead*> _NGM::GetNextReadBatch(int desBatchSize) {\n\tlong long const cvxT0 = Convex::AlignPool::ProbeNow();\n\tNGMLock(&m_Mutex);\n\tlong long const cvxT1 = Convex::AlignPool::ProbeNow();', 'GetNextReadBatch lock')
    s = sub1(s, '\tm_CurCount -= desBatchSize;\n\n\tNGMUnlock(&m_Mutex);', '\tm_CurCount -= desBatchSize;\n\n\tConvex::AlignPool::InputLockTimes(cvxT0, cvxT1, Convex::AlignPool::ProbeNow(), count);\n\tNGMUnlock(&m_Mutex);', 'GetNextReadBatch unlock')
    s = sub1(s, '#include "NGM.h"', '#include "NGM.h"\n#include "align_pool.h"\n#include <vector>\n#include <stdlib.h>\n#include <string.h>', 'NGM.cpp include')
    # the read loop in two halves: the record under the input lock, the MappedRead objects outside it (input_batch_binding.inc)
    s = sub1(s, '\tint i = 0;\n\twhile (count < desBatchSize && !eof) {', '\tint i = 0;\n#include "input_batch_binding.inc"\n\twhile (count < desBatchSize && !eof) {', 'GetNextReadBatch loop')
    open(p, 'w').write(s)
    p = T + '/src/IParser.h'
    s = open(p).read()
    s = sub1(s, '\tint parseRead(MappedRead * pRead) {', '\t/* cvx (input_batch_binding.inc): parseRead in two halves -- the raw record (kseq state: under the caller\'s lock), and the MappedRead from it */\n'
             '\tvirtual int cvxReadRecord(kseq_t * rec) { (void) rec; return -3; }\n'
             '\tint cvxFinishRead(MappedRead * pRead, kseq_t * rec, int const l) { return copyToRead(pRead, rec, l); }\n\n\tint parseRead(MappedRead * pRead) {', 'IParser accessors')
    open(p, 'w').write(s)
    p = T + '/src/FastxParser.h'
    s = open(p).read()
    s = sub1(s, '\tvirtual int doParseRead(MappedRead * read) {', '\t/* cvx: the next record, its strings swapped out of the parser (which goes on with the caller\'s previous buffers) */\n'
             '\tvirtual int cvxReadRecord(kseq_t * rec) {\n\t\tint l = kseq_read(tmp);\n\t\t{      /* (also for l < 0: copyToRead reads the name of a record whose quality string has the wrong length) */\n'
             '\t\t\tkstring_t t;\n\t\t\tt = rec->name; rec->name = tmp->name; tmp->name = t;\n\t\t\tt = rec->comment; rec->comment = tmp->comment; tmp->comment = t;\n'
             '\t\t\tt = rec->seq; rec->seq = tmp->seq; tmp->seq = t;\n\t\t\tt = rec->qual; rec->qual = tmp->qual; tmp->qual = t;\n\t\t}\n\t\treturn l;\n\t}\n\n'
             '\tvirtual int doParseRead(MappedRead * read) {', 'FastXParser::cvxReadRecord')
    open(p, 'w').write(s)
    p = T + '/src/ReadProvider.h'
    s = open(p).read()
    s = sub1(s, '\tvirtual MappedRead * NextRead(IParser * parser, int const id);', '\tvirtual MappedRead * NextRead(IParser * parser, int const id, kseq_t * cvxRec = 0, int const cvxL = 0);\npublic:\n'
             '\t/* cvx (input_batch_binding.inc): the raw record under the input lock, NextRead on it outside */\n'
             '\tint cvxReadRecord(kseq_t * rec) { return parser1->cvxReadRecord(rec); }\n'
             '\tMappedRead * cvxGenerateRead(int const readid, kseq_t * rec, int const l) { return NextRead(parser1, readid, rec, l); }\nprivate:', 'ReadProvider accessors')
    open(p, 'w').write(s)
    p = T + '/src/ReadProvider.cpp'
    s = open(p).read()
    s = sub1(s, 'MappedRead * ReadProvider::NextRead(IParser * parser, int const id) {', 'MappedRead * ReadProvider::NextRead(IParser * parser, int const id, kseq_t * cvxRec, int const cvxL) {', 'NextRead signature')
    s = sub1(s, '\t\tl = parser->parseRead(read);', '\t\tl = cvxRec ? parser->cvxFinishRead(read, cvxRec, cvxL) : parser->parseRead(read);', 'NextRead parse')
    open(p, 'w').write(s)
    p = T + '/src/NGM.cpp'
    s = open(p).read()
    open(p, 'w').write(s)
    p = T + '/src/GenericReadWriter.h'
    s = open(p).read()
    s = sub1(s, 'BUFFER_LIMIT =  10000000;', 'BUFFER_LIMIT =  262144;', 'BUFFER_LIMIT')
    open(p, 'w').write(s)
if SCOREWIN:
    # the scoring calls of ScoreBuffer as windows of the resident genome (ngmlr_amd/csrc/score_windows_binding.inc; needs the scorer
    # plugin and the genome announced in _SequenceProvider::Init, i.e. SCORER, INDEX and POOL)
    assert SCORER and INDEX and POOL
    p = T + '/src/ScoreBuffer.cpp'
    s = open(p).read()
    s = sub1(s, '#include "StrippedSW.h"', '#include "StrippedSW.h"\n#include "score_windows_binding.h"', 'ScoreBuffer include (score windows)')
    s = sub1(s, '\t\t//Prepare for score computation\n\t\tfor (int i = 0; i < iScores; ++i) {',
             '\t\t//Prepare for score computation\n\t\tbool cvxWindows = false;\n#define CVX_SCORE_WINDOWS_SITE 1\n#include "score_windows_binding.inc"\n#undef CVX_SCORE_WINDOWS_SITE\n'
             '\t\tfor (int i = 0; i < (cvxWindows ? 0 : iScores); ++i) {', 'ScoreBuffer::DoRun loop')
    s = sub1(s, 'int res = aligner->BatchScore(0, iScores, m_RefBuffer, m_QryBuffer, m_ScoreBuffer, 0);',
             'int res = cvxWindows ? iScores : aligner->BatchScore(0, iScores, m_RefBuffer, m_QryBuffer, m_ScoreBuffer, 0);', 'ScoreBuffer::DoRun BatchScore')
    s = sub1(s, '\tfor (int i = 0; i < read->numScores(); ++i) {\n\t\tint corridor = read->length * 0.3 + 256;\n',
             '\tbool cvxWindows = false;\n#define CVX_SCORE_WINDOWS_SITE 2\n#include "score_windows_binding.inc"\n#undef CVX_SCORE_WINDOWS_SITE\n'
             '\tfor (int i = 0; i < (cvxWindows ? 0 : read->numScores()); ++i) {\n\t\tint corridor = read->length * 0.3 + 256;\n', 'ScoreBuffer::scoreShortRead loop')
    open(p, 'w').write(s)
if FEED:
    # a CS batch searched and scored in one device call (ngmlr_amd/csrc/cs_feed_binding.inc, included by cs_search_binding.inc once
    # cs_feed_binding.h has defined CVX_CS_FEED_BINDING): ScoreBuffer's completion block becomes a method, addScoredRead calls it
    assert SEARCH and SCOREWIN
    p = T + '/src/CS.cpp'
    s = open(p).read()
    s = sub1(s, '#include "cs_search_binding.h"', '#include "cs_search_binding.h"\n#include "cs_feed_binding.h"', 'CS include (feed)')
    open(p, 'w').write(s)
    p = T + '/src/ScoreBuffer.h'
    s = open(p).read()
    s = sub1(s, '\tScoreBuffer(IAlignment * mAligner, AlignmentBuffer * mOut) :',
             '\t/* cvx (cs_feed_binding.inc): a read whose candidates were scored with its search -- the scores, then the completion block of DoRun */\n'
             '\tvoid addScoredRead(MappedRead * read, float const * scores);\n\tvoid cvxCompleteRead(MappedRead * cur_read);\n'
             '\tIAlignment * cvxAligner() const { return aligner; }\n\tuloc cvxRefMaxLen() const { return refMaxLen; }\n\tint cvxCorridor() const { return corridor; }\n\n'
             '\tScoreBuffer(IAlignment * mAligner, AlignmentBuffer * mOut) :', 'ScoreBuffer.h (feed)')
    open(p, 'w').write(s)
    p = T + '/src/ScoreBuffer.cpp'
    s = open(p).read()
    head = '\t\t\tif (++cur_read->Calculated == cur_read->numScores()) {\n'
    tail = '\n\t\t\t}\n\t\t}\n\t\tscoreTime += tmr.ET();'
    assert s.count(head) == 1 and s.count(tail) == 1
    a, b = s.index(head) + len(head), s.index(tail)
    body = s[a:b]      # the reference's own text: topNSE, updateGroupInfo, processLongReadLIS / processShortRead (or what the pool put there)
    assert 'topNSE(cur_read);' in body and 'updateGroupInfo(cur_read)' in body
    s = s[:a] + '\t\t\t\tcvxCompleteRead(cur_read);' + s[b:]
    s = sub1(s, 'void ScoreBuffer::topNSE(MappedRead* read) {', 'void ScoreBuffer::cvxCompleteRead(MappedRead * cur_read) {\n' + body + '\n}\n\n'
             'void ScoreBuffer::addScoredRead(MappedRead * read, float const * scores) {\n\tint const n = read->numScores();\n'
             '\tfor (int k = 0; k < n; ++k) read->Scores[k].Score.f = scores[k];\n\tread->Calculated = n;\n\tcvxCompleteRead(read);\n}\n\n'
             'void ScoreBuffer::topNSE(MappedRead* read) {', 'ScoreBuffer.cpp (feed)')
    open(p, 'w').write(s)
if SAM:
    p = T + '/src/SAMWriter.cpp'
    s = open(p).read()
    m = re.search(r'void SAMWriter::DoWriteReadGeneric\([^)]*\)\s*\{', s)
    assert m and len(re.findall(r'void SAMWriter::DoWriteReadGeneric\(', s)) == 1
    s = s[:m.end()] + '\n#include "sam_writer_binding.inc"\n' + s[m.end():]
    s = s.replace('#include "SAMWriter.h"', '#include "SAMWriter.h"\n#include <vector>\n#include <string.h>\n#include "cvx_align.h"', 1)
    assert 'cvx_align.h' in s
    open(p, 'w').write(s)
if SCORER:
    p = T + '/src/NGM.cpp'
    s = open(p).read()
    assert s.count('instance = new StrippedSW();') == 1
    s = s.replace('instance = new StrippedSW();', 'instance = new %s();' % SCORER, 1)
    s = s.replace('#include "StrippedSW.h"', '#include "StrippedSW.h"\n#include "stripped_sw_hip.h"', 1)
    assert 'stripped_sw_hip.h' in s
    open(p, 'w').write(s)
if CLASS != 'cpu':
    p = T + '/src/AlignmentBuffer.h'
    s = open(p).read()
    s = s.replace('#include "ConvexAlignFast.h"', '#include "ConvexAlignFast.h"\n#include "convex_align_hip.h"\n#include "batching_aligner.h"' + ('\n#include "parking_cpu_aligner.h"' if 'Parking' in CLASS else '') + ('\n#include "nm_regions_note.h"' if REGIONS else '') + ('\n#include "regions_cpu_aligner.h"' if 'RegionsCpu' in CLASS else '')
                  + ('\n#define CVX_INV_CHECKS_BINDING 1\n#include "inv_checks_binding_logic.h"' if INVCHECKS else '') + ('\n#include "inv_checks_cpu_source.h"' if INVCHECKS and 'RegionsCpu' in CLASS else '')
              + ('\n#include "ladder_binding_logic.h"' if LADDER else '') + ('\n#include "ladder_cpu_aligner.h"' if 'LadderCpu' in CLASS else ''), 1)
    pat = re.compile(r'aligner = new Convex::ConvexAlignFast\(', re.S)
    assert len(pat.findall(s)) == 1
    s = pat.sub('aligner = new %s(' % CLASS, s)
    # the --nosse branch (src/AlignmentBuffer.h:345-353): the same class, constructed in scalar-twin mode -- Convex::ConvexAlign's
    # semantics on the device (CVX_CREATE_SCALAR_TWIN), Align::svType / cigarOpCount left as the caller passed them
    if CLASS in ('Convex::ConvexAlignHip', 'Convex::SharedAligner'):
        twin_args = {'Convex::ConvexAlignHip': '0, 0, true', 'Convex::SharedAligner': '-1, true'}[CLASS]
        nosse = re.compile(r'aligner = new Convex::ConvexAlign\((.*?)Config\.getScoreGapDecay\(\)\);', re.S)
        assert len(nosse.findall(s)) == 1
        s = nosse.sub(lambda m: 'aligner = new %s(%sConfig.getScoreGapDecay(), %s);' % (CLASS, m.group(1), twin_args), s)
    open(p, 'w').write(s)
p = T + '/src/CMakeLists.txt'
c = open(p).read()
c = c.replace('add_executable(ngmlr', ('add_definitions(-DCVX_IN_NGMLR_TREE)\ninclude_directories(${CMAKE_CURRENT_SOURCE_DIR} %s/include %s/ngmlr_amd/csrc REPO_TESTS_CPP)\nadd_executable(ngmlr\n%s/ngmlr_amd/csrc/convex_align_hip.cpp\n%s/ngmlr_amd/csrc/batching_aligner.cpp\n%s/ngmlr_amd/csrc/stripped_sw_hip.cpp\n%s/ngmlr_amd/csrc/candidate_search_hip.cpp\n%s/ngmlr_amd/csrc/device_genome.cpp\n%s/ngmlr_amd/csrc/cvx_fiber.cpp%s' % (REPO, REPO, REPO, REPO, REPO, REPO, REPO, REPO, ('\n%s/ngmlr_amd/csrc/align_pool.cpp' % REPO) if POOL else '') + (('\n%s/ngmlr_amd/csrc/batching_scorer.cpp' % REPO) if CHECKS else '')).replace('REPO_TESTS_CPP', REPO + '/tests/cpp'), 1)
c = c.replace('TARGET_LINK_LIBRARIES(ngmlr ${ZLIB_LIBRARIES})', 'TARGET_LINK_LIBRARIES(ngmlr ${ZLIB_LIBRARIES})\nTARGET_LINK_LIBRARIES(ngmlr %s/ngmlr_amd/libcvxalign.so)\nset_target_properties(ngmlr PROPERTIES BUILD_RPATH "\\$ORIGIN/../../ngmlr_amd;/opt/rocm/lib" SKIP_BUILD_RPATH FALSE)' % REPO, 1)
open(p, 'w').write(c)
PY
fi
mkdir -p "$T/build" && cd "$T/build"
cmake .. -DCMAKE_POLICY_VERSION_MINIMUM=3.5 -DCMAKE_BUILD_TYPE=RELWITHDEBINFO > "$WORK/$OUT_NAME.cmake.log" 2>&1
make -j16 > "$WORK/$OUT_NAME.make.log" 2>&1 || { grep -m5 -B2 -A6 "error" "$WORK/$OUT_NAME.make.log"; exit 1; }
local BIN=$(ls "$T"/bin/ngmlr-*/ngmlr)
cp "$BIN" "$REPO/oracle/_ref/$OUT_NAME"
echo "built $REPO/oracle/_ref/$OUT_NAME"
}
# NGMLR_VARIANTS="ngmlr_pool_cpu ngmlr_hip_all" rebuilds only those (default: all of them)
want() { [ -z "${NGMLR_VARIANTS:-}" ] || [[ " $NGMLR_VARIANTS " == *" $1 "* ]]; }
bv() { if want "$1"; then build_variant "$@" & fi; }
bv ngmlr_hip Convex::ConvexAlignHip
bv ngmlr_hip_batched Convex::SharedAligner
bv ngmlr_hip_full Convex::SharedAligner StrippedSWHip sam
bv ngmlr_sam cpu "" sam
bv ngmlr_hip_pool Convex::SharedAligner StrippedSWHip sam pool
bv ngmlr_pool_cpu cpu "" "" pool
bv ngmlr_pool_parked Convex::ParkingCpuAligner "" "" pool      # CPU aligner behind a park / wake per SingleAlign (tests/cpp/parking_cpu_aligner.h)
bv ngmlr_hip_all Convex::SharedAligner StrippedSWHip sam pool search index
bv ngmlr_hip_checks Convex::SharedAligner StrippedSWHip sam pool search index checks
bv ngmlr_hip_scorewin Convex::SharedAligner StrippedSWHip sam pool search index "" scorewin
bv ngmlr_hip_feed Convex::SharedAligner StrippedSWHip sam pool search index "" scorewin feed
bv ngmlr_hip_readseg Convex::SharedAligner StrippedSWHip sam pool search index "" "" "" readseg
bv ngmlr_hip_regions Convex::SharedAligner StrippedSWHip sam pool search index "" "" "" "" regions
bv ngmlr_regions_cpu Convex::RegionsCpuAligner "" "" "" "" "" "" "" "" "" regions      # the reference's CPU aligner behind the request / note exchange (tests/cpp/regions_cpu_aligner.h)
bv ngmlr_hip_invchecks Convex::SharedAligner StrippedSWHip sam pool search index "" "" "" "" regions "" invchecks
bv ngmlr_invchecks_cpu Convex::RegionsCpuAligner "" "" "" "" "" "" "" "" "" regions "" invchecks      # the binding without a GPU: records from the host rule at the finder site (tests/cpp/inv_checks_cpu_source.h)
bv ngmlr_hip_ladder Convex::SharedAligner StrippedSWHip sam pool search index "" "" "" "" regions ladder
bv ngmlr_ladder_cpu Convex::LadderCpuAligner "" "" "" "" "" "" "" "" "" "" ladder      # the reference's CPU aligner behind Convex::LadderAligner (tests/cpp/ladder_cpu_aligner.h)
bv ngmlr_index_cpu cpu "" "" "" "" index
bv ngmlr_ref unmodified      # the reference as it is: wall-clock yardstick of tools/e2e_rates.py
wait
for v in ngmlr_hip ngmlr_hip_batched ngmlr_hip_full ngmlr_sam ngmlr_hip_pool ngmlr_pool_cpu ngmlr_pool_parked ngmlr_hip_all ngmlr_hip_checks ngmlr_hip_scorewin ngmlr_hip_feed ngmlr_hip_readseg ngmlr_hip_regions ngmlr_regions_cpu ngmlr_hip_invchecks ngmlr_invchecks_cpu ngmlr_hip_ladder ngmlr_ladder_cpu ngmlr_index_cpu ngmlr_ref; do
	test -x "$REPO/oracle/_ref/$v" || { echo "missing oracle/_ref/$v"; exit 1; }
done
readelf -d "$REPO/oracle/_ref/ngmlr_hip" | grep -E "RPATH|RUNPATH|NEEDED" | head
rm -rf "$WORK"
