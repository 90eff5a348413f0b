/*
 * ladder_binding.inc -- included by tools/build_ngmlr_hip.sh in AlignmentBuffer::computeAlignment in front of the retry loop
 * (reference src/AlignmentBuffer.cpp:292, behind `int corridorMultiplier = 1;`), which stays as it stands: it is the fallback.
 * The script also keeps `corridor` as it was passed, before the clamp at :266, in cvxLadderCorridor.
 *
 * Where the aligner is a Convex::LadderAligner (convex_align_hip.h; found with dynamic_cast, IAlignment is untouched) the whole
 * loop is ONE request: a cvx_ladder of 16 bytes instead of a CorridorLine[] built, fitted and verified per attempt, and no wait
 * for another launch per rung.  The rules are ladder_binding_logic.h's: left / right as getCorridorEndpointsWithAnchors holds
 * them before its multiplier, valid <=> the reported rung returned fullReadLength (:415), alignmentId and the two NGM.Stats
 * counters as the loop would have left them.  The loop runs untouched when SingleLadder answers false (CVX_DEVICE_LADDER=0,
 * CVX_DEVICE_TEXT=1), when the aligner is no LadderAligner, and under pacbioDebug or --stdout 6, whose per-attempt output
 * only the loop produces.  A throw lands in the reference's own catch (...) below.
 */
			if (!pacbioDebug && !stdoutPrintAlignCorridor) {
				Convex::LadderAligner * const cvxLadderAligner = dynamic_cast<Convex::LadderAligner *>(aligner);
				if (cvxLadderAligner != 0) {
					int const cvxRefLen = (int) strlen(refSeq), cvxQryLen = (int) strlen(readSeq);      /* what the builders measure (:111-112, :134-135); placeholders have their string's length */
					cvx_ladder cvxLadder;
					cvxLadder.corridor = cvxLadderCorridor;
					cvxLadder.flags = (interval->anchorLength > 0 ? CVX_LADDER_ANCHORS : 0) | (realign ? CVX_LADDER_REALIGN : 0)
							| (shortRead ? CVX_LADDER_SHORT : 0) | (fullAlignment ? CVX_LADDER_FULL : 0);
					cvxLadder.left = cvxLadder.right = 0.0f;
					if (interval->anchorLength > 0 && !realign && !shortRead && !fullAlignment) {      /* the one case in which the loop calls the anchors builder (:309-320) */
						Convex::LadderFill cvxFill(externalQStart, readPartLength, fullReadLength, cvxQryLen, cvxRefLen);
						for (int i = 0; i < interval->anchorLength; ++i) {
							cvxFill.Add((int) (interval->anchors[i].onRef - interval->onRefStart), interval->anchors[i].onRead, interval->anchors[i].isReverse);
						}
						cvxFill.Finish(cvxLadder.left, cvxLadder.right);
					}
#ifdef CVX_LADDER_CALL_CONTEXT
					CVX_LADDER_CALL_CONTEXT(fullReadLength);      /* (a test aligner that records its calls: tests/cpp/ladder_cpu_aligner.h) */
#endif
					align->svType = read->ReadId;      /* as the loop does (:362) */
					int cvxRet = -1, cvxRung = 0, cvxAttempts = 0, cvxWidth = 0;
					if (cvxLadderAligner->SingleLadder(refSeq, readSeq, *align, externalQStart, externalQEnd, cvxLadder, cvxRet, cvxRung, cvxAttempts, cvxWidth)) {
						cvx_tile cvxTile, cvxForm;
						memset(&cvxTile, 0, sizeof(cvxTile));
						memset(&cvxForm, 0, sizeof(cvxForm));
						cvxTile.ref_len = cvxRefLen; cvxTile.qry_len = cvxQryLen;
						int cvxRungs = 0;
						while (cvx_ladder_rung(&cvxTile, &cvxLadder, cvxRungs + 1, &cvxForm) == 1) ++cvxRungs;
						Convex::LadderOutcome const cvxOutcome = Convex::ladder_outcome(cvxRet, fullReadLength, cvxRung, cvxAttempts, cvxRungs);
						validAlignment = cvxOutcome.valid;
						corridorMultiplier = cvxOutcome.corridorMultiplier;
						alignmentId += cvxOutcome.alignmentIds;
						NGM.Stats->invalidAligmentCount += cvxOutcome.invalidAlignments;
						NGM.Stats->corridorLen += Convex::ladder_corridor_len(cvxOutcome.widthsCounted, [&](int const m) {
							return cvx_ladder_rung(&cvxTile, &cvxLadder, m, &cvxForm) == 1 ? (int) cvxForm.corridor_width : 0;
						});
						alignedBp = readLength - (align->QStart - externalQStart) - (align->QEnd - externalQEnd);      /* (:413) */
						retryCount = 0;      /* the ladder was the loop: nothing is left for it */
					}
				}
			}
