/*
 * ladder_binding_logic.h -- the rules ladder_binding.inc keeps when it hands AlignmentBuffer::computeAlignment's retry loop
 * (reference src/AlignmentBuffer.cpp:291-425) to a Convex::LadderAligner as one request, as plain functions free of HIP and of
 * ngmlr: the binding, the CPU stand-in (tests/cpp/ladder_cpu_aligner.h) and a stand-alone test
 * (tests/cpp/ladder_binding_logic_test.cpp) share them.
 *
 *   LadderFill       cvx_ladder's left / right: what getCorridorEndpointsWithAnchors holds in corridorLeft / corridorRight after
 *                    its loop over the anchors and the three lines behind it (:143-182), before the multiplier (:184) -- the
 *                    builder runs it once per attempt, the binding once per call.  binary32 operations, each rounded on its
 *                    own, in the builder's order.
 *   ladder_outcome   acceptance and the counters a call leaves, as the reference's loop would leave them: valid <=> the
 *                    reported rung returned fullReadLength (:415).
 */
#ifndef LADDER_BINDING_LOGIC_H
#define LADDER_BINDING_LOGIC_H

namespace Convex {

/* One anchor at a time, as the builder's loop takes them; Finish() hands out the two floats. */
class LadderFill {
public:
	LadderFill(int const externalQStart_, int const readPartLength_, int const fullReadLength_, int const qryLen, int const refLen) :
			externalQStart(externalQStart_), readPartLength(readPartLength_), fullReadLength(fullReadLength_), left(0.0f), right(0.0f) {
		float const q = (float) qryLen * 1.0f;
		k = q / (float) refLen;      /* the slope of the read against its window (:143) */
	}
	/* x = the anchor's onRef - the interval's onRefStart (as the int the builder stores it in), onRead and isReverse as they stand */
	void Add(int const x, int const onRead, bool const isReverse) {
		/* where the anchor lies on this read part: a reverse anchor counts from the other end of the full read (:150-157) */
		int const y = isReverse ? fullReadLength - onRead - readPartLength - externalQStart : onRead - externalQStart;
		float const found = (float) x;
		float const lifted = (float) y - 0.0f;
		float const expect = lifted / k;      /* where the line from corner to corner has this read position */
		float const diff = expect - found;
		if (diff > 0) {
			if (right < diff) right = diff;
		} else {
			float const away = diff * -1.0f;
			if (left < away) left = away;
		}
	}
	/* the 128 columns either side and a tenth of the sum on top, the right side from the left's new value (:178-182) */
	void Finish(float & outLeft, float & outRight) const {
		float l = left + 128;
		float r = right + 128;
		float sum = l + r;
		float tenth = sum * 0.1f;
		l = l + tenth;
		sum = l + r;
		tenth = sum * 0.1f;
		r = r + tenth;
		outLeft = l; outRight = r;
	}
private:
	int externalQStart, readPartLength, fullReadLength;
	float k, left, right;
};

/* What a finished ladder means to computeAlignment.  ret / rung / attempts: the LadderAligner's answer; rungs: how many rungs the
 * ladder has (cvx_ladder_rung answers 1 for m = 1 .. rungs). */
struct LadderOutcome {
	bool valid;                /* validAlignment */
	int corridorMultiplier;    /* where the loop's variable would stand */
	int alignmentIds;          /* alignmentId += */
	int invalidAlignments;     /* NGM.Stats->invalidAligmentCount += */
	int widthsCounted;         /* NGM.Stats->corridorLen += the widths of rungs 1 .. widthsCounted */
};

inline LadderOutcome ladder_outcome(int const ret, int const fullReadLength, int const rung, int const attempts, int const rungs) {
	LadderOutcome o;
	o.valid = ret == fullReadLength;
	o.alignmentIds = attempts;
	o.widthsCounted = attempts;
	if (o.valid) {
		/* every attempt before the reported one failed */
		o.corridorMultiplier = rung;
		o.invalidAlignments = attempts - 1;
	} else if (ret < 0) {
		/* the last attempt failed too: the ladder ran out of rungs */
		o.corridorMultiplier = attempts + 1;
		o.invalidAlignments = attempts;
	} else {
		/* an alignment of another length: the device stops at the first rung that aligns, the reference's loop goes on -- and
		 * every later attempt that aligns returns the same value, so it tries every rung there is and fails */
		o.corridorMultiplier = rungs + 1;
		o.invalidAlignments = rungs;
	}
	return o;
}

/* the sum NGM.Stats->corridorLen takes: widthOf(m) is rung m's corridor width (cvx_ladder_rung's corridor_width) */
template <typename WidthOf>
inline long ladder_corridor_len(int const rungsCounted, WidthOf widthOf) {
	long sum = 0;
	for (int m = 1; m <= rungsCounted; ++m) sum += (long) widthOf(m);
	return sum;
}

}  // namespace Convex

#endif
