/*
 * read_segments_binding.inc -- inserted by tools/build_ngmlr_hip.sh at the top of the Interval overload of
 * AlignmentBuffer::extractReadSeq (reference src/AlignmentBuffer.cpp:1545-1549; in scope: readSeqLen, interval, read, revComp).
 * Every caller of that overload hands the string to alignInterval / computeAlignment, which only measure it before SingleAlign;
 * so instead of the characters (a strncpy, or computeReverseSeq's byte-at-a-time reverse complement, a second one with revComp)
 * the caller gets a placeholder of the same length that names the segment (Convex::DeviceReads, convex_align_hip.h), and the
 * device writes the query.  Kept from the reference: the length check, and read->computeReverseSeq() for a reverse interval
 * (RevSeq is cached per read and relied on elsewhere).  CVX_DEVICE_READS=0, or a segment that does not lie inside the read,
 * falls through to the reference's own code.
 */
if (Convex::DeviceReads::Enabled() && interval->onReadStart >= 0 && readSeqLen > 0 && readSeqLen <= 200000000 &&
		(long long) interval->onReadStart + readSeqLen <= (long long) read->length) {
	if (interval->isReverse) read->computeReverseSeq();
	unique_ptr<char[]> cvxQuery(new char[Convex::DeviceReads::BufferBytes(readSeqLen)]);
	Convex::DeviceReads::Placeholder(cvxQuery.get(), read->Seq, read->length, interval->onReadStart, readSeqLen, (interval->isReverse != revComp) ? CVX_SEG_REVCOMP : 0);
	return cvxQuery;
}
