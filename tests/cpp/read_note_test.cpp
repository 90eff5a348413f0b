/*
 * read_note_test.cpp -- Convex::DeviceReads' self-describing placeholder, no device: several noted buffers live side by side in
 * one context and each is found with its own note whatever was noted since; a buffer is found from any thread; a plain string,
 * a byte copy of a placeholder and a materialised buffer are not placeholders; Materialise and CopyOut give the characters
 * extractReadSeq would have built.  tests/test_segments_logic_cpu.py builds and runs it.
 */
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "convex_align_hip.h"

typedef Convex::DeviceReads DR;

static char cpl(char c) { return c == 'A' ? 'T' : c == 'T' ? 'A' : c == 'C' ? 'G' : c == 'G' ? 'C' : c; }
static std::string want_of(std::string const & read, int start, int len, int flags) {
	std::string w = read.substr((size_t) start, (size_t) len);
	if (flags) { std::string r; for (size_t k = w.size(); k-- > 0;) r.push_back(cpl(w[k])); w = r; }
	return w;
}

int main() {
	int bad = 0;
	std::string read = "ACGTNacgtGGATCCAATTxyzACGT";
	for (int k = 0; k < 300; ++k) read.push_back("ACGTN"[(k * 7 + k / 5) % 5]);
	struct Noted { std::vector<char> buf; int start, len, flags; };
	/* two, and many, live noted buffers in ONE context: the full read first (alignInterval's string), then the shorter ones a
	 * realign would extract while the first is still in use */
	std::vector<Noted> live;
	int const shapes[][3] = { {0, 326, 0}, {5, 100, 1}, {40, 1, 0}, {100, 226, 1}, {7, 17, 0}, {0, 326, 1} };
	for (auto const & s : shapes) {
		live.push_back(Noted{ std::vector<char>((size_t) DR::BufferBytes(s[1]), 0), s[0], s[1], s[2] });
		DR::Placeholder(live.back().buf.data(), read.c_str(), (int) read.size(), s[0], s[1], s[2]);
	}
	auto check_all = [&](char const * when) {
		for (Noted const & n : live) {
			char const * seq = 0;
			int rl = 0, s = 0, l = 0, f = 0;
			if ((int) strlen(n.buf.data()) != n.len) { printf("%s: strlen\n", when); ++bad; }      /* what the corridor builders measure */
			if (!DR::Lookup(n.buf.data(), seq, rl, s, l, f) || seq != read.c_str() || rl != (int) read.size() || s != n.start || l != n.len || f != n.flags) { printf("%s: a live note was lost\n", when); ++bad; }
		}
	};
	check_all("same context");
	std::thread([&] { check_all("another thread"); }).join();
	/* not placeholders: NULL, a plain string, the inside of a placeholder, a byte copy of one */
	char const * seq = 0;
	int rl = 0, s = 0, l = 0, f = 0;
	std::vector<char> copy = live[1].buf;
	if (DR::Lookup(0, seq, rl, s, l, f) || DR::Lookup("ACGTACGT", seq, rl, s, l, f) || DR::Lookup("", seq, rl, s, l, f) ||
			DR::Lookup(live[1].buf.data() + 1, seq, rl, s, l, f) || DR::Lookup(copy.data(), seq, rl, s, l, f)) { printf("a non-placeholder was recognised\n"); ++bad; }
	/* a plain string at the address a freed placeholder had */
	{
		char * p = new char[DR::BufferBytes(50)];
		DR::Placeholder(p, read.c_str(), (int) read.size(), 3, 50, 1);
		strcpy(p, "GATTACA");
		if (DR::Lookup(p, seq, rl, s, l, f)) { printf("a plain string was taken for the placeholder its address once held\n"); ++bad; }
		delete[] p;
	}
	/* CopyOut: any window of a noted string, and strncpy for a plain one */
	for (Noted const & n : live) {
		std::string const w = want_of(read, n.start, n.len, n.flags);
		for (int off : {0, 1, n.len / 2, n.len - 1}) for (int cnt : {1, 3, 100}) {
			if (off < 0 || off + cnt > n.len) continue;
			std::vector<char> out((size_t) cnt + 1, 0);
			DR::CopyOut(out.data(), n.buf.data(), off, cnt);
			if (w.substr((size_t) off, (size_t) cnt) != out.data()) { printf("CopyOut(%d, %d) of (%d, %d, %d)\n", off, cnt, n.start, n.len, n.flags); ++bad; }
		}
	}
	{
		char out[8] = {0};
		DR::CopyOut(out, "ACGTACGT", 2, 4);
		if (strcmp(out, "GTAC") != 0) { printf("CopyOut of a plain string\n"); ++bad; }
	}
	check_all("after CopyOut");
	/* Materialise: the characters, once; the others stay noted */
	for (size_t i = 0; i < live.size(); i += 2) {
		Noted & n = live[i];
		if (!DR::Materialise(n.buf.data()) || want_of(read, n.start, n.len, n.flags) != n.buf.data()) { printf("Materialise: wrong string\n"); ++bad; }
		if (DR::Materialise(n.buf.data()) || DR::Lookup(n.buf.data(), seq, rl, s, l, f)) { printf("a materialised buffer is still a placeholder\n"); ++bad; }
	}
	for (size_t i = 1; i < live.size(); i += 2) if (!DR::Lookup(live[i].buf.data(), seq, rl, s, l, f) || s != live[i].start) { printf("a neighbour's note was lost\n"); ++bad; }
	if (bad) { printf("read_note_test: %d errors\n", bad); return 1; }
	printf("read_note_test: ok\n");
	return 0;
}
