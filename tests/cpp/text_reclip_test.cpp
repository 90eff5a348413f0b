/*
 * text_reclip_test.cpp -- cvx::text_reclip (ngmlr_amd/csrc/cvx_job_text_logic.h, behind cvx_text_reclip) as a program of its own: hand-written
 * records against strings put together the long way, every output buffer allocated at exactly the capacity passed, so that a
 * byte written past it is the sanitizer's to find (tests/test_text_reclip_san_cpu.py builds this with -fsanitize=address,undefined).
 * No device, no library.
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "cvx_job_text_logic.h"

static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); ++g_fail; } } while (0)

/* a record as the text stage leaves it with both external clips zero; core: the CIGAR between the clips */
static cvx_alignment_text make_rec(int qstart, int qend, const std::string &core, int core_read_bases, int core_pieces, std::string *cigar) {
	cvx_alignment_text r;
	memset(&r, 0, sizeof(r));
	*cigar = (qstart > 0 ? std::to_string(qstart) + "S" : std::string()) + core + (qend > 0 ? std::to_string(qend) + "S" : std::string());
	r.ret = (qstart > 0 ? qstart : 0) + core_read_bases + qend;
	r.score = 123.5f;
	r.position_offset = 7;
	r.qstart = qstart;
	r.qend = qend;
	r.nm = 3;
	r.identity = 0.75f;
	r.alignment_length = core_read_bases + 2;
	r.cigar_op_count = core_pieces + (qstart > 0) + (qend > 0);
	r.sv_type = 1;
	r.first_read = qstart;
	r.last_ref = 40;
	r.last_read = qstart + core_read_bases;
	r.nm_count = 11;
	r.cigar_len = (int32_t) cigar->size();
	r.md_len = 9;
	return r;
}

/* the fields the clips do not enter */
static bool rest_equal(const cvx_alignment_text &a, const cvx_alignment_text &b) {
	return a.score == b.score && a.position_offset == b.position_offset && a.nm == b.nm && a.identity == b.identity &&
			a.alignment_length == b.alignment_length && a.sv_type == b.sv_type && a.first_ref == b.first_ref && a.first_read == b.first_read &&
			a.last_ref == b.last_ref && a.last_read == b.last_read && a.nm_count == b.nm_count && a.md_len == b.md_len;
}

static void one_case(int qstart, int qend, int eqs, int eqe, bool twin) {
	const std::string core = "12M3I40M2D7M";
	const int read_bases = 12 + 3 + 40 + 7, pieces = 5;
	std::string cigar;
	cvx_alignment_text rec = make_rec(qstart, qend, core, read_bases, pieces, &cigar);
	if (twin) rec.cigar_op_count = rec.sv_type = CVX_NOT_WRITTEN;
	const int nq = qstart + eqs, ne = qend + eqe;
	const std::string want = (nq > 0 ? std::to_string(nq) + "S" : std::string()) + core + (ne > 0 ? std::to_string(ne) + "S" : std::string());
	const int len = (int) want.size();
	const int caps[] = {0, 1, 2, len - 1, len, len + 1, len + 2, len + 40};
	for (int cap : caps) {
		if (cap < 0) continue;
		/* the input CIGAR without its NUL and the output at exactly `cap` bytes: the heap's red zones stand right behind both */
		std::vector<char> in(cigar.begin(), cigar.end());
		char *out = cap > 0 ? (char *) malloc((size_t) cap) : nullptr;
		if (out) memset(out, 'Z', (size_t) cap);
		cvx_alignment_text got;
		memset(&got, 0x5a, sizeof(got));
		CHECK(cvx::text_reclip(&rec, in.data(), eqs, eqe, out, cap, &got) == CVX_OK);
		CHECK(got.cigar_len == len);
		CHECK(got.qstart == nq && got.qend == ne);
		CHECK(got.ret == (nq > 0 ? nq : 0) + read_bases + ne);
		CHECK(got.cigar_op_count == (twin ? (int) CVX_NOT_WRITTEN : pieces + (nq > 0) + (ne > 0)));
		CHECK(rest_equal(got, rec));
		if (cap > 0) {
			const int kept = len < cap - 1 ? len : cap - 1;
			CHECK(out[kept] == '\0');
			CHECK(memcmp(out, want.data(), (size_t) kept) == 0);
			for (int i = kept + 1; i < cap; ++i) CHECK(out[i] == 'Z');      /* nothing behind the NUL is touched */
		}
		free(out);
	}
}

int main() {
	const int own[] = {0, 1, 9, 10, 4999, 100000};
	const int ext[][2] = {{0, 0}, {0, 7}, {7, 0}, {4999, 1}, {1, 4999}, {2000000000, 0}};
	int cases = 0;
	for (int qs : own) for (int qe : own) for (const auto &e : ext) for (int twin = 0; twin < 2; ++twin) {
		if ((long long) qs + e[0] > 2100000000LL) continue;
		one_case(qs, qe, e[0], e[1], twin != 0);
		++cases;
	}
	/* a record without an alignment passes through, the string is empty; also in place and with no buffer at all */
	{
		cvx_alignment_text rec;
		memset(&rec, 0, sizeof(rec));
		rec.ret = -1; rec.score = -1.0f;
		cvx_alignment_text twin = rec;
		twin.cigar_op_count = twin.sv_type = CVX_NOT_WRITTEN;
		char *out = (char *) malloc(1);
		out[0] = 'Z';
		cvx_alignment_text got;
		CHECK(cvx::text_reclip(&rec, nullptr, 4999, 1, out, 1, &got) == CVX_OK && memcmp(&got, &rec, sizeof(rec)) == 0 && out[0] == '\0');
		CHECK(cvx::text_reclip(&twin, "", 1, 4999, nullptr, 0, &got) == CVX_OK && memcmp(&got, &twin, sizeof(twin)) == 0);
		CHECK(cvx::text_reclip(&twin, "", 1, 4999, nullptr, 0, &twin) == CVX_OK && twin.cigar_op_count == CVX_NOT_WRITTEN && twin.ret == -1);
		free(out);
	}
	/* in place: out == rec */
	{
		std::string cigar;
		cvx_alignment_text rec = make_rec(5, 0, "30M", 30, 1, &cigar);
		char *out = (char *) malloc(16);
		CHECK(cvx::text_reclip(&rec, cigar.data(), 95, 12, out, 16, &rec) == CVX_OK);
		CHECK(strcmp(out, "100S30M12S") == 0 && rec.qstart == 100 && rec.qend == 12 && rec.ret == 142 && rec.cigar_op_count == 3 && rec.cigar_len == 10);
		free(out);
	}
	/* misuse */
	{
		std::string cigar;
		cvx_alignment_text rec = make_rec(5, 7, "30M", 30, 1, &cigar), got;
		char buf[8];
		CHECK(cvx::text_reclip(nullptr, cigar.data(), 0, 0, buf, 8, &got) == CVX_ERR_ARG);
		CHECK(cvx::text_reclip(&rec, cigar.data(), 0, 0, buf, 8, nullptr) == CVX_ERR_ARG);
		CHECK(cvx::text_reclip(&rec, cigar.data(), 0, 0, buf, -1, &got) == CVX_ERR_ARG);
		CHECK(cvx::text_reclip(&rec, cigar.data(), 0, 0, nullptr, 8, &got) == CVX_ERR_ARG);
		CHECK(cvx::text_reclip(&rec, nullptr, 0, 0, buf, 8, &got) == CVX_ERR_ARG);
		rec.cigar_len = 3;      /* shorter than "5S" + "7S" */
		CHECK(cvx::text_reclip(&rec, cigar.data(), 0, 0, buf, 8, &got) == CVX_ERR_ARG);
	}
	if (g_fail) { printf("text_reclip_test: %d failures\n", g_fail); return 1; }
	printf("text_reclip_test: ok, %d cases\n", cases);
	return 0;
}
