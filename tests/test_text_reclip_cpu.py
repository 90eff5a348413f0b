"""CPU: cvx_text_reclip -- external clips put onto a record and a CIGAR the text stage formatted without them (what a
CVX_CREATE_JOB_TEXT job delivers) -- against the host form itself: reclip(host_form(ext = 0)) == host_form(ext) in every
cvx_alignment_text field, the identity bits and the CIGAR bytes, over the tile zoo and the edge tiles with ops from the port
oracle, for the default and the scalar twin's text stage, invalid records and every truncation boundary."""
import ctypes as C

import numpy as np
import pytest

from tests import util

CLIPS = ((0, 0), (0, 7), (7, 0), (4999, 1), (1, 4999))


def _host_form(lib, capi, r, ops, t, eqs, eqe, twin=False, cigar_cap=None):
    """cvx_format_alignment_ex -> (record, CIGAR bytes as the buffer holds them)"""
    cap = 4 * t.H + 64 if cigar_cap is None else cigar_cap
    txt = capi.CvxAlignmentText()
    cig = C.create_string_buffer(max(cap, 1))
    md = C.create_string_buffer(4 * t.H + 4 * t.W + 64)
    assert lib.cvx_format_alignment_ex(C.byref(r), ops.ctypes.data, t.ref, t.W, t.H, eqs, eqe, cig if cap > 0 else None, cap, md, len(md),
                                       None, 0, capi.FORMAT_SCALAR_TWIN if twin else 0, C.byref(txt)) == 0
    if cigar_cap is None:
        assert txt.cigar_len < cap
    return txt, (cig.value if cap > 0 else b"")


def _fields(capi, txt):
    d = {f: getattr(txt, f) for f, _ in capi.CvxAlignmentText._fields_ if f not in ("score", "identity")}
    d["score_bits"] = int(np.float32(txt.score).view(np.uint32))
    d["identity_bits"] = int(np.float32(txt.identity).view(np.uint32))
    return d


@pytest.fixture(scope="module")
def formatted(port_oracle):
    """every tile once through the oracle: (tile, result record, ops)"""
    from ngmlr_amd import capi
    out = []
    for t in util.tile_zoo() + util.edge_tiles():
        w = port_oracle.align(t)
        r = capi.CvxResult()
        if w["ret"] < 0:
            r.status, r.score = 2, 55.0
            out.append((t, r, np.zeros(1, np.uint32)))
            continue
        f, ops = port_oracle.last_fwd(), port_oracle.last_ops()
        r.score, r.status = w["score"], 0
        r.ref_position, r.qstart, r.qend = f["ref_position"], f["qstart"], f["qend"]
        r.n_ops, r.ops_begin = len(ops), 0
        out.append((t, r, (ops if len(ops) else np.zeros(1, np.uint32)).astype(np.uint32)))
    return out


def test_reclip_equals_the_host_form_with_clips(formatted):
    from ngmlr_amd import capi
    from ngmlr_amd.aligner import reclip
    lib = capi.load()
    seen = {"qstart0": 0, "qstart+": 0, "qend0": 0, "qend+": 0, "invalid": 0, "twin": 0, "twin_invalid": 0}
    for t, r, ops in formatted:
        for twin in (False, True):
            rec0, cig0 = _host_form(lib, capi, r, ops, t, 0, 0, twin)
            if rec0.ret < 0:
                seen["twin_invalid" if twin else "invalid"] += 1
            else:
                seen["twin"] += twin
                seen["qstart0" if rec0.qstart == 0 else "qstart+"] += 1
                seen["qend0" if rec0.qend == 0 else "qend+"] += 1
            if twin:
                assert rec0.cigar_op_count == capi.NOT_WRITTEN and rec0.sv_type == capi.NOT_WRITTEN
            for eqs, eqe in CLIPS:
                want, wcig = _host_form(lib, capi, r, ops, t, eqs, eqe, twin)
                got, gcig = reclip(rec0, cig0, eqs, eqe, lib=lib)
                assert _fields(capi, got) == _fields(capi, want), (t.tag, twin, eqs, eqe)
                assert gcig == wcig, (t.tag, twin, eqs, eqe)
                if rec0.ret < 0:      # passes through unchanged
                    assert bytes(got) == bytes(rec0) and gcig == b""
    assert all(v > 0 for v in seen.values()), seen
    assert seen["qstart+"] >= 5 and seen["qend+"] >= 5 and seen["qstart0"] >= 5 and seen["qend0"] >= 5, seen


def test_truncation_follows_the_host_form(formatted):
    """cigar_cap = 0, 1, len and len + 1 of the clipped CIGAR: the same bytes in the buffer, the full length in the record"""
    from ngmlr_amd import capi
    from ngmlr_amd.aligner import reclip
    lib = capi.load()
    n = 0
    for t, r, ops in formatted[::3]:
        rec0, cig0 = _host_form(lib, capi, r, ops, t, 0, 0)
        if rec0.ret < 0:
            continue
        for eqs, eqe in ((0, 0), (4999, 1), (1, 4999)):
            full, fcig = _host_form(lib, capi, r, ops, t, eqs, eqe)
            for cap in (0, 1, full.cigar_len, full.cigar_len + 1):
                want, wcig = _host_form(lib, capi, r, ops, t, eqs, eqe, cigar_cap=cap)
                got, gcig = reclip(rec0, cig0, eqs, eqe, cigar_cap=cap, lib=lib)
                assert gcig == wcig and _fields(capi, got) == _fields(capi, want), (t.tag, eqs, eqe, cap)
                assert got.cigar_len == full.cigar_len == len(fcig)
                assert len(gcig) == max(0, min(cap - 1, full.cigar_len))
            n += 1
    assert n >= 30


def test_bad_arguments_are_refused(built):
    from ngmlr_amd import capi
    lib = capi.load()
    rec, out = capi.CvxAlignmentText(), capi.CvxAlignmentText()
    buf = C.create_string_buffer(8)
    rec.ret, rec.qstart, rec.cigar_len = 10, 12, 2           # "12S" alone needs three characters
    assert lib.cvx_text_reclip(C.byref(rec), b"5M", 0, 0, buf, 8, C.byref(out)) == -3 and b"cvx_text_reclip" in lib.cvx_last_error()
    rec.qstart = 0
    assert lib.cvx_text_reclip(C.byref(rec), b"5M", 0, 0, buf, -1, C.byref(out)) == -3
    assert lib.cvx_text_reclip(C.byref(rec), b"5M", 0, 0, None, 8, C.byref(out)) == -3
    assert lib.cvx_text_reclip(None, b"5M", 0, 0, buf, 8, C.byref(out)) == -3
    assert lib.cvx_text_reclip(C.byref(rec), None, 0, 0, buf, 8, C.byref(out)) == -3
    assert lib.cvx_text_reclip(C.byref(rec), b"5M", 3, 0, buf, 8, C.byref(rec)) == 0      # in place
    assert buf.value == b"3S5M" and rec.qstart == 3 and rec.ret == 13 and rec.cigar_len == 4
