"""CPU: the scalar twin (Convex::ConvexAlign, ngmlr --nosse) -- its fixtures, the oracle that covers it on x-free tiles, the host
text stage in twin mode and the kernel-class selection of a twin handle."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from oracle.pyoracle import Oracle, same_alignment
from tests import twin_cases
from tests.twin_cases import TWIN_KEYS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", ["twin_xfree.npz", "twin_x.npz"])
def test_fixtures_are_what_the_recorder_library_gives(built, name):
    """Re-running the reference's own Convex::ConvexAlign on every fixture input reproduces the recorded outputs."""
    if not os.path.exists(twin_cases.TWIN_SO):
        pytest.skip("the recorder's twin library is built only where the reference sources are")
    rec = {}
    for family, params, t, w, _ in twin_cases.load(name):
        if params not in rec:
            rec[params] = twin_cases.TwinRecorder(params)
        got = rec[params].align(t)
        assert got["rc"] == 0
        if w["ret"] < 0:
            assert got["ret"] < 0, t.tag
            continue
        assert same_alignment(w, got) is None, (t.tag, same_alignment(w, got))
        assert (got["cigar_op_count"], got["sv_type"]) == (-1, -1)      # as they went in: the twin writes neither
    for r in rec.values():
        r.close()


def test_fixture_families_cannot_pass_vacuously():
    """same_alignment treats two invalid results as equal, and a fixture on which the twin equals ConvexAlignFast shows nothing:
    at least 75 % of every family is a valid alignment under the twin, and at least a fifth of the x-bearing tiles have a twin
    result that is not ConvexAlignFast's."""
    fam = {}
    for name in ("twin_xfree.npz", "twin_x.npz"):
        for family, _, t, w, f in twin_cases.load(name):
            s = fam.setdefault(family, [0, 0, 0])
            s[0] += 1
            s[1] += w["ret"] >= 0
            s[2] += twin_cases.differs(w, f)
            assert 40 <= t.H <= 600 and (name != "twin_xfree.npz" or b"x" not in t.ref)
    for family, (n, valid, _) in fam.items():
        assert valid >= 0.75 * n, (family, n, valid)
    assert set(twin_cases.X_FAMILIES) <= set(fam)
    n_x = sum(fam[f][0] for f in twin_cases.X_FAMILIES)
    n_diff = sum(fam[f][2] for f in twin_cases.X_FAMILIES)
    assert 5 * n_diff >= n_x, (n_x, n_diff)
    # and the x-free tiles of the default scoring are the ones where twin == fast (the fast regime)
    assert fam["xfree_default"][2] == 0 and all(fam["xfree_scoring%d" % k][2] > 0 for k in (1, 2, 3))
    for name in ("twin_xfree.npz", "twin_x.npz"):
        assert os.path.getsize(os.path.join(twin_cases.GOLDEN, name)) < 1 << 20


def test_port_in_spec_fill_mode_is_the_twin_on_x_free_tiles(built):
    """The scalar recurrence of the port (set_spec_fill) equals the recorded twin on every x-free tile, for every recorded scoring:
    the oracle the GPU tests use where the reference tree is not."""
    orc = {}
    n_valid = 0
    for family, params, t, w, _ in twin_cases.load("twin_xfree.npz"):
        if params not in orc:
            orc[params] = Oracle("port", params)
            orc[params].set_spec_fill(True)
        d = same_alignment(w, orc[params].align(t), keys=TWIN_KEYS)
        assert d is None, (t.tag, d)
        n_valid += w["ret"] >= 0
    assert len(orc) == 4 and n_valid >= 60


def _text(lib, capi, res, ops, t, flags):
    txt = capi.CvxAlignmentText()
    cap = 4 * t.H + 64
    cig, md = C.create_string_buffer(cap), C.create_string_buffer(cap)
    nm = np.zeros((2 * (t.H + 1) + t.W + 16, 3), dtype=np.int32)
    assert lib.cvx_format_alignment_ex(C.byref(res), ops.ctypes.data, t.ref, t.W, t.H, t.ext_qstart, t.ext_qend, cig, cap, md, cap,
                                       nm.ctypes.data, len(nm), flags, C.byref(txt)) == 0
    return txt, cig.value.decode(), md.value.decode()


def test_host_text_stage_in_twin_mode(built, port_oracle):
    """The ops of x-free tiles through the twin form of the host text stage: the port's text fields, cigar_op_count and sv_type
    reported as not written."""
    from ngmlr_amd import capi
    from ngmlr_amd.aligner import format_alignment
    lib = capi.load()
    n = 0
    for family, params, t, w, _ in twin_cases.load("twin_xfree.npz"):
        if family != "xfree_default":
            continue
        want = port_oracle.align(t)
        if want["ret"] < 0:
            continue
        ops = port_oracle.last_ops()
        f = port_oracle.last_fwd()
        res = capi.CvxResult(np.float32(want["score"]), 0, f["best_x"], f["best_y"], f["ref_position"], f["qstart"], f["qend"], len(ops), 0, 0)
        got = format_alignment(lib, res, ops, t, scalar_twin=True)
        assert same_alignment(want, got, keys=TWIN_KEYS) is None, (t.tag, same_alignment(want, got, keys=TWIN_KEYS))
        assert same_alignment(w, got, keys=TWIN_KEYS) is None, t.tag
        assert (got["cigar_op_count"], got["sv_type"]) == (capi.NOT_WRITTEN, capi.NOT_WRITTEN)
        fast = format_alignment(lib, res, ops, t)
        assert (fast["cigar_op_count"], fast["sv_type"]) == (want["cigar_op_count"], want["sv_type"])
        n += 1
    assert n >= 24
    bad = capi.CvxAlignmentText()
    assert lib.cvx_format_alignment_ex(None, None, b"", 0, 0, 0, 0, None, 0, None, 0, None, 0, 8, C.byref(bad)) != 0      # unknown flag


def test_n_clip_block_is_the_fast_form_only(built):
    """A window whose clip borders a run of 'X' (more than 80 of the 100 probed characters, src/ConvexAlignFast.cpp:493-528): the
    fast form sets flag bit 0x1, the twin form never does."""
    from ngmlr_amd import capi, synth
    lib = capi.load()
    rng = np.random.default_rng(3)
    core = synth.random_ref(rng, 200).tobytes()
    ref = b"X" * 120 + core + b"X" * 120
    t = synth.Tile(ref, core, *synth.corridor_linear(200, 300), tag="X-flanks")
    ops = np.array([(200 << 4) | 7], dtype=np.uint32)      # 200 columns of CVX_OP_EQ
    res = capi.CvxResult(np.float32(400.0), 0, 319, 199, 120, 0, 0, 1, 0, 0)
    txt, cig, _ = _text(lib, capi, res, ops, t, 0)
    assert cig == "200M"
    assert txt.sv_type & 1 and txt.cigar_op_count == 1
    twin, cig2, _ = _text(lib, capi, res, ops, t, capi.FORMAT_SCALAR_TWIN)
    assert cig2 == "200M" and (twin.sv_type, twin.cigar_op_count) == (capi.NOT_WRITTEN, capi.NOT_WRITTEN)
    assert (twin.nm, twin.alignment_length, twin.position_offset) == (txt.nm, txt.alignment_length, txt.position_offset)


def test_batch_form_of_the_host_text_stage_in_twin_mode(built, port_oracle):
    """cvx_format_batch_ex with the twin flag (ngmlr_amd.aligner.format_tileset(scalar_twin=True)): the single form's fields for
    every tile, and the plain batch form still reports op count and flags."""
    from ngmlr_amd import capi, synth
    from ngmlr_amd.aligner import RESULT_DTYPE, format_alignment, format_tileset
    lib = capi.load()
    tiles, res, arena = [], [], []
    for family, params, t, w, _ in twin_cases.load("twin_xfree.npz"):
        if family != "xfree_default" or len(tiles) >= 20:
            continue
        want = port_oracle.align(t)
        ops, f = port_oracle.last_ops(), port_oracle.last_fwd()
        ok = want["ret"] >= 0
        res.append((want["score"] if ok else -1.0, 0 if ok else 1, f["best_x"], f["best_y"], f["ref_position"], f["qstart"], f["qend"],
                    len(ops) if ok else 0, sum(len(a) for a in arena), 0))
        arena.append(ops if ok else ops[:0])
        tiles.append(t)
    results = np.array(res, dtype=RESULT_DTYPE)
    ops = np.concatenate(arena + [np.zeros(1, np.uint32)])
    ts = synth.tileset_from_tiles(tiles)
    idx = np.arange(len(tiles))
    twin = format_tileset(lib, ts, idx, results, ops, n_threads=3, scalar_twin=True)
    fast = format_tileset(lib, ts, idx, results, ops, n_threads=3)
    for i, t in enumerate(tiles):
        one = format_alignment(lib, capi.CvxResult.from_buffer_copy(results[i].tobytes()), ops, t, want_nm=False, scalar_twin=True)
        for k in ("ret", "score_bits", "position_offset", "qstart", "qend", "nm", "alignment_length", "cigar_op_count", "sv_type", "cigar", "md"):
            assert twin[i][k] == one[k], (t.tag, k)
        assert (twin[i]["cigar_op_count"], twin[i]["sv_type"]) == (capi.NOT_WRITTEN, capi.NOT_WRITTEN)
        assert fast[i]["cigar"] == twin[i]["cigar"] and fast[i]["sv_type"] == 0 and (fast[i]["cigar_op_count"] > 0) == (fast[i]["ret"] >= 0)
    assert sum(x["ret"] >= 0 for x in twin) >= 15


def test_the_included_kernel_text_includes_nothing_of_the_oracle():
    """cvx_fill_ring.inc is product source like the .hip file that includes it: no oracle header, no reference path."""
    text = open(os.path.join(ROOT, "ngmlr_amd", "csrc", "cvx_fill_ring.inc")).read()
    assert not re.search(r"#include\s*[<\"][^>\"]*oracle", text)
    assert "dlopen" not in text and "libcvx_oracle" not in text and "#include" not in text


def test_kernel_class_selection_of_twin_handles(tmp_path):
    """tests/cpp/twin_host_logic_test.cpp: fill_semantics / twin_mismatch_x and host_plan_rows with the twin's tuning."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "twin_host_logic_test"
    subprocess.run([gxx, "-O1", "-std=c++17", "-pthread", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "ngmlr_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "twin_host_logic_test.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "twin_host_logic_test: ok" in r.stdout
