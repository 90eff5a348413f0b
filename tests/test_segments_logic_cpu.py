"""CPU: alignment queries as segments of a read block, host half.  tests/cpp/segments_logic_test.cpp (validation, the chunk split
against a brute-force enumeration, the upload schedule's segments mode) built with plain g++ under -fsanitize=address,undefined --
the program has its own main and is never loaded into Python -- and the C ABI's host restatement, cvx_stage_segments_host, against
the rule written out in Python."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.segment_cases import want_string

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_segments_logic(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "segments_logic_test"
    subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "ngmlr_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "segments_logic_test.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "segments_logic_test: ok" in r.stdout


def test_abi_has_the_segment_entries(built):
    from ngmlr_amd import capi
    lib = capi.load()
    for name in ("cvx_submit_segments", "cvx_stage_segments", "cvx_stage_segments_host"):
        assert hasattr(lib, name) and name in capi.EXPORTS, name
    assert lib.cvx_abi_version() == 9      # additive


def test_host_restatement_through_the_abi(built):
    """every byte value, both directions, empty strings, a read used by several strings; the arena is left as it was"""
    from ngmlr_amd import capi
    from ngmlr_amd.aligner import stage_segments_host, KmerIndex
    lib = capi.load()
    rng = np.random.default_rng(3)
    reads = [bytes(range(1, 256)), b"ACGTNacgtnRYKM*-", b"", b"G"] + [bytes(rng.choice(list(b"ACGTNacgt"), size=n).astype(np.uint8)) for n in (300, 4097, 9000)]
    segs, lens = [], []
    for r, rd in enumerate(reads):
        for k in range(12):
            start = int(rng.integers(0, len(rd) + 1))
            length = 0 if k == 11 else int(rng.integers(0, len(rd) - start + 1))
            segs.append((r, start, k & 1))
            lens.append(length)
        segs += [(r, 0, 0), (r, 0, 1)]
        lens += [len(rd), len(rd)]
    arena, offsets, _ = KmerIndex.make_arena(reads)
    before = arena.copy()
    got = stage_segments_host(lib, (arena, offsets), segs, lens)
    assert (arena == before).all()
    assert got == [want_string(reads[r], s, n, f) for (r, s, f), n in zip(segs, lens)]
    assert stage_segments_host(lib, (arena, offsets), [], []) == []


def test_argument_errors_through_the_abi(built):
    import ctypes as C
    from ngmlr_amd import capi
    from ngmlr_amd.aligner import stage_segments_host, KmerIndex, _segments
    lib = capi.load()
    reads = [b"ACGTACGTAC", b"GG"]
    for seg, length in (((2, 0, 0), 1), ((-1, 0, 0), 1), ((0, -1, 0), 1), ((0, 4, 0), 7), ((1, 0, 1), 3), ((0, 0, 2), 1), ((0, 0, 0), -1)):
        with pytest.raises(capi.CvxError) as e:
            stage_segments_host(lib, reads, [seg], [length])
        assert e.value.code == -3, (seg, length)
    arena, offsets, _ = KmerIndex.make_arena(reads)
    bad = offsets.copy()
    bad[1] = bad[2]                                   # read 1 without even its NUL
    with pytest.raises(capi.CvxError) as e:
        stage_segments_host(lib, (arena, bad), [(0, 0, 0)], [1])
    assert e.value.code == -3 and "ascend" in str(e.value)
    # too small an arena: CVX_ERR_CAPACITY, the size and the offsets still reported
    seg, ln = _segments([(0, 0, 0), (0, 2, 1)]), np.array([10, 8], dtype=np.int32)
    out, qo, used = np.zeros(32, dtype=np.uint8), np.zeros(2, dtype=np.uint64), C.c_uint64()
    rc = lib.cvx_stage_segments_host(2, arena.ctypes.data, offsets.ctypes.data, 2, seg.ctypes.data, ln.ctypes.data, out.ctypes.data, 17, qo.ctypes.data, C.byref(used))
    assert rc == -6 and used.value == 18 and list(qo) == [0, 10] and not out.any()


def test_read_note_on_threads(built, tmp_path):
    """Convex::DeviceReads (the drop-in's self-describing placeholder of a query): several live noted buffers in one context,
    against the library, no device"""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "read_note_test"
    lib_dir = os.path.join(ROOT, "ngmlr_amd")
    subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-pthread", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "ngmlr_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "read_note_test.cpp"), "-o", str(exe),
                    "-L" + lib_dir, "-lcvxalign", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"],
                   check=True, capture_output=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "read_note_test: ok" in r.stdout
