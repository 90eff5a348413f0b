"""CPU (hipcc cross-compiles): the compiled shape of the FAST ring fills -- fill_ring_kernel / fill_ring_twin_kernel
<M, false, kFillTwoPhase, TAB, 1>, M = 1 .. 4, the kernels of every default handle's and the scalar twin's ring classes -- after the
cell update lost its multiply and its separate zero clamp (cvx_fill_ring.inc):

  - no scratch segment and no spilled register in any of the eight;
  - the waves per SIMD the registers and the LDS allow are the ones the parent had -- 8, 8, 7, 5 for M = 1 .. 4 (the M = 3 figure is
    what fill_two_phase_waves_per_simd reports on the device and what the tail split sizes its resident round by);
  - the zero clamp is the clamp bit of the maximum (no v_max against a constant 0 is left in the step loop's cell update) and the
    gap-extension offer has no multiply: the step loop holds no v_mul_f32 by -2^100.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ngmlr_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
PARENT_WAVES = {1: 8, 2: 8, 3: 7, 4: 5}
VGPRS_PER_SIMD_LANE, VGPR_GRANULE, MAX_WAVES, LDS_PER_CU = 512, 8, 8, 160 * 1024      # gfx950


@pytest.fixture(scope="module")
def device_asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("asm") / "cvx_kernels.s"
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-honor-nans", "-fPIC",
           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S", "--cuda-device-only",
           os.path.join(CSRC, "cvx_kernels.hip"), "-o", str(out)]
    subprocess.run(cmd, check=True, capture_output=True, timeout=900)
    return out.read_text()


def _fast_kernels(txt):
    for m in re.finditer(r"^(_ZN3cvx(?:16fill_ring_kernel|21fill_ring_twin_kernel)ILi([1-4])ELb0ELi0ELb1ELi1EEEvNS_8FillArgsE):", txt, re.M):
        body = txt[m.start():]
        yield m.group(1), int(m.group(2)), body[:body.index(".end_amdhsa_kernel")]


def _meta(txt, name, key):
    """a key of the kernel's record in the code object's metadata (one record per kernel, each opening with .agpr_count)"""
    recs = [r for r in txt.split("\n  - .agpr_count:") if re.search(r"\n\s+\.name:\s+%s\n" % re.escape(name), r)]
    assert len(recs) == 1, name
    return int(re.search(r"\n\s+\.%s:\s+(\d+)" % key, recs[0]).group(1))


def test_fast_fills_keep_scratch_free_and_their_waves(device_asm):
    seen = 0
    for name, M, body in _fast_kernels(device_asm):
        seen += 1
        assert _meta(device_asm, name, "private_segment_fixed_size") == 0, name
        assert _meta(device_asm, name, "vgpr_spill_count") == 0 and _meta(device_asm, name, "sgpr_spill_count") == 0, name
        vg = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", body).group(1))
        vg = (vg + VGPR_GRANULE - 1) // VGPR_GRANULE * VGPR_GRANULE
        lds = _meta(device_asm, name, "group_segment_fixed_size")
        waves = min(MAX_WAVES, VGPRS_PER_SIMD_LANE // vg, (LDS_PER_CU // max(lds, 1)) // 4)
        assert waves >= PARENT_WAVES[M], (name, vg, lds, waves)
        if M == 3:
            assert waves == 7, (name, vg, lds)      # (the kernel asks for exactly seven: fill_waves_min / fill_waves_max, cvx_kernels.hip)
    assert seen == 8


def test_fast_cell_update_has_the_clamp_bit_and_no_multiply(device_asm):
    for name, M, body in _fast_kernels(device_asm):
        clamped = len(re.findall(r"^\s+v_max3?_f32\w* .* clamp", body, re.M))
        assert clamped >= 4 * M, (name, clamped)                       # one per slot and step of the unrolled group, in either tracking phase
        assert not re.search(r"^\s+v_mul_f32\w* .*0xf1800000", body, re.M), name      # -2^100
        assert not re.search(r"^\s+v_max3_f32 v\d+, v\d+, v\d+, 0\s*$", body, re.M), name


def _built_rule():
    """the instantiations the launcher's selector (pick_fill, cvx_kernels.hip) reaches: (kernel, M, wrap, mode, table, gang)"""
    two_phase, exact, chain = 0, 1, 2
    want = set()
    for kernel in ("16fill_ring_kernel", "21fill_ring_twin_kernel"):
        for M in (1, 2, 3, 4):
            for wrap in (0, 1):
                want.add((kernel, M, wrap, two_phase, 0, 1))
                want.add((kernel, M, wrap, exact, 0, 1))
                if M != 3:
                    want.add((kernel, M, wrap, chain, 0, 1))      # (chained row blocks: rings of a power of two)
            want.add((kernel, M, 0, two_phase, 1, 1))             # the penalty table: float runs, two-phase
    for G in (2, 3):                                              # gangs: M = 3, float runs, whole tiles, not for the twin
        want.update({("16fill_ring_kernel", 3, 0, exact, 0, G), ("16fill_ring_kernel", 3, 0, two_phase, 0, G), ("16fill_ring_kernel", 3, 0, two_phase, 1, G)})
    return want


def test_code_object_holds_exactly_the_fill_kernels_of_the_rule(device_asm):
    want = {"_ZN3cvx%sILi%dELb%dELi%dELb%dELi%dEEEvNS_8FillArgsE" % k for k in _built_rule()}
    assert len(want) == 58
    got = set(re.findall(r"^(_ZN3cvx(?:16fill_ring_kernel|21fill_ring_twin_kernel)I\w+): *(?:;.*)?$", device_asm, re.M))
    assert got == want, (sorted(got - want), sorted(want - got))
