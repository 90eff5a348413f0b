"""CPU (hipcc cross-compiles): the FAST ring fills -- fill_ring_kernel / fill_ring_twin_kernel <M, false, kFillTwoPhase, TAB, 1>,
M = 1 .. 4 -- apply a lane's row activity through EXEC (cvx_fill_ring.inc, phase1): one block of inline assembly
per slot and step, v_cmpx_lt_u32 (EXEC = cnt < len), the clamped v_max3_f32 into a register that holds zero, the three equality
compares, EXEC back to all lanes.  From the device assembly:

  - in every FAST kernel there is one v_cmpx_lt_u32 per clamped v_max3_f32 (and at least one per slot and step of the unrolled group);
  - after each v_cmpx, EXEC is restored (s_mov_b64 exec) before anything that must run on every lane of the wave or that ends the
    straight line: the plane words' v_addc_co_u32, a DPP op, a ds_read, a store, v_add_u32 (the column counter) or a branch -- and
    within the five instructions a DPP op needs between a VALU write of EXEC and itself, the compiler not looking inside the block;
  - no other fill kernel (arithmetic, int16 runs, exact, chain, gangs) contains a v_cmpx.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ngmlr_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
FAST = re.compile(r"^_ZN3cvx(?:16fill_ring_kernel|21fill_ring_twin_kernel)ILi([1-4])ELb0ELi0ELb1ELi1EEEvNS_8FillArgsE$")
FORBIDDEN_UNDER_ROW_EXEC = re.compile(r"^(v_addc_co_u32|v_add_u32|ds_read|ds_write|global_store|flat_store|buffer_store|scratch_store|s_c?branch|\w+_dpp\b)|\b(?:wave_ror|wave_rol|wave_shr|wave_shl|row_shr|row_shl|row_ror|row_bcast|quad_perm|row_mirror|row_half_mirror)\b")


@pytest.fixture(scope="module")
def fill_kernels(tmp_path_factory):
    """{mangled name: [instruction lines]} of every fill_ring kernel of the code object"""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("asm") / "cvx_kernels.s"
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-honor-nans", "-fPIC",
           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S", "--cuda-device-only",
           os.path.join(CSRC, "cvx_kernels.hip"), "-o", str(out)]
    subprocess.run(cmd, check=True, capture_output=True, timeout=900)
    txt = out.read_text()
    kernels = {}
    for m in re.finditer(r"^(_ZN3cvx(?:16fill_ring_kernel|21fill_ring_twin_kernel)I\w+): *(?:;.*)?$", txt, re.M):
        body = txt[m.end():]
        body = body[:body.index(".end_amdhsa_kernel")]
        lines = [l.split(";")[0].strip() for l in body.split("\n")]
        kernels[m.group(1)] = [l for l in lines if l and not l.startswith(".") and not l.endswith(":")]
    assert len(kernels) == 58
    return kernels


def test_one_cmpx_per_clamped_maximum_in_every_fast_kernel(fill_kernels):
    seen = 0
    for name, lines in fill_kernels.items():
        m = FAST.match(name)
        if not m:
            continue
        seen += 1
        M = int(m.group(1))
        cmpx = sum(1 for l in lines if l.startswith("v_cmpx_lt_u32"))
        clamped = sum(1 for l in lines if re.match(r"v_max3_f32\w* .* clamp$", l))
        assert cmpx == clamped, (name, cmpx, clamped)
        assert cmpx >= 2 * 4 * M, (name, cmpx)      # the early and the exactly tracked step loop, four steps of M slots each
        assert not any(l.startswith("v_cmpx") and not l.startswith("v_cmpx_lt_u32") for l in lines), name
    assert seen == 8


def test_exec_is_restored_before_anything_that_needs_every_lane(fill_kernels):
    for name, lines in fill_kernels.items():
        if not FAST.match(name):
            continue
        for i, l in enumerate(lines):
            if not l.startswith("v_cmpx"):
                continue
            k = i + 1
            while k < len(lines) and not re.match(r"s_mov_b64 exec\b", lines[k]):
                assert not FORBIDDEN_UNDER_ROW_EXEC.search(lines[k]), (name, i, lines[i:k + 1])
                k += 1
            assert k < len(lines), (name, i)
            # v_max3, three compares, the restore: EXEC is narrowed for exactly the block, and whatever follows it has the five
            # instructions between the VALU write of EXEC and itself that a DPP op needs
            assert k - i == 5, (name, i, lines[i:k + 1])
            assert re.match(r"v_max3_f32\w* .* clamp$", lines[i + 1]), (name, lines[i:k + 1])
            assert all(q.startswith("v_cmp_eq_f32") for q in lines[i + 2:k]), (name, lines[i:k + 1])


def test_no_other_fill_kernel_has_a_cmpx(fill_kernels):
    others = 0
    for name, lines in fill_kernels.items():
        if FAST.match(name):
            continue
        others += 1
        assert not any(l.startswith("v_cmpx") for l in lines), name
    assert others == 50
