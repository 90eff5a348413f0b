"""CPU: plan_kernel's per-tile corridor analysis (ngmlr_amd/csrc/cvx_plan_logic.h, compiled for the host) -- the strip form that
plan_kernel<256> runs and the on-demand form of plan_kernel<64> -- against the brute-force restatement next to it, on every
field of the plan record: affine closed forms over slopes, widths and heights on both sides of the strip and of the staged
stretch, constant corridors, explicit rows (a decreasing row start, a shrinking row end, zero-length rows, empty corridors),
40 000-row tiles (the kPlanWrap16 logic) and 2 000 seeded random corridors (tests/cpp/plan_logic_test.cpp)."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROGRAM = os.path.join(ROOT, "ngmlr_amd", "plan_logic_test")


def test_strip_form_equals_the_brute_force_restatement(built):
    res = subprocess.run([PROGRAM], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert res.returncode == 0 and res.stdout.strip().endswith("ok"), res.stdout[-3000:]
    fam = {m.group(1).strip(): [int(x) for x in m.groups()[1:]] for m in re.finditer(
        r"^(.+?)\s+(\d+) tiles,\s+(\d+) irregular,\s+(\d+) empty,\s+(\d+) wrap16,\s+(\d+) with need beyond the staged stretch: equal$", res.stdout, re.M)}
    assert set(fam) == {"affine closed forms", "constant corridors", "explicit rows", "40 000 rows", "2 000 random corridors"}, res.stdout
    # the families do what they are for: the fall-back past the staged stretch runs, irregular and empty corridors and the wrap flag occur
    assert fam["affine closed forms"][0] >= 5 * 7 * 14 and fam["affine closed forms"][4] > 0
    assert fam["explicit rows"][1] > 0 and fam["explicit rows"][2] > 0
    assert fam["40 000 rows"][3] >= 3
    assert fam["2 000 random corridors"][0] == 2000 and fam["2 000 random corridors"][1] > 0
