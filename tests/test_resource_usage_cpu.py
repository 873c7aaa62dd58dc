"""CPU: the hot kernels compile without scratch spills.

The Makefile saves hipcc's -Rpass-analysis=kernel-resource-usage remarks of every
compile (build/csrc/*.ru.txt).  A spill inside the resident kernel's iteration loop
costs scratch round trips every iteration, so a spill coming back must fail a test,
not hide in the build log.  If the library has not been built here, the resident
translation unit (seconds) is compiled with the remarks on the spot.
"""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nlspn_eccv20_amd", "csrc")
sys.path.insert(0, CSRC)
import resource_usage as RU  # noqa: E402

HOT = ("prop_step_kernel", "bwd_step_kernel", "s2d_pyramid_kernel")
# The resident kernel runs at its 168-VGPR cap (768-thread launch bound = 3 waves per
# SIMD) with 80 VGPRs of tap geometry held across its iteration loop.  Since round 4 (the
# abort path moved below the iteration loop) every build compiles without scratch; a
# spill coming back must fail here.  The GROUPS builds (several image groups in turn per
# launch) wrap the iteration loop in the group loop, so it sits at depth 2.  The loop is
# also checked on the kernel's device assembly: no scratch instruction inside it.
RESIDENT_SCRATCH_CAP = 0          # bytes per lane, single-group builds
# bytes per lane, GROUPS builds: setup spill slots only (the loop check below holds them out of
# the iteration loop).  Round 6 builds: 20-28 B for the step-1 form, 20-32 B for the
# prologue-in-the-launch form (FIRST)
RESIDENT_SCRATCH_CAP_GROUPS = 32
RESIDENT_SCRATCH_CAP_GROUPS_FIRST = 40
RESIDENT_LOOP_RELOADS = 0         # scratch instructions inside the iteration loop, per instantiation
RESIDENT_LOOP_RELOADS_F16 = 0     # the fp16 builds alike


def _groups(name):
    # template <T, KH, KW, MAXNT, SMAX, NTC, GROUPS, FIRST, PXO>: GROUPS is the first of the two bools
    return re.search(r"ELb1ELb[01]E", name) is not None


def _first(name):
    return re.search(r"ELb[01]ELb1E", name) is not None


def _scratch_cap(name):
    if not _groups(name):
        return RESIDENT_SCRATCH_CAP
    return RESIDENT_SCRATCH_CAP_GROUPS_FIRST if _first(name) else RESIDENT_SCRATCH_CAP_GROUPS


_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-slp-vectorize"]


def _rows(tmp):
    rows = RU.load_build()
    if any("prop_resident_kernel" in n for n in rows):
        return rows
    out = subprocess.run(["/opt/rocm/bin/hipcc", *_FLAGS, "-Rpass-analysis=kernel-resource-usage", "-c", "-o",
                          os.path.join(tmp, "nlspn_ru_test.o"), os.path.join(CSRC, "nlspn_kern_resident.hip")],
                         capture_output=True, text=True, cwd=CSRC)
    assert out.returncode == 0, out.stderr[-2000:]
    return RU.parse(out.stderr)


def test_hot_kernels_have_no_scratch():
    rows = RU.load_build()
    if not rows:
        pytest.skip("library not built here (make -C nlspn_eccv20_amd/csrc writes the remarks)")
    hot = {n: r for n, r in rows.items() if any(h in n for h in HOT)}
    assert any("prop_step_kernel" in n for n in hot), "step kernel remarks missing"
    spilled = {n: r.get("ScratchSize") for n, r in hot.items() if r.get("ScratchSize", 0) != 0}
    assert not spilled, f"scratch spills in hot kernels: {spilled}"
    vspill = {n: r.get("VGPRs Spill") for n, r in hot.items() if r.get("VGPRs Spill", 0) != 0}
    assert not vspill, f"VGPR spills in hot kernels: {vspill}"


def test_resident_kernel_registers_and_scratch(tmp_path):
    """The resident kernel's launch bound (768 threads = 3 waves per SIMD) caps it at
    168 VGPRs; its scratch stays under the cap, and its iteration loop (nested in the
    image-group loop) holds at most RESIDENT_LOOP_RELOADS scratch instructions (device
    assembly)."""
    rows = _rows(str(tmp_path))
    res = {n: r for n, r in rows.items() if "prop_resident_kernel" in n}
    assert res and all(r["VGPRs"] <= 168 and r.get("Occupancy", 0) >= 3 for n, r in res.items()), res
    assert any("ELi576E" in n for n in res) and any("ELi128E" in n for n in res), "fixed thread-count builds missing"
    assert any(_groups(n) for n in res) and any(not _groups(n) for n in res), "GROUPS builds missing"
    over = {n: r.get("ScratchSize", 0) for n, r in res.items() if r.get("ScratchSize", 0) > _scratch_cap(n)}
    assert not over, over
    asm, asm_path = "", str(tmp_path / "nlspn_res_test.s")
    for tu in ("nlspn_kern_resident.hip", "nlspn_kern_resident_wide.hip"):  # 3x3; 1x17 and 5x5
        out = subprocess.run(["/opt/rocm/bin/hipcc", *_FLAGS, "--cuda-device-only", "-S", "-o", asm_path,
                              os.path.join(CSRC, tu)], capture_output=True, text=True, cwd=CSRC)
        assert out.returncode == 0, out.stderr[-2000:]
        with open(asm_path) as f:
            asm += f.read()
    for name in res:
        loop = RU.loop_scratch(asm, name, 2 if _groups(name) else 1)["loop"]
        cap = RESIDENT_LOOP_RELOADS_F16 if "6__half" in name else RESIDENT_LOOP_RELOADS
        assert len(loop) <= cap, (name, loop)


@pytest.mark.parametrize("text,expect", [
    ("x.h:1:1: remark: Function Name: _Zfoo [-R]\nx.h:1:1: remark:     VGPRs: 12 [-R]\n"
     "x.h:1:1: remark:     ScratchSize [bytes/lane]: 8 [-R]\n", {"_Zfoo": {"VGPRs": 12, "ScratchSize": 8}}),
])
def test_parse(text, expect):
    assert RU.parse(text) == expect
