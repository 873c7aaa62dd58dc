"""CPU: the tiling contract of the split-bf16 GRU-mode convolutions (csrc/nlspn_gconv_x3.h).

tests/gconv_x3_plan_check.cpp, a host-only program (no device, no HIP header, no Python), runs
the planner (gc_tile) and the kernel's window arithmetic (gc_window) over every preset of
NLSPN_GCX3_CONFIGS x heights {1, 2, 3, 7, 17, 29} x widths 1..400, stages every tile's window
cell by cell as the kernel's LDS-DMA offsets do, and for every pixel, tap and lane group
requires the B fragment's 16-byte cell to be a staged one holding that lane group's cell block
(hi or lo of a channel block) of the convolution's own input pixel, and the A fragments to be
the hi and lo weights of the same channel block inside the chunk's staged weights.  Every pixel
is covered once, each preset's LDS bytes are within the 160 KB budget, and GRU1's workgroup map
hits every (co tile, pixel tile) pair once for batch sizes 1, 2 and 8.  No grid is refused.
"""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nlspn_eccv20_amd", "csrc")
IDS = [64, 65, 66, 67, 68]
HEIGHTS = [1, 2, 3, 7, 17, 29]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    path = str(tmp_path_factory.mktemp("gconv_x3_plan") / "gconv_x3_plan_check")
    out = subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-I", CSRC, os.path.join(ROOT, "tests", "gconv_x3_plan_check.cpp"),
                          "-o", path], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    return path


@pytest.fixture(scope="module")
def report(exe):
    run = subprocess.run([exe], capture_output=True, text=True, env={})
    assert run.returncode == 0, run.stderr[-2000:]
    return json.loads(run.stdout)


def test_every_fragment_read_is_a_staged_cell_of_its_own_channels(report):
    assert report["grids"] == len(IDS) * len(HEIGHTS) * 400
    assert report["violations"] == 0, report["first"]
    assert report["first"] == [] and report["refused"] == 0
    # every pixel of every grid: 9 taps (transposed: the 4 of the phases' union) x 4 lane groups
    pixels = sum(gh * gw for gh in HEIGHTS for gw in range(1, 401))
    assert report["reads"] == pixels * (9 * 3 + 4 * 2) * 4
    assert report["staged"] > 0
    assert report["gru1_maps"] == len(HEIGHTS) * 400 * 3 * 2   # batch 1, 2, 8 x hc 128, 256, the GRU1 preset


def test_lds_budget_and_geometry(report):
    assert [p["id"] for p in report["presets"]] == IDS
    assert report["lds_budget"] == 160 * 1024
    for p in report["presets"]:
        assert 0 < p["lds"] <= report["lds_budget"], p
        assert p["ccb"] % 4 == 0 and (p["xr"] * p["xp"]) % 16 == 0, p   # k-step; bank slots of the lane groups
        assert p["chunk_channels"] == 16, p                              # hi and lo of two 8-channel blocks
    lds = {p["id"]: p["lds"] for p in report["presets"]}
    # two stages of [4][taps][co] + [4][XR][XP] cells of 16 bytes, each rounded to 256 cells
    assert lds[64] == 2 * (4 * 9 * 64 + 2048) * 16 and lds[65] == lds[66] == 2 * (4 * 9 * 64 + 1024) * 16
    assert lds[67] == 2 * (4 * 4 * 64 + 1024) * 16 and lds[68] == 2 * (256 + 2048) * 16


def _one(exe, *args):
    run = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, env={})
    assert run.returncode == 0, run.stderr[-2000:]
    return json.loads(run.stdout)


# (preset, gh, gw, a band width wider than the window pitch holds)
@pytest.mark.parametrize("pid,gh,gw,bw", [(64, 14, 100, 60), (65, 17, 100, 60), (66, 17, 100, 60), (67, 17, 100, 60),
                                          (68, 27, 200, 120)])
def test_the_check_sees_a_forced_band_width_and_a_shifted_pitch(exe, pid, gh, gw, bw):
    """The plan is clean; a band wider than the pitch allows is reported as a window overrun, and
    reads at a pitch one cell off the staging's are reported cell by cell (so neither check is
    vacuous)."""
    assert _one(exe, pid, gh, gw) == []
    wide = _one(exe, pid, gh, gw, bw)
    assert wide and all("window" in v["detail"] for v in wide), wide
    for shift in (1, -1):
        off = _one(exe, pid, gh, gw, 0, shift)
        assert off and all("is not that input cell" in v["detail"] for v in off), off
