"""CPU: the tiling contract of the f16-operand GRU-mode convolutions (csrc/nlspn_gconv16.h).

tests/gconv16_plan_check.cpp, a host-only program (no device, no HIP header, no Python), runs
the planner (gc_tile) and the kernel's window arithmetic (gc_window) — the functions the
launcher and the kernel call — over every preset of NLSPN_GC16_CONFIGS x grid 1..64 x 1..400,
and for every non-empty tile walks every tap of every pixel: the cell the kernel reads must lie
inside the staged window's rows and columns (for the stride-2 preset: at the even / odd-split
cell the staging wrote it to) and stand for the convolution's own input cell.  This is the
property the 20 | 19 band defect of the f32 family violated.  Each preset's LDS bytes must be
within the 160 KB budget.  No grid is refused (one pixel always fits a window), so
NLSPN_EUNSUPPORTED is unreachable for these presets.
"""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nlspn_eccv20_amd", "csrc")
IDS = [48, 49, 50, 51, 52]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    path = str(tmp_path_factory.mktemp("gconv16_plan") / "gconv16_plan_check")
    out = subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-I", CSRC, os.path.join(ROOT, "tests", "gconv16_plan_check.cpp"),
                          "-o", path], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    return path


@pytest.fixture(scope="module")
def report(exe):
    run = subprocess.run([exe], capture_output=True, text=True, env={})
    assert run.returncode == 0, run.stderr[-2000:]
    return json.loads(run.stdout)


def test_every_tap_of_every_pixel_lies_inside_the_staged_window(report):
    assert report["grids"] == len(IDS) * 64 * 400
    assert report["violations"] == 0, report["first"]
    assert report["first"] == [] and report["refused"] == 0
    # every pixel of every grid, 9 taps (transposed: the 4 of the phases' union)
    pixels = sum(gh * gw for gh in range(1, 65) for gw in range(1, 401))
    assert report["taps"] == pixels * (9 * 3 + 4 * 2)
    assert report["gru1_maps"] == 2 * 512


def test_lds_budget_and_geometry(report):
    assert [p["id"] for p in report["presets"]] == IDS
    assert report["lds_budget"] == 160 * 1024
    for p in report["presets"]:
        assert 0 < p["lds"] <= report["lds_budget"], p
        assert p["ccb"] % 4 == 0 and (p["xr"] * p["xp"]) % 16 == 0, p   # k-step; bank slots of the lane groups
    lds = {p["id"]: p["lds"] for p in report["presets"]}
    # two stages of [4][taps][co] + [4][XR][XP] cells of 16 bytes, each rounded to 256 cells
    assert lds[48] == 2 * (4 * 9 * 64 + 2048) * 16 and lds[49] == lds[50] == 2 * (4 * 9 * 64 + 1024) * 16
    assert lds[51] == 2 * (4 * 4 * 64 + 1024) * 16 and lds[52] == 2 * (256 + 2048) * 16


def _one(exe, *args):
    run = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, env={})
    assert run.returncode == 0, run.stderr[-2000:]
    return json.loads(run.stdout)


# (preset, gh, gw, a forced tile size, uneven): for the stride-2 and stride-1 presets the tile the
# widest band alone would allow at a grid whose last band is narrower (the f32 family's defect);
# the transposed presets' 6 window rows hold a full tile in any band wide enough to have a
# neighbour, so theirs is just an oversized tile
@pytest.mark.parametrize("pid,gh,gw,npx,uneven", [(48, 14, 23, 49, True), (49, 17, 39, 61, True), (50, 17, 39, 61, True),
                                                  (51, 17, 41, 200, False), (52, 27, 160, 400, False)])
def test_the_check_sees_an_oversized_tile(exe, pid, gh, gw, npx, uneven):
    """The plan is clean; with the larger tile forced the program reports the window overrun
    (so the check is not vacuous), for the uneven grids in the last band only."""
    assert _one(exe, pid, gh, gw) == []
    bad = _one(exe, pid, gh, gw, npx)
    assert bad and "window" in bad[0]["detail"], bad
    if uneven:
        assert all(v["band"] == v["nbands"] - 1 for v in bad), bad
