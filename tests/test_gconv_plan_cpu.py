"""CPU: the tiling contract of the GRU-mode convolutions (csrc/nlspn_gconv_plan.h).

The planner (gc_tile) sizes a tile's pixel count so that the input rows it spans fit the LDS
window the kernel stages; the kernel (gc_window) cuts every column band, the narrower last one
included, into runs of that size.  A run the planner undersized for reads one row past the
staged window: a wrong value, no fault, and invisible at every grid whose bands divide evenly.
tests/gconv_plan_check.cpp, a host-only program (no device, no HIP header, no Python), runs
both functions — the ones the launcher and the kernel call — over every preset x grid 1..64 x
1..400 and the scale grids of 480x640, 375x1242, 352x1216 and 228x304, and reports every tile
whose window exceeds XR rows / XP columns, every band its tiles do not partition, and every
GRU1 workgroup map that misses or repeats a (co tile, pixel tile) pair.

Sizing npx by the widest band alone (the planner before this test) the program reported
222,793 window violations, presets 0 / 20 / 34, 1 / 35, 2 / 17, 5 / 22 / 25 / 33, 18 and 23, the
first of each at 6x97, 17x37, 17x39, 22x241, 22x39 and 4x154 (and at 14x23, 10x21, 23x39, 27x160,
NYU's 120x160 decoder grid and raw KITTI's 47x156 and 94x311 encoder grids).

The plans of the benchmark grids (tests/golden/gconv_plans.json, recorded from that planner:
their bands divide evenly, so they were right) must not move: a fix that changed them would
change the benchmark.
"""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nlspn_eccv20_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "gconv_plans.json")
IDS = [0, 1, 2, 3, 4, 5, 16, 17, 18, 20, 21, 22, 23, 24, 25, 32, 33, 34, 35, 36]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    path = str(tmp_path_factory.mktemp("gconv_plan") / "gconv_plan_check")
    out = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-I", CSRC, os.path.join(ROOT, "tests", "gconv_plan_check.cpp"),
                          "-o", path], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    return path


@pytest.fixture(scope="module")
def report(exe):
    run = subprocess.run([exe], capture_output=True, text=True, env={})
    assert run.returncode == 0, run.stderr[-2000:]
    return json.loads(run.stdout)


def test_every_tile_fits_its_window_and_every_pixel_is_tiled_once(report):
    # 20 presets x (64 x 400 grids + 12 scale grids); GRU1: 3 presets x 2 widths x (512 + 12) counts
    assert report["grids"] == len(IDS) * (64 * 400 + 12)
    assert report["gru1_maps"] == 3 * 2 * (512 + 12)
    assert report["violations"] == 0, report["first_per_preset"]
    assert report["first"] == []
    # a pixel always fits: no grid is refused (a refusal would be NLSPN_EUNSUPPORTED, never a bad plan)
    assert report["refused"] == 0


# (preset, gh, gw, the tile size the widest band alone allows): grids whose last band overran
OVERRUN = ((0, 14, 23, 49), (20, 14, 23, 49), (23, 10, 21, 23), (1, 17, 37, 58), (2, 17, 39, 61), (17, 17, 39, 61),
           (18, 23, 39, 101), (5, 27, 160, 217), (25, 27, 160, 217), (5, 120, 160, 217), (0, 47, 156, 64), (0, 94, 311, 64),
           (34, 34, 78, 64))


def _one(exe, *args):
    run = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, env={})
    assert run.returncode == 0, run.stderr[-2000:]
    return json.loads(run.stdout)


@pytest.mark.parametrize("pid,gh,gw,npx_wide", OVERRUN)
def test_the_last_band_sizes_the_tile(exe, pid, gh, gw, npx_wide):
    """At the grids that overran, the plan is clean and its tile is smaller than the widest
    band alone allows; with that larger tile forced the program reports the window overrun
    (so the check is not vacuous: it sees the defect it was written for)."""
    assert _one(exe, pid, gh, gw) == []
    bad = _one(exe, pid, gh, gw, npx_wide)
    assert bad and all(v["rule"] == "a" and v["band"] == v["nbands"] - 1 for v in bad), bad
    assert "window" in bad[0]["detail"]


def test_benchmark_plans_are_the_recorded_ones(report):
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert len(golden) == len(IDS) * 8 and {r["preset"] for r in golden} == set(IDS)
    assert {(r["gh"], r["gw"]) for r in golden} >= {(29, 38), (30, 152), (57, 76), (60, 304), (58, 76), (116, 152), (120, 608)}
    assert all(r["planned"] for r in golden)
    assert report["plans"] == golden, [(g, w) for g, w in zip(report["plans"], golden) if g != w][:5]
    # spot rows: the 1/8-scale NYU grid is one 38-wide band of full tiles in the GRU presets
    rows = {(r["preset"], r["gh"], r["gw"]): r for r in golden}
    assert (rows[2, 29, 38]["bw"], rows[2, 29, 38]["nbands"], rows[2, 29, 38]["npx"]) == (38, 1, 64)
    assert (rows[0, 30, 152]["bw"], rows[0, 30, 152]["nbands"]) == (19, 8)
