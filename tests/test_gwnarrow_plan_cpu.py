"""CPU: the plan, the staging and the LDS addressing of the streaming weight gradient of the
narrow layers (csrc/nlspn_gwnarrow.h, csrc/nlspn_gwnarrow_plan.h).

tests/gwnarrow_plan_check.cpp, a host-only program (no device, no HIP header, no Python), plans
with gwn_plan (the launcher's function) for Cs, Cl in {1, 3, 8, 9, 16} x Ws 1..400 x a few (B, Hs)
and the cropped large sizes (one short, seven short), replays the staging of every unit with the
kernel's own functions (lines, 16-byte chunks from the boundary at or before the first column,
dword loads at the row's ends, zeros) and walks every read of the k-loop and of the large-side
bias sum: inside what the staging wrote for that unit and holding the correlation's own element
or a zero; every 16-byte load aligned and inside its row.  The units of all slices hit every
(image, small row, band) once, the owned large pixels every stored pixel once; every kernel's
LDS is within 160 KB; the workspace is a pure function of the shape and the C ABI's query returns
the plan's; the Python mirror of tests/_gwnarrow_cases.py equals the plan field by field."""
import json
import os
import shutil
import subprocess

import pytest

import _gwnarrow_cases as nc
from nlspn_eccv20_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nlspn_eccv20_amd", "csrc")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    path = str(tmp_path_factory.mktemp("gwnarrow_plan") / "gwnarrow_plan_check")
    out = subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-I", CSRC, os.path.join(ROOT, "tests", "gwnarrow_plan_check.cpp"),
                          "-o", path], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    return path


def _one(exe, *args):
    run = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, env={})
    assert run.returncode == 0, run.stderr[-2000:]
    return json.loads(run.stdout)


@pytest.fixture(scope="module")
def report(exe):
    return _one(exe)


def test_every_load_and_read_over_the_sweep(report):
    assert report["violations"] == 0 and report["first"] == [], report["first"]
    # per (Cs, Cl): Ws 1..130 x two (B, Hs) and 131..400 x one; one short at every Ws; seven short from Ws = 4 on
    assert report["grids"] == 25 * (130 * 2 + 270 + 400 + 397)
    assert report["units"] > report["grids"] and report["reads"] > 1000 * report["units"]
    assert report["vector_loads"] > 10 * report["dword_loads"] > 0   # the rows go by 16 bytes, their ends by dwords


def test_lds_budget_and_constants(report):
    assert report["lds_budget"] == 160 * 1024
    assert (report["rows"], report["waves"], report["band_max"], report["target_wgs"]) == (nc.R, nc.NW, nc.BW, nc.TARGET)
    assert [k["nb"] for k in report["kernels"]] == list(range(1, 10))
    for k in report["kernels"]:
        assert k["clmax"] == 16 * k["nb"] // 9 and -(-9 * k["clmax"] // 16) == k["nb"]
        stage, red = nc.R * 16 * nc.GP + k["clmax"] * nc.XCP, nc.NW * (k["nb"] * 256 + 64)
        assert 0 < k["lds"] == 4 * (max(stage, red) + 16) <= report["lds_budget"], k
    assert [k["clmax"] for k in report["kernels"] if k["nb"] in (1, 5, 6, 9)] == [1, 8, 10, 16]


@pytest.mark.parametrize("cid", [c["id"] for c in nc.CASES])
def test_plan_is_the_mirrors_and_the_workspace_query(exe, cid):
    c = nc.BY_ID[cid]
    a, m = _one(exe, *nc.shape_of(c)), nc.plan_of(c)
    assert a == _one(exe, *nc.shape_of(c)) and a["covers"] == 1 and a["violations"] == []
    for k in ("nb", "nbands", "bw", "ngroups", "units", "ups", "nsl", "lds_bytes", "slab", "floats"):
        assert a[k] == m[k], (k, a, m)
    assert _lib.get().nlspn_gconv_wgrad_narrow_workspace_bytes(*nc.shape_of(c)) == 4 * a["floats"]


def test_covers_grid_is_the_mirrors(exe):
    bits = _one(exe, "covers")["covers"]
    want = "".join(str(int(nc.gwn_covers(st, Cs, c0, c1))) for st in range(4) for Cs in range(19) for c0 in range(19) for c1 in (0, 16))
    assert bits == want and bits.count("1") == 256


@pytest.mark.parametrize("shape,bw,shift,what", [
    ((2, 16, 9, 3, 5, 65, 9, 129), 70, 0, "not the small tensor's element"),   # a band wider than the LDS row
    ((2, 3, 8, 1, 6, 100, 5, 193), 100, 0, "not"),
    ((2, 16, 1, 2, 5, 38, 10, 76), 0, 1, "not the small tensor's element"),    # every read one float on
    ((2, 8, 16, 1, 4, 64, 8, 128), 0, 150, "not"),                             # a window row pitch on
])
def test_the_check_sees_a_bad_band_or_pitch(exe, shape, bw, shift, what):
    """The plan is clean; with a band width the plan would not choose, or every read address
    shifted as a wrong pitch would shift it, the program reports violations."""
    assert _one(exe, *shape)["violations"] == []
    bad = _one(exe, *shape, bw, shift)["violations"]
    assert bad and any(what in v["detail"] for v in bad), bad
