"""CPU: the plan and the LDS addressing of the split-bf16 weight gradient (csrc/nlspn_gwgrad16.h,
csrc/nlspn_gwgrad16_plan.h).

tests/gwgrad16_plan_check.cpp, a host-only program (no device, no HIP header, no Python), plans
with gw16_plan (the launcher's function) for each of the three tilings x Ws 1..400 x a few (B, Hs)
from 1 x 1, and at stride 2 the cropped large sizes (one short and seven short), replays the
staging of every unit with the kernel's own item functions and walks every read of the k-loop
(k-step, lane group, element, tap, part, channel): aligned to its 16 bytes, inside what the
staging wrote for that unit, and holding the correlation's own element or a zero (A: zeros past
the band, the row's end and the channels).  The units of all slices hit every (image, small
row, band) once; each tiling's LDS is within 160 KB; the workspace is a pure function of the
shape and the C ABI's query returns the plan's.

The same program's "f32" mode plans with gw_plan (csrc/nlspn_gwgrad_plan.h, the f32 launcher's
function) and sweeps the four f32 tilings over the same widths, (B, Hs) and cropped sizes: bands,
slices, tiles and workspace floats.  Its plan of every weight-gradient case of
tests/_gconv_bwd_cases.py equals the Python mirror there field by field, 4 floats is the C ABI's
query, and the bias slices of the split-bf16 plan are the f32 plan's (the two entries' bias
gradients are bit-equal because they run the same launches on the same slices)."""
import json
import os
import shutil
import subprocess

import pytest

import _gconv_bwd_cases as bc
from nlspn_eccv20_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nlspn_eccv20_amd", "csrc")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    path = str(tmp_path_factory.mktemp("gwgrad16_plan") / "gwgrad16_plan_check")
    out = subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-I", CSRC, os.path.join(ROOT, "tests", "gwgrad16_plan_check.cpp"),
                          "-o", path], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    return path


@pytest.fixture(scope="module")
def report(exe):
    run = subprocess.run([exe], capture_output=True, text=True, env={})
    assert run.returncode == 0, run.stderr[-2000:]
    return json.loads(run.stdout)


def _one(exe, *args):
    run = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, env={})
    assert run.returncode == 0, run.stderr[-2000:]
    return json.loads(run.stdout)


def test_every_read_is_aligned_staged_and_the_correlations_own(report):
    assert report["violations"] == 0, report["first"]
    assert report["first"] == []
    # stride 1: two (B, Hs) up to three bands, one above; stride 2 (two tilings): the same plus the two crops
    assert report["grids"] == (130 * 2 + 270) + 2 * (130 * 2 + 270 + 400 + 397)
    assert report["units"] > report["grids"] and report["reads"] > 1000 * report["units"]


def test_lds_budget_and_tilings(report):
    assert report["lds_budget"] == 160 * 1024
    assert [t["tiling"] for t in report["tilings"]] == [0, 1, 2] and [t["S"] for t in report["tilings"]] == [1, 2, 2]
    for t in report["tilings"]:
        assert 0 < t["lds"] <= report["lds_budget"], t
        # two stages of [mt][hi, lo][64] + [nt][3][3][hi, lo][64] bf16, the channel pitches 16 elements longer
        assert t["lds"] == 2 * 2 * (t["mt"] * (2 * 64 + 16) + t["nt"] * (18 * 64 + 16)), t
        assert (t["mt"], t["nt"], t["nthr"]) == (128, 16, 256), t


# (stride, Cs, Cl, B, Hs, Ws, Hl, Wl)
SHAPES = [(1, 256, 256, 8, 29, 38, 29, 38), (1, 128, 256, 8, 29, 38, 29, 38), (2, 128, 256, 8, 29, 38, 57, 76),
          (2, 256, 16, 8, 57, 76, 114, 152), (2, 256, 16, 8, 57, 76, 114, 152), (2, 40, 24, 2, 7, 9, 13, 17),
          (1, 40, 48, 1, 3, 130, 3, 130)]


@pytest.mark.parametrize("shape", SHAPES)
def test_workspace_is_the_plans_and_a_pure_function_of_the_shape(exe, shape):
    lib = _lib.get()
    a, b = _one(exe, *shape), _one(exe, *shape)
    assert a == b and a["violations"] == []
    assert lib.nlspn_gconv_wgrad_bf16x3_workspace_bytes(*shape) == 4 * a["floats"]
    stride, Cs, Cl, B, Hs, Ws, Hl, Wl = shape
    mtiles, ntiles = -(-Cs // 128), -(-Cl // 16)
    nbands = -(-Ws // 64)
    units = B * Hs * nbands
    nsl0 = max(1, min(units, -(-256 // (mtiles * ntiles))))   # about 256 workgroups: a constant, not the CU count
    ups = -(-units // nsl0)
    nsl = -(-units // ups)
    assert (a["mtiles"], a["ntiles"], a["nbands"], a["units"], a["ups"], a["nsl"]) == (mtiles, ntiles, nbands, units, ups, nsl)
    assert a["floats"] == nsl * mtiles * 128 * ntiles * 16 * 9 + a["nsb"] * max(Cs, Cl)


def test_both_narrow_shapes_keep_the_f32_plan(exe):
    lib = _lib.get()
    for shape in ((2, 16, 9, 2, 13, 18, 25, 35), (2, 16, 8, 2, 28, 36, 50, 70), (1, 16, 16, 1, 8, 8, 8, 8)):
        assert _one(exe, *shape)["tiling"] == -1
        assert lib.nlspn_gconv_wgrad_bf16x3_workspace_bytes(*shape) == lib.nlspn_gconv_wgrad_workspace_bytes(*shape) > 0
    assert lib.nlspn_gconv_wgrad_bf16x3_workspace_bytes(3, 256, 256, 8, 29, 38, 29, 38) == 0


@pytest.mark.parametrize("shape,bw,shift,what", [
    ((2, 136, 40, 1, 4, 100, 7, 199), 70, 0, "not the small tensor's element"),   # a band wider than the LDS row
    ((1, 136, 40, 2, 3, 150, 3, 150), 75, 0, "not the small tensor's element"),
    ((1, 136, 40, 1, 2, 38, 2, 38), 0, 4, "misaligned"),                           # a pitch off by 8 bytes
    ((2, 136, 9, 1, 2, 38, 4, 76), 0, 64, "not"),                                  # aligned, but the other part's row
])
def test_the_check_sees_a_bad_band_or_pitch(exe, shape, bw, shift, what):
    """The plan is clean; with a band width the plan would not choose, or every read address
    shifted as a wrong pitch would shift it, the program reports violations."""
    assert _one(exe, *shape)["violations"] == []
    bad = _one(exe, *shape, bw, shift)["violations"]
    assert bad and any(what in v["detail"] for v in bad), bad


# ---------------------------------------------------------------------------- the f32 plan
def test_f32_plan_bands_slices_and_floats_over_the_sweep(exe):
    r = _one(exe, "f32")
    assert r["violations"] == 0 and r["first"] == [], r["first"]
    # stride 1: Ws 1..400 x two (B, Hs); stride 2 (three tilings): the same plus the two crops
    assert r["grids"] == 400 * 2 + 3 * (400 * 2 + 400 + 397)
    assert (r["band_max"], r["target_wgs"], r["bias_slices_max"]) == (bc.GW_BW, bc.GW_TARGET, bc.GW_MAX_BIAS)


@pytest.mark.parametrize("cid", [c["id"] for c in bc.GW_CASES])
def test_f32_plan_is_the_mirrors_and_the_workspace_query(exe, cid):
    c = bc.GW_BY_ID[cid]
    shape = (c["stride"], c["Cs"], c["c0"] + c["c1"], c["B"], c["Hs"], c["Ws"], c["Hl"], c["Wl"])
    a, m = _one(exe, "f32", *shape), bc.gw_plan(*shape)
    assert a == _one(exe, "f32", *shape)
    assert "".join(str(a[k]) for k in ("S", "wm", "wgm", "wgn")) == m["tiling"]
    for k in ("mtiles", "ntiles", "nbands", "bw", "units", "ups", "nsl", "nsb", "floats"):
        assert a[k] == m[k], (k, a, m)
    assert (a["mt"], a["nt"], a["nthr"]) == (16 * a["wm"] * a["wgm"], 16 * a["wgn"], 64 * a["wgm"] * a["wgn"])
    assert a["slab"] == a["mtiles"] * a["mt"] * a["ntiles"] * a["nt"] * 9 and a["bias_off"] == a["slab"] * a["nsl"]
    assert a["floats"] == a["slab"] * a["nsl"] + a["nsb"] * max(shape[1], shape[2])
    assert _lib.get().nlspn_gconv_wgrad_workspace_bytes(*shape) == 4 * a["floats"]


@pytest.mark.parametrize("shape", SHAPES)
def test_bf16_plan_takes_the_f32_plans_bias_slices(exe, shape):
    assert _one(exe, *shape)["nsb"] == _one(exe, "f32", *shape)["nsb"]
