"""CPU: the split-bf16 data gradients of the GRU-mode convolutions (nlspn_gconv_x3_dgrad, the
NLSPN_GCX3_DG_* presets) without a device.

  * the split's own error: on every element of every case of tests/_gconv_x3_dgrad_cases.py the
    emulation of the three split products is within 2^-15 X of the float64 reference on the
    unsplit operands (the contract of include/nlspn_prop.h), and the emulation is not the
    reference (the bound is not vacuous);
  * every case's claimed edge is true of gc_tile, the launcher's own function, asked through
    tests/gconv_x3_dg_plan_check.cpp;
  * that program's cell-by-cell staging and fragment check (tests/gconv_x3_plan_check.cpp's code)
    over NLSPN_GCX3_DG_CONFIGS x heights {1, 2, 3, 7, 17, 29} x widths 1..400: no violation;
  * the new translation unit's kernels use no scratch (the compiler's kernel-resource-usage
    remarks: the code object's metadata values);
  * the entry points validate before any device call, `covers` answers for exactly the shapes
    the entry serves, the adjoint packers hold the adjoint tensors of pack_adjoint /
    pack_adjoint_s1, and the switches refuse bad values.
"""
import ctypes
import json
import os
import shutil
import subprocess
import sys

import pytest
import torch
import torch.nn as nn

import _gconv_bwd_cases as bc
import _gconv_x3_dgrad_cases as xc
from nlspn_eccv20_amd import _lib
from nlspn_eccv20_amd import gru as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nlspn_eccv20_amd", "csrc")
P = ctypes.c_void_p(64)  # never dereferenced: validation fails first
IDS = [c["id"] for c in xc.CASES]
HEIGHTS = [1, 2, 3, 7, 17, 29]


# ------------------------------------------------------------------ the split's error
@pytest.mark.parametrize("cid", IDS)
def test_emulation_is_within_the_split_bound_of_the_unsplit_reference(cid):
    R = xc.reference(cid)
    err = (R["emu"] - R["ref"]).abs()
    assert bool((err <= xc.SPLIT_BOUND * R["X"]).all()), float((err / (R["X"] + 1e-300)).max())
    assert float(err.max()) > 0  # (the split moves the value: the emulation is its own reference)


def test_the_table_holds_the_cases_the_presets_need():
    by = {p: [c for c in xc.CASES if c["preset"] == p] for p in xc.PRESETS}
    for p, cases in by.items():
        e = set().union(*(c["edges"] for c in cases))
        assert {"full_band", "band_plus_one", "npx_shrunk"} <= e, (p, e)
        assert any(c["cg"] % 16 for c in cases) and any(c["cout"] % xc.CO_TILE[p] for c in cases), p
    for p in (xc.DG_T2, xc.DG_S2):
        e = set().union(*(c["edges"] for c in by[p]))
        assert {"uneven_last_band", "empty_tile"} <= e, (p, e)
        assert any(c["dxs"] for c in by[p])
    for p in (xc.DG_T2, xc.DG_T2_C16):
        assert {(2 * c["Hg"] - c["Ho"], 2 * c["Wg"] - c["Wo"]) for c in by[p]} >= {(0, 1), (1, 0), (1, 1)}
    for p in (xc.DG_T2, xc.DG_T2_C16, xc.DG_S2):
        assert {(c["act"], c["add"]) for c in by[p] if c["scale"] == 0.25} >= {
            (a, d) for a in (bc.ACT_RELU, bc.ACT_TANH) for d in ("none", "sep")}
    assert {(c["cg"], c["cout"], c["split"], c["add"]) for c in xc.GRU} == {(128, 256, 128, "none"), (256, 256, 128, "alias")}


# ------------------------------------------------------------------ the planner
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    path = str(tmp_path_factory.mktemp("gconv_x3_dg_plan") / "gconv_x3_dg_plan_check")
    out = subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-I", CSRC, "-I", os.path.join(ROOT, "tests"),
                          os.path.join(ROOT, "tests", "gconv_x3_dg_plan_check.cpp"), "-o", path], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    return path


def _run(exe, *args):
    run = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, env={})
    assert run.returncode == 0, run.stderr[-2000:]
    return json.loads(run.stdout)


@pytest.mark.parametrize("cid", IDS)
def test_case_hits_its_claimed_edge(exe, cid):
    c = xc.BY_ID[cid]
    t = _run(exe, "tile", c["preset"], c["gh"], c["gw"])
    assert t["ok"] == 1 and t["bwmax"] == xc.BWMAX[c["preset"]] and t["wgco"] == xc.CO_TILE[c["preset"]], t
    assert c["edges"] <= xc.edges_of(c, t), (c["edges"], xc.edges_of(c, t), t)
    # the Python mirror the f32 cases use agrees with the launcher's function on this grid
    m = bc.gc_tiling(c["mode"], t["npx_full"], {80: 6, 81: 6, 82: 12, 83: 6}[c["preset"]], xc.XP[c["preset"]], c["gh"], c["gw"])
    assert {k: m[k] for k in ("nbands", "bw", "bwl", "npx", "tpb")} == {k: t[k] for k in ("nbands", "bw", "bwl", "npx", "tpb")}
    assert bool(m["empty_last"]) == bool(t["empty_last"])


def test_every_fragment_read_of_the_dgrad_presets_is_a_staged_cell(exe):
    report = _run(exe)
    assert [p["id"] for p in report["presets"]] == list(xc.PRESETS)
    assert report["grids"] == len(xc.PRESETS) * len(HEIGHTS) * 400
    assert report["violations"] == 0 and report["first"] == [] and report["refused"] == 0, report["first"]
    pixels = sum(gh * gw for gh in HEIGHTS for gw in range(1, 401))
    assert report["reads"] == pixels * (9 * 2 + 4 * 2) * 4   # a stride-1, a stride-2 and two transposed presets
    assert report["staged"] > 0 and report["gru1_maps"] == 0
    for p in report["presets"]:
        assert 0 < p["lds"] <= report["lds_budget"] == 160 * 1024 and p["chunk_channels"] == 16, p
    # each takes the tiling, hence the LDS bytes, of the forward preset of its adjoint kind
    lds = {p["id"]: p["lds"] for p in report["presets"]}
    assert lds[80] == 2 * (4 * 4 * 64 + 1024) * 16 and lds[81] == 2 * (256 + 2048) * 16
    assert lds[82] == 2 * (4 * 9 * 64 + 2048) * 16 and lds[83] == 2 * (4 * 9 * 64 + 1024) * 16


def test_the_check_sees_a_forced_band_width_and_a_shifted_pitch(exe):
    for pid, gh, gw, bw in ((80, 17, 100, 60), (81, 27, 200, 120), (82, 14, 100, 60), (83, 17, 100, 60)):
        assert _run(exe, pid, gh, gw) == []
        wide = _run(exe, pid, gh, gw, bw)
        assert wide and all("window" in v["detail"] for v in wide), wide
        off = _run(exe, pid, gh, gw, 0, 1)
        assert off and all("is not that input cell" in v["detail"] for v in off), off


# ------------------------------------------------------------------ the code objects
def test_dgrad_unit_compiles_without_scratch(tmp_path):
    sys.path.insert(0, CSRC)
    import resource_usage as RU
    path = os.path.join(RU.BUILD_DIR, "nlspn_kern_gconv_x3_dg.ru.txt")
    if os.path.exists(path):
        rows = RU.parse(open(path).read())
    else:
        out = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
                              "-ffp-contract=off", "-Rpass-analysis=kernel-resource-usage", "-c", "-o",
                              str(tmp_path / "gx3dg.o"), os.path.join(CSRC, "nlspn_kern_gconv_x3_dg.hip")],
                             capture_output=True, text=True, cwd=CSRC)
        assert out.returncode == 0, out.stderr[-2000:]
        rows = RU.parse(out.stderr)
    # the four data-gradient presets and the f32 -> c8x2 kernel
    assert len(rows) == 5 and sum("gconvx3_kernel" in n for n in rows) == 4 and sum("gcx3_split_kernel" in n for n in rows) == 1, sorted(rows)
    bad = {n: (r.get("ScratchSize"), r.get("VGPRs Spill")) for n, r in rows.items()
           if r.get("ScratchSize", 0) != 0 or r.get("VGPRs Spill", 0) != 0}
    assert not bad, bad


# ------------------------------------------------------------------ validation before any device call
def _err(rc):
    return rc, _lib.get().nlspn_last_error().decode()


def _dgrad(**over):
    a = dict(layer=G.GCX3_DG_S1, gs=P, cg=128, wpk=P, ysave=None, add0=None, add1=None, dx0=P, dx1=P, split=128, dxs=None,
             B=1, Hg=8, Wg=8, cout=256, Ho=8, Wo=8, act=0, scale=1.0, stream=None)
    a.update(over)
    return _err(_lib.get().nlspn_gconv_x3_dgrad(*a.values()))


ONE = dict(dx1=None, split=256)  # one output tensor


@pytest.mark.parametrize("over,code,msg", [
    (dict(gs=None), _lib.EINVAL, "null"),
    (dict(dx0=None), _lib.EINVAL, "null"),
    (dict(layer=G.GCX3_S2), _lib.EINVAL, "not a split-bf16 data-gradient preset"),    # a forward x3 preset
    (dict(layer=G.GCX3_GRU2), _lib.EINVAL, "not a split-bf16 data-gradient preset"),
    (dict(layer=G.GC_DG_S1), _lib.EINVAL, "not a split-bf16 data-gradient preset"),   # an f32 data-gradient preset
    (dict(layer=G.GC_DG_T2), _lib.EINVAL, "not a split-bf16 data-gradient preset"),
    (dict(split=300), _lib.EINVAL, "cout mismatch"),
    (dict(dx1=None), _lib.EINVAL, "cout mismatch"),
    (dict(add1=P, **ONE), _lib.EINVAL, "cout mismatch"),
    (dict(dxs=P), _lib.EINVAL, "split copy needs one output"),                         # dxs with two outputs
    (dict(act=1, ysave=None, **ONE), _lib.EINVAL, "needs the saved output"),           # an activation without ysave
    (dict(act=1, ysave=P), _lib.EINVAL, "needs the saved output"),                     # ... with two outputs
    (dict(act=3, ysave=P, **ONE), _lib.EINVAL, "activation 3"),
    (dict(Ho=9), _lib.EINVAL, "does not belong"),
    (dict(layer=G.GCX3_DG_T2, Ho=14, Wo=16, **ONE), _lib.EINVAL, "does not belong"),
    (dict(layer=G.GCX3_DG_S2, Hg=17, Wg=16, **ONE), _lib.EINVAL, "does not belong"),
    (dict(layer=G.GCX3_DG_S2, Hg=15, Wg=16, **ONE), _lib.EUNSUPPORTED, "stored cropped"),  # a cropped stride-2-mode gradient
    (dict(layer=G.GCX3_DG_S2, Hg=16, Wg=13, **ONE), _lib.EUNSUPPORTED, "stored cropped"),
    (dict(layer=G.GCX3_DG_S2, Hg=16, Wg=16, cg=8, cout=16, dx1=None, split=16), _lib.EUNSUPPORTED, "at most 16 channels"),  # both <= 16
    (dict(layer=G.GCX3_DG_S2, Hg=16, Wg=16, cg=16, **ONE), _lib.EUNSUPPORTED, "at most 16 channels"),
    (dict(B=0), _lib.EINVAL, "bad shape"),
])
def test_dgrad_entry_validates_first(over, code, msg):
    rc, err = _dgrad(**over)
    assert rc == code and msg in err, (rc, err)


def test_the_other_entries_refuse_the_new_presets():
    lib = _lib.get()
    for layer in xc.PRESETS:
        rc, err = _err(lib.nlspn_gconv_x3(layer, P, 64, None, 0, P, P, P, None, None, None, None, None, None, None, 1, 8, 8,
                                          64, 8, 8, 0, 1.0, 0, None))
        assert rc == _lib.EINVAL and "not a split-bf16 preset" in err, (rc, err)
        rc, err = _err(lib.nlspn_gconv_dgrad(layer, P, 64, P, None, None, None, P, None, 64, 1, 8, 8, 64, 8, 8, 0, 1.0, None))
        assert rc == _lib.EINVAL and "not a data-gradient preset" in err, (rc, err)
        co, cc, tr = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        assert lib.nlspn_gconv_x3_pack_layout(layer, ctypes.byref(co), ctypes.byref(cc), ctypes.byref(tr)) == _lib.EINVAL
        assert lib.nlspn_gconv_x3_dgrad_pack_layout(layer, ctypes.byref(co), ctypes.byref(cc), ctypes.byref(tr)) == 0
        assert (co.value, cc.value, tr.value) == (xc.CO_TILE[layer], 16, int(xc.MODE[layer] == bc.T2))
    assert lib.nlspn_gconv_x3_dgrad_pack_layout(G.GCX3_S2, None, None, None) == _lib.EINVAL


def test_split_entry_validates_first():
    lib = _lib.get()
    for args, msg in (((None, P, 1, 8, 4, 4), "null"), ((P, None, 1, 8, 4, 4), "null"), ((P, P, 0, 8, 4, 4), "bad shape"),
                      ((P, P, 1, 0, 4, 4), "bad shape")):
        rc, err = _err(lib.nlspn_gconv_x3_split(*args, None))
        assert rc == _lib.EINVAL and msg in err, (rc, err)


def test_covers_answers_for_exactly_what_the_entry_serves():
    cov = _lib.get().nlspn_gconv_x3_dgrad_covers
    # the section's data gradients at hc = 128 (NYU 228 x 304: 114 x 152, 57 x 76, 29 x 38)
    assert cov(G.GCX3_DG_S1, 128, 256, 29, 38, 29, 38) == 1 and cov(G.GCX3_DG_S1, 256, 256, 29, 38, 29, 38) == 1
    assert cov(G.GCX3_DG_T2, 128, 256, 29, 38, 57, 76) == 1       # of the 2hc -> hc encoder conv (57 = 2 * 29 - 1)
    assert cov(G.GCX3_DG_T2_C16, 256, 16, 57, 76, 114, 152) == 1  # of the 16 -> 2hc encoder conv
    assert cov(G.GCX3_DG_S2, 256, 128, 58, 76, 29, 38) == 1       # of the hc -> 2hc decoder layer
    # not served: the 2hc -> 16 decoder layer's (a 16-channel gradient: measured slower than the f32
    # entry), the f32 last decoder layer's cropped gradient, both channel counts <= 16
    assert cov(G.GCX3_DG_S2, 16, 256, 116, 152, 58, 76) == 0 and cov(G.GCX3_DG_S2, 17, 256, 116, 152, 58, 76) == 1
    assert cov(G.GCX3_DG_S2, 8, 16, 228, 304, 116, 152) == 0 and cov(G.GCX3_DG_S2, 64, 64, 15, 16, 8, 8) == 0
    assert cov(G.GCX3_DG_T2_C16, 16, 9, 114, 152, 228, 304) == 0 and cov(G.GCX3_DG_S2, 8, 16, 16, 16, 8, 8) == 0
    # sizes that belong to no gradient, and anything that is not a NLSPN_GCX3_DG_* preset
    assert cov(G.GCX3_DG_S1, 128, 256, 8, 8, 9, 8) == 0 and cov(G.GCX3_DG_T2, 64, 64, 8, 8, 14, 16) == 0
    assert cov(G.GCX3_S2, 64, 64, 16, 16, 8, 8) == 0 and cov(G.GC_DG_S2, 64, 64, 16, 16, 8, 8) == 0
    assert cov(G.GCX3_DG_S1, 0, 256, 8, 8, 8, 8) == 0
    for c in xc.CASES:  # every case of the per-element table is served
        assert cov(c["preset"], c["cg"], c["cout"], c["Hg"], c["Wg"], c["Ho"], c["Wo"]) == 1, c["id"]


# ------------------------------------------------------------------ packers and switches
def test_adjoint_packers_hold_the_adjoint_tensors_split():
    gen = torch.Generator().manual_seed(3)
    conv = nn.Conv2d(16, 40, 3, 2, 1)      # its adjoint: the transposed conv 40 -> 16 of the same tensor
    wide = nn.Conv2d(40, 24, 3, 2, 1)
    convt = nn.ConvTranspose2d(24, 40, 3, 2, 1, 1)
    with torch.no_grad():
        for m in (conv, wide, convt):
            m.weight.copy_(torch.randn(m.weight.shape, generator=gen))
    dg, w = G.pack_adjoint_x3(conv)
    assert dg == G.GCX3_DG_T2_C16 and w.dtype == torch.bfloat16
    hi, lo = G.split_bf16(conv.weight.detach())
    assert torch.equal(G.unpack_convt_x3(w, 40, 16, dg), hi.float() + lo.float())
    dg, w = G.pack_adjoint_x3(wide)
    assert dg == G.GCX3_DG_T2
    hi, lo = G.split_bf16(wide.weight.detach())
    assert torch.equal(G.unpack_convt_x3(w, 24, 40, dg), hi.float() + lo.float())
    dg, w = G.pack_adjoint_x3(convt)       # the conv reading (Cin, Cout, 3, 3) as (out, in)
    assert dg == G.GCX3_DG_S2
    hi, lo = G.split_bf16(convt.weight.detach())
    assert torch.equal(G.unpack_conv_x3(w, 24, 40, dg), hi.float() + lo.float())
    ws1 = torch.randn((24, 40, 3, 3), generator=gen)
    adj = ws1.transpose(0, 1).flip(2, 3)
    hi, lo = G.split_bf16(adj)
    assert torch.equal(G.unpack_conv_x3(G.pack_adjoint_s1_x3(ws1), 40, 24, G.GCX3_DG_S1), hi.float() + lo.float())
    # the same adjoint tensors as the f32 packers' (those hold them unsplit)
    assert torch.equal(G.unpack_conv(G.pack_adjoint_s1(ws1), 40, 24, G.GC_DG_S1), adj)


def test_switches_refuse_bad_values():
    gc = G.GruConvs()
    assert gc.dgrad_precision == "fp32" and gc.stats["dgrad_x3"] == 0
    assert gc._dgrad_x3() is False
    gc.dgrad_precision = "bf16x3"
    assert gc._dgrad_x3() is True
    gc.dgrad_precision = "bf16"
    with pytest.raises(ValueError, match="dgrad_precision"):
        gc._dgrad_x3()
