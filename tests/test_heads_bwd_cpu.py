"""CPU: the head epilogue's backward (include/nlspn_prop.h: nlspn_head_backward_pre,
nlspn_head_dgrad_single, nlspn_head_wgrad_workspace_bytes, nlspn_head_wgrad;
csrc/nlspn_heads_bwd.h, csrc/nlspn_heads_bwd_plan.h).

 1. The float64 references of tests/_heads_bwd_cases.py (explicit sums for gpre, the four data
    gradients, dW and db) equal torch's double autograd of the reference's op sequence
    (torch.cat, F.conv2d, ReLU, sigmoid) to 1e-12 relative on every case.
 2. The new symbols are in the header, in _lib.SIGNATURES and in _lib.AB_OPTIONAL; the ABI
    version stays 3.
 3. Every refusal is reached with arguments alone (dummy pointers; only where no GPU is
    visible, as tests/test_capi_guards_cpu.py), and the workspace query answers 0 on a refused
    shape.
 4. tests/heads_bwd_plan_check.cpp (host only, built here) sweeps shapes over the plan header:
    units and slices partition the (image, row, band) space in order, the workspace regions are
    the plan's, LDS within 160 KB, the plan a function of the shape alone; the Python mirror of
    the cases file and the library's workspace query agree with it.
 5. The new translation unit's resource-usage remarks show no scratch in any new kernel.
"""
import ctypes
import json
import os
import shutil
import subprocess
import sys

import pytest
import torch

import _heads_bwd_cases as hc
from nlspn_eccv20_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nlspn_eccv20_amd", "csrc")
P = ctypes.c_void_p(64)  # never dereferenced: validation fails first
NEW = ("nlspn_head_backward_pre", "nlspn_head_dgrad_single", "nlspn_head_wgrad_workspace_bytes", "nlspn_head_wgrad")


# ------------------------------------------------------------------ 1. the references
def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-300))


@pytest.mark.parametrize("cid", hc.IDS)
def test_reference_is_torch_double_autograd(cid):
    c, o = hc.BY_ID[cid], hc.operands(cid)
    B, C, H, W, nout = c["B"], c["C"], c["H"], c["W"], c["nout"]
    ar = hc.autograd_reference(o, nout)
    gpre = hc.gpre_reference(o["g_oa"], o["g_pi"], o["g_cf"], ar["pred_init"], ar["conf"], B, H, W, nout)
    dg = hc.dgrad_reference(gpre, o["w_oa"], o["w_id"], o["w_cf"], C)
    wg = hc.wgrad_reference(gpre, o["fe1"], o["fd_oa"], o["fd_id"], o["fd_cf"], hc.plan_of(c))
    pairs = [("d_fe1", "fe1"), ("d_fd_oa", "fd_oa"), ("d_fd_id", "fd_id"), ("d_fd_cf", "fd_cf"), ("dw_oa", "w_oa"),
             ("dw_id", "w_id"), ("dw_cf", "w_cf")]
    seen = 0
    for ours, theirs in pairs:
        ref = (dg if ours.startswith("d_") else wg).get(ours)
        if ref is None:
            assert o[theirs] is None
            continue
        want = ar["grads"][theirs]
        if want is None:  # (the head's output had no incoming gradient: autograd reports "unused")
            assert c.get("no_g_conf") and not bool(ref[0].any())
            continue
        assert _rel(ref[0], want) <= 1e-12, (ours, _rel(ref[0], want))
        assert bool((ref[1] >= ref[0].abs() * (1 - 1e-12)).all())  # X bounds the value: the sum of |terms|
        seen += 1
    assert seen >= 4
    # db against the sum of the pre-activation gradient autograd implies (zero biases: d/db = sum gpre)
    assert _rel(wg["db_oa"][0], o["g_oa"].double().sum((0, 2, 3))) <= 1e-12


def test_gpre_reference_is_a_select_and_keeps_zero_rows():
    o = hc.operands("no-g-conf-2x16x40x64-24")
    gp = hc.gpre_reference(o["g_oa"], o["g_pi"], None, o["pred_init"], None, 2, 40, 64, 24)
    assert not bool(gp[:, 25].any()) and bool(gp[:, 24].any())
    pi = o["pred_init"].view(-1)
    assert float(pi[0]) == 0 and float(pi[1]) == 0 and float(pi[2]) > 0  # exact zero, -0.0, the smallest normal
    assert [float(v) for v in gp[0, 24].view(-1)[:2]] == [0.0, 0.0] and float(gp[0, 24].view(-1)[2]) == float(o["g_pi"].view(-1)[2])
    cf = hc.operands("base-2x64x40x64-24")["conf"]
    assert float(cf.min()) > 0 and float(cf.max()) < 1 and float(cf.min()) <= 2.0 ** -20 and float(cf.max()) >= 1 - 2.0 ** -20


# ------------------------------------------------------------------ 2. the ABI
def test_new_symbols_are_declared_bound_and_optional():
    lib = _lib.get()
    declared = _lib.header_symbols()
    for s in NEW:
        assert s in declared and s in _lib.SIGNATURES and s in _lib.AB_OPTIONAL and hasattr(lib, s), s
    assert lib.nlspn_abi_version() == 3


# ------------------------------------------------------------------ 3. refusals
def _err(rc):
    return rc, _lib.get().nlspn_last_error().decode()


def _pre(**over):
    a = dict(g_oa=P, g_pi=P, g_cf=P, pred_init=P, conf=P, gpre=P, B=1, H=8, W=8, nout=24, stream=None)
    a.update(over)
    return _err(_lib.get().nlspn_head_backward_pre(*a.values()))


def _single(**over):
    a = dict(gpre=P, w_id=P, w_cf=P, d_id=P, d_cf=P, B=1, C=16, H=8, W=8, nout=24, stream=None)
    a.update(over)
    return _err(_lib.get().nlspn_head_dgrad_single(*a.values()))


def _wgrad(**over):
    a = dict(gpre=P, fe1=P, fd_oa=P, fd_id=P, fd_cf=P, dw_oa=P, db_oa=P, dw_id=P, db_id=P, dw_cf=P, db_cf=P, ws=P,
             ws_bytes=1 << 62, B=1, C=16, H=8, W=8, nout=24, stream=None)
    a.update(over)
    return _err(_lib.get().nlspn_head_wgrad(*a.values()))


G = 1 << 14
REFUSALS = [
    (_pre, dict(gpre=None), _lib.EINVAL, "null pointer"),
    (_pre, dict(pred_init=None), _lib.EINVAL, "both be given or both NULL"),
    (_pre, dict(g_cf=None), _lib.EINVAL, "both be given or both NULL"),
    (_pre, dict(nout=0), _lib.EINVAL, "nout=0"),
    (_pre, dict(nout=159), _lib.EUNSUPPORTED, "at most 158"),
    (_pre, dict(W=0), _lib.EINVAL, "empty input"),
    (_pre, dict(H=G, W=G), _lib.EINVAL, "input too large"),             # 26 planes of 2^28 pixels
    (_pre, dict(B=1 << 20, H=64, W=64), _lib.EINVAL, "input too large"),  # B H W = 2^32
    (_single, dict(gpre=None), _lib.EINVAL, "null pointer"),
    (_single, dict(d_id=None), _lib.EINVAL, "both be given or both NULL"),
    (_single, dict(w_cf=None), _lib.EINVAL, "both be given or both NULL"),
    (_single, dict(C=24), _lib.EINVAL, "multiple of 16"),
    (_single, dict(C=0), _lib.EINVAL, "multiple of 16"),
    (_single, dict(nout=159), _lib.EUNSUPPORTED, "at most 158"),
    (_single, dict(B=0), _lib.EINVAL, "empty input"),
    (_single, dict(C=64, H=4096, W=4096), _lib.EINVAL, "input too large"),  # 64 planes of 2^24 pixels: 2^32 bytes
    (_wgrad, dict(gpre=None), _lib.EINVAL, "null pointer"),
    (_wgrad, dict(fe1=None), _lib.EINVAL, "null pointer"),
    (_wgrad, dict(db_oa=None), _lib.EINVAL, "null pointer"),
    (_wgrad, dict(ws=None), _lib.EINVAL, "null pointer"),
    (_wgrad, dict(fd_id=None), _lib.EINVAL, "all be given or all NULL"),
    (_wgrad, dict(db_cf=None), _lib.EINVAL, "all be given or all NULL"),
    (_wgrad, dict(C=40), _lib.EINVAL, "multiple of 16"),
    (_wgrad, dict(nout=0), _lib.EINVAL, "nout=0"),
    (_wgrad, dict(nout=159), _lib.EUNSUPPORTED, "at most 158"),
    (_wgrad, dict(H=0), _lib.EINVAL, "empty input"),
    (_wgrad, dict(ws_bytes=1024), _lib.EINVAL, "workspace too small"),
    (_wgrad, dict(C=64, H=4096, W=4096), _lib.EINVAL, "input too large"),
    (_wgrad, dict(B=1 << 30, H=2, W=1), _lib.EINVAL, "input too large"),   # 2^31 units
]


@pytest.mark.parametrize("fn,over,code,msg", REFUSALS)
def test_entries_refuse_before_any_device_call(fn, over, code, msg):
    rc, text = fn(**over)
    # (the size rule is the forward's check, in its wording; the others name the backward)
    assert rc == code and msg in text and (text.startswith("head backward") or msg == "empty input"), (rc, text)


def test_refusal_order_is_the_documented_one():
    """null pointers, C, nout, sizes, workspace, too large: two faults give the earlier message."""
    assert "null pointer" in _wgrad(gpre=None, C=24)[1]
    assert "multiple of 16" in _wgrad(C=24, nout=0)[1]
    assert "nout=0" in _wgrad(nout=0, B=0)[1]
    assert "empty input" in _wgrad(B=0, ws_bytes=0)[1]
    assert "workspace too small" in _wgrad(C=64, H=4096, W=4096, ws_bytes=1024)[1]


@pytest.mark.skipif(torch.cuda.is_available(), reason="a call past every guard is made on dummy pointers: no GPU may be visible")
def test_a_good_call_passes_every_guard():
    lib = _lib.get()
    need = lib.nlspn_head_wgrad_workspace_bytes(1, 16, 8, 8, 24)
    for fn, over in ((_pre, {}), (_single, {}), (_wgrad, dict(ws_bytes=need)), (_wgrad, dict(ws_bytes=need, fd_cf=None, dw_cf=None, db_cf=None))):
        rc, text = fn(**over)
        assert rc == _lib.EHIP and "head backward" not in text, (rc, text)  # the launch finds no device
    assert _wgrad(ws_bytes=need - 1)[0] == _lib.EINVAL


def test_workspace_query_is_zero_on_a_refused_shape():
    q = _lib.get().nlspn_head_wgrad_workspace_bytes
    assert q(1, 16, 8, 8, 24) > 0
    for bad in ((0, 16, 8, 8, 24), (1, 24, 8, 8, 24), (1, 16, 8, 8, 0), (1, 16, 8, 8, 159), (1, 16, 0, 8, 24),
                (1, 64, 4096, 4096, 24), (1 << 30, 16, 2, 1, 24)):
        assert q(*bad) == 0, bad


# ------------------------------------------------------------------ 4. the plan
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    path = str(tmp_path_factory.mktemp("heads_bwd_plan") / "heads_bwd_plan_check")
    out = subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-I", CSRC, os.path.join(ROOT, "tests", "heads_bwd_plan_check.cpp"),
                          "-o", path], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    return path


def test_plan_sweep(exe):
    run = subprocess.run([exe], capture_output=True, text=True, env={})
    r = json.loads(run.stdout)
    assert r["violations"] == 0 and r["first"] == [] and run.returncode == 0, r["first"]
    assert r["grids"] == 4 * 330 * 4 * 9 + 17 * 9 and r["units"] > r["grids"]
    assert 0 < r["lds"] <= r["lds_budget"] == 160 * 1024
    assert (r["target_wgs"], r["band_max"]) == (hc.TARGET, hc.BW)


@pytest.mark.parametrize("cid", hc.IDS + ["nyu", "kitti"])
def test_plan_is_the_mirrors_and_the_workspace_query(exe, cid):
    shape = {"nyu": (8, 64, 228, 304, 24), "kitti": (4, 64, 240, 1216, 24)}.get(cid) or \
        tuple(hc.BY_ID[cid][k] for k in ("B", "C", "H", "W", "nout"))
    one = lambda: json.loads(subprocess.run([exe] + [str(v) for v in shape], capture_output=True, text=True, env={}).stdout)  # noqa: E731
    a, m = one(), hc.hb_plan(*shape)
    assert a == one() and a["fits"] == 1
    for k, v in m.items():
        assert a[k] == v, (k, a, m)
    assert _lib.get().nlspn_head_wgrad_workspace_bytes(*shape) == 4 * a["floats"]
    if cid == "nyu":  # one row tile x two channel tiles: 254 K slices of 36 units, one slab 32 x 128 x 9 floats
        assert (a["mtiles"], a["ntiles"], a["nbands"], a["bw"], a["nsl"], a["nvs"], a["nsb"]) == (1, 2, 5, 61, 254, 34, 34)


# ------------------------------------------------------------------ 5. no scratch
NEW_KERNELS = ("head_pre_kernel", "head_dgrad_single_kernel", "hwgrad_kernel", "hwgrad_single_kernel")


def test_backward_unit_compiles_without_scratch(tmp_path):
    sys.path.insert(0, CSRC)
    import resource_usage as RU
    path = os.path.join(RU.BUILD_DIR, "nlspn_kern_heads_bwd.ru.txt")
    if os.path.exists(path):
        rows = RU.parse(open(path).read())
    else:
        out = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
                              "-ffp-contract=off", "-Rpass-analysis=kernel-resource-usage", "-c", "-o",
                              str(tmp_path / "hb.o"), os.path.join(CSRC, "nlspn_kern_heads_bwd.hip")],
                             capture_output=True, text=True, cwd=CSRC)
        assert out.returncode == 0, out.stderr[-2000:]
        rows = RU.parse(out.stderr)
    assert len(rows) == len(NEW_KERNELS), sorted(rows)
    for k in NEW_KERNELS:
        assert any(k in n for n in rows), k
    bad = {n: (r.get("ScratchSize"), r.get("VGPRs Spill")) for n, r in rows.items()
           if r.get("ScratchSize", 0) != 0 or r.get("VGPRs Spill", 0) != 0}
    assert not bad, bad
    # the matrix-core kernel keeps two waves per SIMD (at most 256 registers a lane)
    hw = next(r for n, r in rows.items() if "hwgrad_kernel" in n)
    assert hw.get("VGPRs", 0) + hw.get("AGPRs", 0) <= 256, hw
