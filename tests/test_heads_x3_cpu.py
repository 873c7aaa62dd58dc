"""CPU: the split-bf16 head epilogue (csrc/nlspn_heads_x3.h) off the device: the LDS addressing
check (a host program over nlspn_heads_x3_plan.h, once more under the address and UB
sanitizers), the packed layout's round trip, every refusal of the new entry points before a
device call, the unit's resource remarks (no scratch), the model's head_precision switch, and the
emulation the GPU test (tests/test_gpu_heads_x3.py) is held against.

The emulation is the contract in float64: conv(w_hi, x_hi) + conv(w_hi, x_lo) + conv(w_lo, x_hi)
with (hi, lo) = split_bf16 of the f32 operands.  Measured here with torch.rand inputs and default
nn.Conv2d init, as max |emu - unsplit| / sum |w||x|:
    C = 64 / nout 24: 7.0e-7      C = 16 / nout 144: 1.54e-6        (bar: 2^-15 = 3.05e-5)
    without w_hi x_lo: 2.7e-4 / 6.1e-4    without w_lo x_hi: 2.3e-4 / 6.0e-4
    hi and lo of the activation swapped: 2.3e-4 / 6.0e-4
so the GPU test's bar of 2e-6 against the emulation tells a kernel that drops or swaps a part
from a right one by two orders of magnitude.
"""
import ctypes
import os
import subprocess
import sys
import types

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from nlspn_eccv20_amd import NLSPNModel, _lib
from nlspn_eccv20_amd import heads as HD
from nlspn_eccv20_amd.gru import split_bf16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nlspn_eccv20_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "heads_x3_plan_check.cpp")
P = ctypes.c_void_p(64)  # never dereferenced: validation fails first


# ------------------------------------------------------------------ the addressing check
def _build_check(tmp_path, name, *flags):
    exe = str(tmp_path / name)
    out = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I", CSRC, *flags, "-o", exe, SRC],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    return exe


def test_plan_check_walks_every_fragment_read(tmp_path):
    out = subprocess.run([_build_check(tmp_path, "check")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:]
    assert "violations 0" in out.stdout and "tiles 4608" in out.stdout  # 4 MB x 5 H x 80 W, every tile


def test_plan_check_sees_a_shifted_pitch(tmp_path):
    out = subprocess.run([_build_check(tmp_path, "shifted", "-DNLSPN_HX3_PITCH=35")], capture_output=True, text=True)
    assert out.returncode == 1 and "B read holds another element" in out.stdout
    assert "violations 0" not in out.stdout


def test_plan_check_under_sanitizers(tmp_path):
    """The same stand-alone host program with -fsanitize=address,undefined (nothing is loaded
    into python)."""
    exe = _build_check(tmp_path, "san", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, (out.stdout[-1000:], out.stderr[-3000:])
    assert "violations 0" in out.stdout and not out.stderr.strip()


# ------------------------------------------------------------------ the packed layout
def _convs(C, nout, seed=0, with_id=True, with_cf=True):
    torch.manual_seed(seed)
    oa = nn.Conv2d(2 * C, nout, 3, padding=1)
    idc = nn.Conv2d(2 * C, 1, 3, padding=1) if with_id else None
    cfc = nn.Conv2d(2 * C, 1, 3, padding=1) if with_cf else None
    return oa, idc, cfc


@pytest.mark.parametrize("C,nout,with_id,with_cf", [(64, 24, True, True), (16, 144, True, True), (32, 48, False, True),
                                                    (16, 8, True, False), (16, 62, True, True)])
def test_pack_reference_round_trip(C, nout, with_id, with_cf):
    oa, idc, cfc = _convs(C, nout, C + nout, with_id, with_cf)
    wm = HD.pack_wm_x3_reference(oa, idc, cfc)
    lib = _lib.get()
    nm, nv, nb = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    assert lib.nlspn_head_x3_packed_size(C, nout, ctypes.byref(nm), ctypes.byref(nv), ctypes.byref(nb)) == 0
    fm, fv, fb = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    assert lib.nlspn_head_packed_size(C, nout, ctypes.byref(fm), ctypes.byref(fv), ctypes.byref(fb)) == 0
    mb = HD._mb(nout)
    assert wm.dtype == torch.bfloat16 and wm.numel() == nm.value == 2 * fm.value == 2 * C * 9 * 32 * mb * 2
    assert (nv.value, nb.value) == (fv.value, fb.value) == (2 * C * 9, 32 * mb)
    hi, lo = HD.unpack_wm_x3(wm, C, nout)
    whi, wlo = split_bf16(oa.weight.detach())
    for part, src in ((hi, whi), (lo, wlo)):
        assert torch.equal(part[0, :, :, :nout], src[:, C:].reshape(nout, C, 9).permute(1, 2, 0))   # fe1 half
        assert torch.equal(part[1, :, :, :nout], src[:, :C].reshape(nout, C, 9).permute(1, 2, 0))   # decoder half
    for k, c in enumerate((idc, cfc)):
        if c is None:
            assert not bool(hi[:, :, :, nout + k].any()) and not bool(lo[:, :, :, nout + k].any())
        else:
            chi, clo = split_bf16(c.weight.detach())
            assert torch.equal(hi[0, :, :, nout + k], chi[0, C:].reshape(C, 9))
            assert torch.equal(lo[0, :, :, nout + k], clo[0, C:].reshape(C, 9))
            # the id / cf columns of source 1 are zero: their decoder halves are the VALU sums
            assert not bool(hi[1, :, :, nout + k].any()) and not bool(lo[1, :, :, nout + k].any())
    assert not bool(hi[:, :, :, nout + 2:].any()) and not bool(lo[:, :, :, nout + 2:].any())  # the padded columns
    # the layout itself: [source][chunk][tap][M-block][part][lane = 32 h + l32][8]
    v = wm.view(2, C // 16, 9, mb, 2, 64, 8)
    co, c, t = nout - 1, C - 3, 5
    at = (0, c // 16, t, co // 32, slice(None), 32 * ((c % 16) // 8) + co % 32, c % 8)
    assert torch.equal(v[at], torch.stack((whi[co, C + c, 1, 2], wlo[co, C + c, 1, 2])))


# ------------------------------------------------------------------ refusals before any device call
def _epi(**over):
    a = dict(dtype=0, fe1=P, fd_oa=P, fd_id=P, fd_cf=P, wm=P, wv=P, bias=P, off_aff=P, pred_init=P, conf=P, B=1, C=16,
             H=8, W=8, nout=24, stream=None)
    a.update(over)
    lib = _lib.get()
    rc = lib.nlspn_head_epilogue_x3(*a.values())
    return rc, lib.nlspn_last_error().decode()


def _pro(**over):
    a = dict(dtype=0, fe1=P, fd_oa=P, fd_id=P, fd_cf=P, wm=P, wv=P, bias=P, dep=P, gamma=P, pred_init=P, conf_out=P,
             aff_out=P, off_out=P, p0=P, B=1, C=16, H=8, W=8, kh=3, kw=3, kind=3, flags=1, stream=None)
    a.update(over)
    lib = _lib.get()
    rc = lib.nlspn_head_epilogue_prologue_x3(*a.values())
    return rc, lib.nlspn_last_error().decode()


@pytest.mark.parametrize("over,code,msg", [
    (dict(dtype=1), _lib.EUNSUPPORTED, "float32"),
    (dict(B=0), _lib.EINVAL, "empty input"),
    (dict(C=24), _lib.EINVAL, "multiple of 16"),
    (dict(C=8), _lib.EINVAL, "multiple of 16"),
    (dict(nout=0), _lib.EINVAL, "nout=0"),
    (dict(nout=159), _lib.EUNSUPPORTED, "at most 158"),
    (dict(fe1=None), _lib.EINVAL, "null pointer"),
    (dict(wm=None), _lib.EINVAL, "null pointer"),
    (dict(off_aff=None), _lib.EINVAL, "null pointer"),
    (dict(fd_id=None), _lib.EINVAL, "both be given or both NULL"),
    (dict(conf=None), _lib.EINVAL, "both be given or both NULL"),
])
def test_epilogue_x3_validates_before_any_device_call(over, code, msg):
    rc, text = _epi(**over)
    assert rc == code and msg in text, (rc, text)


@pytest.mark.parametrize("over,code,msg", [
    (dict(dtype=1), _lib.EUNSUPPORTED, "float32"),
    (dict(H=0), _lib.EINVAL, "empty input"),
    (dict(kh=5, kw=5), _lib.EUNSUPPORTED, "3x3 propagation only"),
    (dict(kind=9), _lib.EINVAL, "affinity kind"),
    (dict(C=40), _lib.EINVAL, "multiple of 16"),
    (dict(fd_id=None), _lib.EINVAL, "null pointer"),
    (dict(gamma=None), _lib.EINVAL, "null pointer"),
    (dict(p0=None), _lib.EINVAL, "null pointer"),
    (dict(conf_out=None), _lib.EINVAL, "both be given or both NULL"),
    (dict(dep=None), _lib.EINVAL, "preserve_input requires dep"),
])
def test_prologue_x3_validates_before_any_device_call(over, code, msg):
    rc, text = _pro(**over)
    assert rc == code and msg in text, (rc, text)


def test_x3_refusals_are_the_f32_entries():
    """Same code and message as the f32 namesake for the same bad argument."""
    lib = _lib.get()
    for over in (dict(C=24), dict(nout=159), dict(fe1=None), dict(fd_id=None), dict(dtype=1)):
        a = dict(dtype=0, fe1=P, fd_oa=P, fd_id=P, fd_cf=P, wm=P, wv=P, bias=P, off_aff=P, pred_init=P, conf=P, B=1,
                 C=16, H=8, W=8, nout=24, stream=None)
        a.update(over)
        rc32 = lib.nlspn_head_epilogue(*a.values())
        text32 = lib.nlspn_last_error().decode()
        assert (rc32, text32) == _epi(**over)
    nm = ctypes.c_int64()
    assert lib.nlspn_head_x3_packed_size(24, 24, ctypes.byref(nm), None, None) == _lib.EINVAL
    assert lib.nlspn_head_x3_packed_size(16, 159, ctypes.byref(nm), None, None) == _lib.EUNSUPPORTED
    assert lib.nlspn_head_x3_pack_weights(P, P, P, P, P, P, None, P, P, 16, 24, None) == _lib.EINVAL
    assert "null pointer" in lib.nlspn_last_error().decode()
    assert lib.nlspn_head_x3_pack_weights(None, P, P, P, P, P, P, P, P, 16, 24, None) == _lib.EINVAL
    assert lib.nlspn_abi_version() == 3


def test_python_refuses_an_unknown_precision():
    x = torch.zeros(1, 16, 4, 4)
    oa, idc, cfc = _convs(16, 24)
    for bad in ("bf16", "fp16", "BF16X3", None, 3):
        with pytest.raises(ValueError, match="precision"):
            HD.head_epilogue(x, x, oa, precision=bad)
        with pytest.raises(ValueError, match="precision"):
            HD.head_epilogue_prologue(x, x, oa, x, idc, None, 1.0, precision=bad)
    assert HD.PRECISIONS == ("fp32", "bf16x3") and set(HD.stats) == set(HD.PRECISIONS)


# ------------------------------------------------------------------ resource remarks
def test_x3_unit_compiles_without_scratch(tmp_path):
    sys.path.insert(0, CSRC)
    import resource_usage as RU
    path = os.path.join(RU.BUILD_DIR, "nlspn_kern_heads_x3.ru.txt")
    if os.path.exists(path):
        rows = RU.parse(open(path).read())
    else:
        out = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
                              "-ffp-contract=off", "-Rpass-analysis=kernel-resource-usage", "-c", "-o",
                              str(tmp_path / "hx3.o"), os.path.join(CSRC, "nlspn_kern_heads_x3.hip")],
                             capture_output=True, text=True, cwd=CSRC)
        assert out.returncode == 0, out.stderr[-2000:]
        rows = RU.parse(out.stderr)
    # MB in {1, 2, 3, 5} x {VEC, scalar}, the two fused-prologue builds, the x3 packer, and the
    # f32 packer every unit that includes nlspn_heads.h carries (static)
    x3 = [n for n in rows if "headsx3_kernel" in n]
    assert len(x3) == 10 and len(rows) == 12, sorted(rows)
    assert sum("headsx3_pack_kernel" in n for n in rows) == 1 and sum("heads_pack_kernel" in n for n in rows) == 1
    bad = {n: (r.get("ScratchSize"), r.get("VGPRs Spill")) for n, r in rows.items()
           if r.get("ScratchSize", 0) != 0 or r.get("VGPRs Spill", 0) != 0}
    assert not bad, bad


# ------------------------------------------------------------------ the switch
def _model(use_gru=False):
    args = types.SimpleNamespace(prop_kernel=3, affinity="TGASS", affinity_gamma=0.5, prop_time=2,
                                 preserve_input=True, always_clip=False, conf_prop=True, offset=True,
                                 network="resnet18", from_scratch=True, zero_init_aff=False, use_GRU=use_gru,
                                 use_S2D=False, GRU_hidden_dim=8, GRU_input_dim=8, lr=1e-3, max_depth=10.0,
                                 patch_height=32, patch_width=32, model_name="NLSPN")
    torch.manual_seed(0)
    return NLSPNModel(args).eval()


def test_head_precision_accepts_bf16x3_and_refuses_the_rest():
    m = _model()
    assert m.head_precision == "fp32"
    m.head_precision = "bf16x3"
    assert m.head_precision == "bf16x3"
    for bad in ("bf16", "fp16", "half", 16, None, "FP32", "BF16X3"):
        with pytest.raises(ValueError, match="head_precision"):
            m.head_precision = bad
    assert m.head_precision == "bf16x3"  # a refused value changes nothing
    assert "head_precision" not in m.state_dict() and "_head_precision" not in m.state_dict()


def test_head_precision_is_ignored_on_cpu_and_under_gradients():
    m = _model()
    g = torch.Generator().manual_seed(1)
    s = {"rgb": torch.rand((1, 3, 32, 32), generator=g), "dep": torch.rand((1, 1, 32, 32), generator=g)}
    before = dict(HD.stats)
    with torch.no_grad():
        a = m.heads(s)
        m.head_precision = "bf16x3"
        b = m.heads(s)
    for x, y in zip(a, b):
        assert torch.equal(x, y)  # the torch convolutions, both times
    m.train()
    for p in m.parameters():
        p.requires_grad_(True)
    m.eval()
    c = m.heads(s)  # gradients on: the torch convolutions, with a graph
    assert c[0].requires_grad and torch.allclose(c[1], a[1], atol=1e-6)
    assert HD.stats == before  # no kernel of either precision ran


# ------------------------------------------------------------------ the emulation yardstick
def _split64(t):
    hi, lo = split_bf16(t.float())
    return hi.double(), lo.double()


def emu_conv(x, w, drop=None, swap=False):
    """The three split products of a 3x3 convolution in float64 (no bias)."""
    xh, xl = _split64(x)
    wh, wl = _split64(w)
    if swap:
        xh, xl = xl, xh
    terms = {"hh": F.conv2d(xh, wh, None, padding=1), "hl": F.conv2d(xl, wh, None, padding=1),
             "lh": F.conv2d(xh, wl, None, padding=1)}
    return sum(v for k, v in terms.items() if k != drop)


@pytest.mark.parametrize("C,nout,want", [(64, 24, 7.1e-7), (16, 144, 1.45e-6)])
def test_emulation_is_inside_the_term_bound_and_every_part_matters(C, nout, want):
    torch.manual_seed(C)
    conv = nn.Conv2d(2 * C, nout, 3, padding=1)
    g = torch.Generator().manual_seed(nout)
    x = torch.rand((1, 2 * C, 20, 36), generator=g)
    w = conv.weight.detach()
    full = F.conv2d(x.double(), w.double(), None, padding=1)
    bound = F.conv2d(x.double().abs(), w.double().abs(), None, padding=1)
    ratio = lambda y: float(((y - full).abs() / bound).max())  # noqa: E731
    got = {"emu": ratio(emu_conv(x, w)), "no_hl": ratio(emu_conv(x, w, drop="hl")),
           "no_lh": ratio(emu_conv(x, w, drop="lh")), "swap": ratio(emu_conv(x, w, swap=True))}
    print(f"C={C} nout={nout}:", {k: f"{v:.3g}" for k, v in got.items()})
    assert got["emu"] <= 2.0 ** -15
    assert 0.5 * want <= got["emu"] <= 2.0 * want  # the figure of the docstring, on these very inputs
    for k in ("no_hl", "no_lh", "swap"):
        assert got[k] >= 100 * 2e-6, (k, got[k])
