"""GPU: the split-bf16 head epilogue (nlspn_head_epilogue_x3, csrc/nlspn_heads_x3.h) per element
against two float64 references, on the small shapes where the tiling can go wrong.  Operand
tensors sit between NaN guards (a read outside one poisons the output), outputs between
sentinels.  With bound = sum |w||x| + |b| (oracle.conv3x3 on absolute values):
    emu: the three split products of the very operands passed in (w_hi x_hi + w_hi x_lo +
         w_lo x_hi over fe1 and, for the off / aff columns, off_aff_fd1) plus the unsplit VALU half
         (id_fd1 / cf_fd1):                      |got - emu| <= c_acc * bound + e_act
    ref: the unsplit convolution (oracle.head_epilogue):
                                                 |got - ref| <= (2^-15 + c_acc) * bound + e_act
c_acc = min(2e-6, (3 n + 2) 2^-24) for an n-term sum (n = 18 C: 2e-6 in every case here) and
e_act = 4e-7 on the sigmoid output only (expf and the division).  ReLU and the sigmoid (slope
<= 1/4) do not widen a pre-activation difference.  A kernel that drops a cross product or swaps
hi and lo is off by 2e-4 or more of the bound (tests/test_heads_x3_cpu.py).

Measured on the MI355X, worst |got - want| / bar per case over the three outputs (1.0 = the bar):
    case                      emu      ref
    2x64x40x64/24             0.094    0.027
    2x64x37x50/24             0.085    0.028
    1x64x9x8/8                0.032    0.018
    2x32x24x96/48             0.088    0.045
    1x64x20x36/72             0.072    0.029
    1x16x13x40/144            0.085    0.061
    1x16x1x36/24              0.051    0.068
    1x16x9x1/24               0.035    0.058
and at the model level (1x3x64x96, T = 18, resnet18) `pred` RMSE 3.3e-6 against the f32 heads
(largest difference 1.0e-4), under the 1e-4 bar.
"""
import types

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from nlspn_eccv20_amd import NLSPNModel, _lib, propagate, propagate_normalized
from nlspn_eccv20_amd import heads as HD
from nlspn_eccv20_amd.gru import split_bf16
from nlspn_eccv20_amd.heads import HeadWeights, head_epilogue, head_epilogue_prologue
from oracle import oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 4096
SENT = -77.25
TERM = 2.0 ** -15
E_ACT = 4e-7

CASES = [
    (2, 64, 40, 64, 24, True, True),      # K=8 with offsets (the default model), W % 4 == 0
    (2, 64, 37, 50, 24, True, True),      # partial tiles, W % 4 != 0 (scalar VALU window)
    (1, 64, 9, 8, 8, True, False),        # no offsets (nout = K), no confidence head
    (2, 32, 24, 96, 48, False, True),     # K=16 (2 M-blocks), no id head
    (1, 64, 20, 36, 72, True, True),      # K=24 (3 M-blocks)
    (1, 16, 13, 40, 144, True, True),     # K=48 (5 M-blocks)
    (1, 16, 1, 36, 24, True, True),       # a single row
    (1, 16, 9, 1, 24, True, True),        # a single column
]


def c_acc(n):
    return min(2e-6, (3 * n + 2) * 2.0 ** -24)


def _guarded(t):
    """t on the device between NaN guards: a read outside it poisons the output."""
    t = t.contiguous()
    buf = torch.full((t.numel() + 2 * GUARD,), float("nan"), device=DEV, dtype=t.dtype)
    v = buf[GUARD:GUARD + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def _out(shape):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), SENT, device=DEV, dtype=torch.float32)
    return buf, buf[GUARD:GUARD + n].view(shape)


def _guard_ok(buf):
    return bool((buf[:GUARD] == SENT).all()) and bool((buf[-GUARD:] == SENT).all())


def _case(B, C, H, W, nout, with_id=True, with_cf=True, seed=0):
    torch.manual_seed(seed)
    oa = nn.Conv2d(2 * C, nout, 3, padding=1).to(DEV)
    idc = nn.Conv2d(2 * C, 1, 3, padding=1).to(DEV) if with_id else None
    cfc = nn.Conv2d(2 * C, 1, 3, padding=1).to(DEV) if with_cf else None
    g = torch.Generator(device=DEV).manual_seed(seed + 1)
    src = [_guarded(torch.randn((B, C, H, W), device=DEV, generator=g) * 3) for _ in range(4)]  # both signs
    return oa, idc, cfc, src


def _split64(t):
    hi, lo = split_bf16(t.detach().float().cpu())
    return hi.double(), lo.double()


def _emu3(x, w):
    """conv(w_hi, x_hi) + conv(w_hi, x_lo) + conv(w_lo, x_hi), float64, no bias."""
    xh, xl = _split64(x)
    wh, wl = _split64(w)
    cv = lambda a, b: F.conv2d(a, b, None, padding=1)  # noqa: E731
    return cv(xh, wh) + cv(xl, wh) + cv(xh, wl)


def _emu_head(conv, fd, fe1, split_fd):
    """The pre-activation of one head as the kernel forms it: the fe1 half split; the decoder
    half split (off_aff) or unsplit on the VALU (id, cf); bias."""
    C = fe1.shape[1]
    w = conv.weight.detach().cpu()
    y = _emu3(fe1, w[:, C:])
    if split_fd:
        y = y + _emu3(fd, w[:, :C])
    else:
        y = y + F.conv2d(fd.detach().cpu().double(), w[:, :C].double(), None, padding=1)
    return y + conv.bias.detach().cpu().double()[None, :, None, None]


def _bound(fd, fe1, conv):
    n = lambda t: t.detach().double().cpu().numpy()  # noqa: E731
    return torch.from_numpy(O.conv3x3(np.abs(np.concatenate([n(fd), n(fe1)], 1)), np.abs(n(conv.weight)),
                                      np.abs(n(conv.bias))))


def _ratios(got, emu, ref, bound, n, e_act):
    """worst |got - want| / bar against each reference (<= 1 passes)."""
    got = got.detach().double().cpu()
    assert bool(torch.isfinite(got).all()), "a non-finite output (a read of a NaN guard?)"
    c = c_acc(n)
    return (float(((got - emu).abs() / (c * bound + e_act)).max()),
            float(((got - ref).abs() / ((TERM + c) * bound + e_act)).max()))


def _name(B, C, H, W, nout):
    return f"{B}x{C}x{H}x{W}/{nout}"


@pytest.mark.parametrize("B,C,H,W,nout,with_id,with_cf", CASES)
def test_head_epilogue_x3_per_element(B, C, H, W, nout, with_id, with_cf, record_metric):
    oa, idc, cfc, (fe1, fd_oa, fd_id, fd_cf) = _case(B, C, H, W, nout, with_id, with_cf, seed=H + W)
    fd_id, fd_cf = (fd_id if with_id else None), (fd_cf if with_cf else None)
    hw = HeadWeights()
    before = dict(HD.stats)
    with torch.no_grad():
        p, o, c = head_epilogue(fe1, fd_oa, oa, fd_id, idc, fd_cf, cfc, weights=hw, precision="bf16x3")
    torch.cuda.synchronize()
    # path proof: one launch of the bf16x3 kernel, none of the f32 one
    assert HD.stats["bf16x3"] == before["bf16x3"] + 1 and HD.stats["fp32"] == before["fp32"]
    # the pack kernel against the torch reference of the layout; wv and bias against the f32 pack
    e3, e32 = hw.get(oa, idc, cfc, "bf16x3"), hw.get(oa, idc, cfc, "fp32")
    assert e3.wm.dtype == torch.bfloat16
    assert torch.equal(e3.wm.view(torch.int16), HD.pack_wm_x3_reference(oa, idc, cfc).view(torch.int16))
    assert torch.equal(e3.wv, e32.wv) and torch.equal(e3.bias, e32.bias)
    # the C entry itself: packed weights between guards, outputs between sentinels; the same bits
    wm, wv, bias = _guarded(e3.wm), _guarded(e3.wv), _guarded(e3.bias)
    bo, o2 = _out((B, nout, H, W))
    bp, p2 = _out((B, 1, H, W)) if with_id else (None, None)
    bc, c2 = _out((B, 1, H, W)) if with_cf else (None, None)
    _lib.call("nlspn_head_epilogue_x3", fe1.device, _lib.DTYPE_F32, fe1, fd_oa, fd_id, fd_cf, wm, wv, bias, o2, p2, c2,
              B, C, H, W, nout, _lib.STREAM)
    torch.cuda.synchronize()
    assert all(_guard_ok(b) for b in (bo, bp, bc) if b is not None), "a store outside an output"
    assert torch.equal(o2, o) and (p is None or torch.equal(p2, p)) and (c is None or torch.equal(c2, c))

    n = lambda t: None if t is None else t.detach().double().cpu().numpy()  # noqa: E731
    rp, ro, rc = O.head_epilogue(n(fe1), n(fd_oa), n(oa.weight), n(oa.bias),
                                 n(fd_id), n(idc.weight) if idc else None, n(idc.bias) if idc else None,
                                 n(fd_cf), n(cfc.weight) if cfc else None, n(cfc.bias) if cfc else None)
    terms = 18 * C
    worst = [_ratios(o, _emu_head(oa, fd_oa, fe1, True), torch.from_numpy(ro), _bound(fd_oa, fe1, oa), terms, 0.0)]
    if with_id:
        worst.append(_ratios(p, torch.relu(_emu_head(idc, fd_id, fe1, False)), torch.from_numpy(rp),
                             _bound(fd_id, fe1, idc), terms, 0.0))
    else:
        assert p is None
    if with_cf:
        worst.append(_ratios(c, torch.sigmoid(_emu_head(cfc, fd_cf, fe1, False)), torch.from_numpy(rc),
                             _bound(fd_cf, fe1, cfc), terms, E_ACT))
    else:
        assert c is None
    emu, ref = max(w[0] for w in worst), max(w[1] for w in worst)
    name = _name(B, C, H, W, nout)
    print(f"heads_x3/{name}: emu {emu:.3g} ref {ref:.3g} (of the bar)")
    record_metric(f"heads_x3/{name}/emu", emu)
    record_metric(f"heads_x3/{name}/ref", ref)
    assert emu <= 1.0 and ref <= 1.0, (emu, ref)


def test_default_path_untouched():
    """precision="fp32" is the call without the argument: same kernel, same pack, same bits."""
    oa, idc, cfc, (fe1, fd_oa, fd_id, fd_cf) = _case(2, 64, 37, 50, 24, seed=3)
    hw = HeadWeights()
    before = dict(HD.stats)
    with torch.no_grad():
        a = head_epilogue(fe1, fd_oa, oa, fd_id, idc, fd_cf, cfc, weights=hw)
        b = head_epilogue(fe1, fd_oa, oa, fd_id, idc, fd_cf, cfc, weights=hw, precision="fp32")
        x = head_epilogue(fe1, fd_oa, oa, fd_id, idc, fd_cf, cfc, weights=hw, precision="bf16x3")
        c = head_epilogue(fe1, fd_oa, oa, fd_id, idc, fd_cf, cfc, weights=hw)
    assert all(torch.equal(u, v) for u, v in zip(a, b)) and all(torch.equal(u, v) for u, v in zip(a, c))
    assert not torch.equal(a[1], x[1])  # another kernel, other bits
    assert HD.stats["fp32"] == before["fp32"] + 3 and HD.stats["bf16x3"] == before["bf16x3"] + 1
    e32, e3 = hw.get(oa, idc, cfc), hw.get(oa, idc, cfc, "bf16x3")
    assert e32 is hw.get(oa, idc, cfc, "fp32") and e32 is not e3 and e32.wm.dtype == torch.float32


def test_two_runs_give_the_same_bits():
    oa, idc, cfc, (fe1, fd_oa, fd_id, fd_cf) = _case(2, 64, 37, 50, 24, seed=4)
    hw = HeadWeights()
    with torch.no_grad():
        a = head_epilogue(fe1, fd_oa, oa, fd_id, idc, fd_cf, cfc, weights=hw, precision="bf16x3")
        b = head_epilogue(fe1, fd_oa, oa, fd_id, idc, fd_cf, cfc, weights=hw, precision="bf16x3")
    assert all(torch.equal(u, v) for u, v in zip(a, b))


def test_nan_reaches_exactly_the_neighbourhood():
    oa, idc, cfc, (fe1, fd_oa, fd_id, fd_cf) = _case(1, 16, 16, 32, 24, seed=5)
    fe1[0, 3, 5, 7] = float("nan")
    with torch.no_grad():
        p, o, c = head_epilogue(fe1, fd_oa, oa, fd_id, idc, fd_cf, cfc, precision="bf16x3")
    for plane in (*o[0], p[0, 0], c[0, 0]):
        bad = torch.isnan(plane)
        assert bad[4:7, 6:9].all() and bad.sum().item() == 9


def test_weight_cache_follows_updates_per_precision():
    oa, idc, cfc, (fe1, fd_oa, fd_id, fd_cf) = _case(1, 16, 12, 32, 24, seed=6)
    hw = HeadWeights()
    with torch.no_grad():
        _, x1, _ = head_epilogue(fe1, fd_oa, oa, weights=hw, precision="bf16x3")
        _, f1, _ = head_epilogue(fe1, fd_oa, oa, weights=hw)
        oa.weight.mul_(2.0)   # in-place update: new version counter -> both entries repacked
        oa.bias.mul_(2.0)
        _, x2, _ = head_epilogue(fe1, fd_oa, oa, weights=hw, precision="bf16x3")
        _, f2, _ = head_epilogue(fe1, fd_oa, oa, weights=hw)
    assert torch.equal(x2, 2 * x1) and torch.equal(f2, 2 * f1)  # a power of two: exact in both kernels
    assert torch.allclose(x1, f1, rtol=1e-4, atol=1e-4)


# ------------------------------------------------------------------ the fused prologue
def _pro_case(B, C, H, W, seed=0, with_cf=True):
    torch.manual_seed(seed)
    oa = nn.Conv2d(2 * C, 24, 3, padding=1).to(DEV)
    idc = nn.Conv2d(2 * C, 1, 3, padding=1).to(DEV)
    cfc = nn.Conv2d(2 * C, 1, 3, padding=1).to(DEV) if with_cf else None
    with torch.no_grad():
        oa.weight.mul_(3.0)  # offsets of a few pixels, affinities of either sign
        idc.bias.add_(2.0)
    g = torch.Generator(device=DEV).manual_seed(seed + 1)
    src = [_guarded(torch.rand((B, C, H, W), device=DEV, generator=g)) for _ in range(4)]
    dep = torch.rand((B, 1, H, W), device=DEV, generator=g) * 10
    dep = dep * (torch.rand((B, 1, H, W), device=DEV, generator=g) < 0.05)
    return oa, idc, cfc, src, dep


def _run_both(oa, idc, cfc, src, dep, kind, T, preserve, clip):
    fe1, fd_oa, fd_id, fd_cf = src
    gamma = torch.tensor([4.0], device=DEV)
    hw = HeadWeights()
    before = HD.stats["bf16x3"]
    with torch.no_grad():
        pi, off_aff, conf = head_epilogue(fe1, fd_oa, oa, fd_id, idc, fd_cf if cfc else None, cfc, weights=hw,
                                          precision="bf16x3")
        ref = propagate(pi, dep if preserve else None, conf, off_aff[:, 16:], off_aff[:, :16], gamma, prop_time=T,
                        affinity=kind, preserve_input=preserve, always_clip=clip)
        h = head_epilogue_prologue(fe1, fd_oa, oa, fd_id, idc, dep if preserve else None, gamma, kind,
                                   fd_cf if cfc else None, cfc, preserve, clip, weights=hw, precision="bf16x3")
        o = propagate_normalized(h["p0"], dep if preserve else None, h["confidence"], h["aff"], h["offset"], T,
                                 3, preserve, clip)
    torch.cuda.synchronize()
    assert HD.stats["bf16x3"] == before + 2
    assert torch.equal(h["pred_init"], pi)
    assert torch.equal(h["aff"], ref["aff"]) and torch.equal(h["offset"], ref["offset"])
    if cfc is not None:
        assert torch.equal(h["confidence"], ref["confidence"])
    else:
        assert h["confidence"] is None
    assert torch.equal(o["pred_inter_tensor"], ref["pred_inter_tensor"])  # every pred_inter plane
    assert torch.equal(o["pred"], ref["pred"])


@pytest.mark.parametrize("kind", ["TGASS", "AS", "ASS", "TC"])
@pytest.mark.parametrize("preserve,clip", [(True, False), (False, True), (True, True)])
def test_fused_prologue_x3_bitexact(kind, preserve, clip):
    _run_both(*_pro_case(2, 64, 40, 64, seed=1), kind, 18, preserve, clip)


@pytest.mark.parametrize("B,C,H,W,T,with_cf", [
    (1, 16, 13, 40, 6, True),      # partial tiles
    (3, 32, 37, 50, 6, True),      # W % 4 != 0: scalar kernels, per-iteration steps
    (1, 16, 24, 32, 1, False),     # T = 1, no confidence head
])
def test_fused_prologue_x3_shapes(B, C, H, W, T, with_cf):
    _run_both(*_pro_case(B, C, H, W, seed=2, with_cf=with_cf), "TGASS", T, True, False)


def test_fused_prologue_x3_per_iteration_path(monkeypatch):
    """propagate_normalized's per-iteration form (NLSPN_RESIDENT=0) at a width the resident kernel
    would take."""
    monkeypatch.setenv("NLSPN_RESIDENT", "0")
    _run_both(*_pro_case(2, 16, 40, 64, seed=4), "TGASS", 7, True, False)


# ------------------------------------------------------------------ the model
def _model(use_gru, H=64, W=96, T=18):
    args = types.SimpleNamespace(prop_kernel=3, affinity="TGASS", affinity_gamma=0.5, prop_time=T,
                                 preserve_input=True, always_clip=False, conf_prop=True, offset=True,
                                 network="resnet18", from_scratch=True, zero_init_aff=False, use_GRU=use_gru,
                                 use_S2D=False, GRU_hidden_dim=128, GRU_input_dim=128, lr=1e-3, max_depth=10.0,
                                 patch_height=H, patch_width=W, model_name="NLSPN")
    torch.manual_seed(0)
    return NLSPNModel(args).to(DEV).eval()


def _sample(H=64, W=96):
    g = torch.Generator(device=DEV).manual_seed(5)
    rgb = torch.rand((1, 3, H, W), device=DEV, generator=g)
    dep = torch.rand((1, 1, H, W), device=DEV, generator=g) * 10 * (torch.rand((1, 1, H, W), device=DEV,
                                                                                generator=g) < 0.05)
    return {"rgb": rgb, "dep": dep}


def test_model_head_precision(record_metric):
    m, other = _model(False), _model(False)   # `other` never touches the switch
    s = _sample()
    with torch.no_grad():
        # one decoder pass for all (MIOpen may pick another algorithm on a second pass)
        dec = m._decoder(s)
        before = dict(HD.stats)
        f32 = m._forward_fused(*dec, s["dep"])
        assert HD.stats["fp32"] == before["fp32"] + 1 and HD.stats["bf16x3"] == before["bf16x3"]
        m.head_precision = "bf16x3"
        x3 = m._forward_fused(*dec, s["dep"])
        assert HD.stats["bf16x3"] == before["bf16x3"] + 1 and HD.stats["fp32"] == before["fp32"] + 1
        m.head_precision = "fp32"
        back = m._forward_fused(*dec, s["dep"])
        dflt = other._forward_fused(*dec, s["dep"])
        assert HD.stats["bf16x3"] == before["bf16x3"] + 1
    for k in ("pred", "pred_init", "offset", "aff", "confidence"):
        assert torch.equal(f32[k], dflt[k]) and torch.equal(f32[k], back[k]), k
    assert all(torch.equal(a, b) for a, b in zip(f32["pred_inter"], dflt["pred_inter"]))
    rmse = float((x3["pred"].double() - f32["pred"].double()).pow(2).mean().sqrt())
    print(f"heads_x3/model/pred_rmse {rmse:.3g}  max {float((x3['pred'] - f32['pred']).abs().max()):.3g}")
    record_metric("heads_x3/model/pred_rmse", rmse)
    assert rmse <= 1e-4
    assert not torch.equal(x3["pred_init"], f32["pred_init"])  # the other kernel did run


def test_model_head_precision_with_the_gru():
    """GRU mode takes heads() (no fused prologue): the switch reaches head_epilogue there."""
    m = _model(True, 32, 32, 2)
    s = _sample(32, 32)
    with torch.no_grad():
        before = dict(HD.stats)
        a = m.heads(s)
        assert HD.stats["fp32"] == before["fp32"] + 1 and HD.stats["bf16x3"] == before["bf16x3"]
        m.head_precision = "bf16x3"
        b = m.heads(s)
        assert HD.stats["bf16x3"] == before["bf16x3"] + 1 and HD.stats["fp32"] == before["fp32"] + 1
    for u, v in zip(a, b):
        assert torch.allclose(u, v, rtol=1e-3, atol=1e-3)
