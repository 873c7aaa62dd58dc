"""GPU: the split-bf16 data gradients of the GRU-mode convolutions per element, through the C ABI
(nlspn_gconv_x3_dgrad on the NLSPN_GCX3_DG_* presets, nlspn_gconv_x3_split,
nlspn_gconv_x3_dgrad_covers).  Cases, references and bars: tests/_gconv_x3_dgrad_cases.py (its
docstring derives the bars; none comes from these kernels).

Every case asserts, for every element of every output,
    finite,  |got - emulation| <= c X + e   and   |got - ref64| <= c X + e + 2^-15 X
(emulation: the three split products of the very operands passed, in float64; ref64: the unsplit
operands; c = min(2e-6, (3 n + 4) 2^-24)) on operands that are views into NaN buffers and outputs
pre-filled with NaN between sentinel guards (an element not written stays NaN, a store outside
breaks a guard).  The gradient is passed as to_c8x2 of the f32 operand, the weights as
pack_adjoint_x3 / pack_adjoint_s1_x3 make them from the forward layer's own tensor.  Where the
split copy dxs is asked for it equals split_bf16 of the f32 output bit for bit, and the f32
output has the bits it has without dxs.  nlspn_gconv_x3_split equals to_c8x2 bit for bit.  Every
entry gives the same bits on a second run.

Measured on an MI355X (gconv_x3_dgrad/<preset>/<case id>): the worst |got - emulation| / X per
preset and the case that gave it (informational: the bars above do not depend on them):
    DG_T2      1.97e-7  x3dg80-2x48>64-3x43              DG_T2_C16  1.98e-7  x3dg81-2x48>16-6x41-off1.0
    DG_S2      1.96e-7  x3dg82-2x48>64-17x39             DG_S1      2.21e-7  x3dg83-2x20>64-7x21-cg20
    (the Tanh cases: 0 .. 2.3e-8 beside e; the bar c is 2e-6 at every case's term count)
All 49 cases and the split, refusal and rerun assertions passed on the first run.
"""
import pytest
import torch
import torch.nn as nn

import _gconv_bwd_cases as bc
import _gconv_x3_dgrad_cases as xc
from nlspn_eccv20_amd import _lib
from nlspn_eccv20_amd import gru as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _pack(c, w):
    """The split adjoint weights as the model makes them, from the forward layer's own tensor."""
    wd = w.to(DEV)
    if c["mode"] == bc.S1:
        return G.pack_adjoint_s1_x3(wd)
    if c["mode"] == bc.T2:   # the forward layer is a stride-2 conv cout -> cg
        mod = nn.Conv2d(c["cout"], c["cg"], 3, 2, 1)
    else:                    # a transposed conv cout -> cg
        mod = nn.ConvTranspose2d(c["cout"], c["cg"], 3, 2, 1, 1)
    with torch.no_grad():
        mod.weight = nn.Parameter(wd)
    dg, adj = G.pack_adjoint_x3(mod)
    assert dg == c["preset"], (c["id"], dg)
    return adj


def _guarded(t):
    """t (any dtype) on the device as a view into a NaN buffer."""
    t = t.contiguous()
    buf = torch.full((t.numel() + 2 * bc.GUARD,), float("nan"), device=DEV, dtype=t.dtype)
    v = buf[bc.GUARD:bc.GUARD + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def _split_out(shape):
    """(buffer, view) of a c8x2 output pre-filled with NaN between sentinels."""
    B, C, H, W = shape
    n = B * ((C + 7) // 8) * 2 * H * W * 8
    buf = torch.full((n + 2 * bc.GUARD,), bc.SENT, device=DEV, dtype=torch.bfloat16)
    v = buf[bc.GUARD:bc.GUARD + n].view(B, (C + 7) // 8, 2, H, W, 8)
    v.fill_(float("nan"))
    return buf, v


def _launch(c, o, gs, wpk, ysave, want_dxs):
    """One call on fresh guarded outputs: (f32 output (B, cout, Ho, Wo) on the CPU, dxs or None)."""
    B, cout, Ho, Wo, split = c["B"], c["cout"], c["Ho"], c["Wo"], c["split"]
    adds = [None, None]
    if o["add"] is not None:
        adds = [o["add"][:, :split].contiguous(), o["add"][:, split:].contiguous() if split < cout else None]
    alias = c["add"] == "alias"
    b0, dx0 = bc.guarded_out((B, split, Ho, Wo), DEV, fill=adds[0] if alias else None)
    b1, dx1 = bc.guarded_out((B, cout - split, Ho, Wo), DEV, fill=adds[1] if alias else None) if split < cout else (None, None)
    a0, a1 = (dx0, dx1) if alias else (bc.guarded(adds[0], DEV), bc.guarded(adds[1], DEV))
    bs, dxs = _split_out((B, cout, Ho, Wo)) if want_dxs else (None, None)
    _lib.call("nlspn_gconv_x3_dgrad", gs.device, c["preset"], gs, c["cg"], wpk, ysave, a0, a1, dx0, dx1, split, dxs, B,
              c["Hg"], c["Wg"], cout, Ho, Wo, c["act"], c["scale"], _lib.STREAM)
    torch.cuda.synchronize()
    assert bc.guards_intact(b0) and (b1 is None or bc.guards_intact(b1)), "a store outside an output (beyond cout or the stored size)"
    if want_dxs:
        assert bool((bs[:bc.GUARD] == bc.SENT).all()) and bool((bs[-bc.GUARD:] == bc.SENT).all()), "a store outside dxs"
    return (dx0 if dx1 is None else torch.cat([dx0, dx1], 1)).cpu(), (dxs.cpu() if want_dxs else None)


def _run(cid, record):
    c = xc.BY_ID[cid]
    o = bc.dgrad_operands(cid)
    R = xc.reference(cid)
    lib = _lib.get()
    assert lib.nlspn_gconv_x3_dgrad_covers(c["preset"], c["cg"], c["cout"], c["Hg"], c["Wg"], c["Ho"], c["Wo"]) == 1
    gs = _guarded(G.to_c8x2(o["g"].to(DEV)))
    wpk = _guarded(_pack(c, o["w"]))
    ysave = bc.guarded(o["ysave"], DEV)
    got, dxs = _launch(c, o, gs, wpk, ysave, c["dxs"])
    name = f"{xc.NAMES[c['preset']]}/{cid}"
    got64 = got.double()
    assert bool(torch.isfinite(got64).all()), f"{name}: a non-finite output (an element not written, or a read of a NaN guard)"
    bar = R["c"] * R["X"] + R["e"]
    err = (got64 - R["emu"]).abs()
    worst = bc.ratio(got, R["emu"], R["X"], R["e"])
    record(f"gconv_x3_dgrad/{name}", worst)
    print(f"gconv_x3_dgrad/{name}: worst |got - emulation| / X = {worst:.3g}")
    bad = ~(err <= bar)
    assert not bool(bad.any()), (f"{name}: {int(bad.sum())} of {bad.numel()} elements outside c = {float(R['c'].max()):g} of the "
                                 f"emulation (worst ratio {worst:.3g}), first at {bad.nonzero()[:6].tolist()}")
    assert bool(((got64 - R["ref"]).abs() <= bar + xc.SPLIT_BOUND * R["X"]).all()), f"{name}: outside the bar against float64"
    if c["act"] == bc.ACT_RELU:  # at y <= 0 (+0, -0 and negatives): exactly the add, or +0
        off = ~(o["ysave"] > 0)
        want = o["add"][off] if o["add"] is not None else torch.zeros(int(off.sum()))
        assert int(off.sum()) >= len(bc.RELU_PLANTS) and torch.equal(got[off], want)
    # the same bits on a second run; with dxs: the f32 bits it has without, and dxs their split
    again, dxs2 = _launch(c, o, gs, wpk, ysave, c["dxs"])
    assert torch.equal(again, got) and (dxs is None or torch.equal(dxs2.view(torch.int16), dxs.view(torch.int16)))
    if c["dxs"]:
        plain, _ = _launch(c, o, gs, wpk, ysave, False)
        assert torch.equal(plain.view(torch.int32), got.view(torch.int32))
        assert torch.equal(dxs.view(torch.int16), G.to_c8x2(got).view(torch.int16))


IDS = lambda cases: [c["id"] for c in cases]  # noqa: E731


@pytest.mark.parametrize("cid", IDS(xc.BAND + xc.GRIDS))
def test_band_and_tile_edges(cid, record_metric):
    """One full band, one pixel more and 1 x 1 under every preset; 17 x 39, 3 x 43 (and 4 x 33)
    under the 64-channel transposed and stride-2 tilings: an uneven last band, an empty tile."""
    _run(cid, record_metric)


@pytest.mark.parametrize("cid", IDS(xc.CHANNELS + xc.CROP))
def test_channel_edges_and_cropped_outputs(cid, record_metric):
    """cg = 20 (a padded 16-channel chunk), cout no multiple of the co tile (72 on 64, 8 on 16), and
    the transposed adjoints' output one row and / or one column short: nothing stored outside."""
    _run(cid, record_metric)


@pytest.mark.parametrize("cid", IDS(xc.EPI + xc.GRU))
def test_epilogue_and_the_convgru_calls(cid, record_metric):
    """ReLU (planted +0, -0, the smallest normal, negatives) and Tanh (+-1 and within ulps of them)
    on the saved output at scale 0.25 without and with an addend; the ConvGRU's two calls: two
    outputs split at hc, the second adding into both in place."""
    _run(cid, record_metric)


@pytest.mark.parametrize("cid", IDS(xc.DXS))
def test_split_copy_is_the_split_of_the_f32_output(cid, record_metric):
    _run(cid, record_metric)


# ------------------------------------------------------------------ nlspn_gconv_x3_split
def _split(x):
    B, C, H, W = x.shape
    bs, xs = _split_out((B, C, H, W))
    _lib.call("nlspn_gconv_x3_split", x.device, x, xs, B, C, H, W, _lib.STREAM)
    torch.cuda.synchronize()
    assert bool((bs[:bc.GUARD] == bc.SENT).all()) and bool((bs[-bc.GUARD:] == bc.SENT).all()), "a store outside the output"
    return xs


def _split_input(shape, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=gen) * torch.exp2(torch.randint(-20, 20, shape, generator=gen).float())
    x.view(-1)[:4] = torch.tensor([0.0, -0.0, 2.0 ** -126, -(1.0 + 2.0 ** -8)])  # (a tie of the hi rounding)
    return x


@pytest.mark.parametrize("shape", [(2, 1, 5, 7), (2, 8, 5, 7), (2, 20, 5, 7), (2, 128, 5, 7), (1, 3, 3, 5)])
def test_split_equals_to_c8x2(shape):
    """C in {1, 8, 20, 128} at 5 x 7 and a tensor of 45 elements (no multiple of 4): bit for bit
    to_c8x2, pad channels zero, the same bits on a second run."""
    x = bc.guarded(_split_input(shape, 11), DEV)
    xs = _split(x)
    want = G.to_c8x2(x)
    assert xs.shape == want.shape and torch.equal(xs.view(torch.int16), want.view(torch.int16))
    assert torch.equal(_split(x).view(torch.int16), xs.view(torch.int16))
    assert torch.equal(G.from_c8x2(xs, shape[1]), G.from_c8x2(want, shape[1]))


def test_split_of_a_view_one_element_into_its_buffer():
    shape = (2, 20, 5, 7)
    x = _split_input(shape, 12)
    buf = torch.full((x.numel() + 2,), float("nan"), device=DEV)
    v = buf[1:1 + x.numel()].view(shape)   # 4-byte aligned only
    v.copy_(x)
    assert v.data_ptr() % 16 == 4
    assert torch.equal(_split(v).view(torch.int16), G.to_c8x2(x.to(DEV)).view(torch.int16))


# ------------------------------------------------------------------ refusals on the device
def test_refusals_launch_nothing():
    c = xc.BY_ID[xc.DXS[1]["id"]]   # DG_S2, 7 x 21
    o = bc.dgrad_operands(c["id"])
    gs, wpk = G.to_c8x2(o["g"].to(DEV)), _pack(c, o["w"])
    B, cg, cout, Hg, Wg, Ho, Wo = c["B"], c["cg"], c["cout"], c["Hg"], c["Wg"], c["Ho"], c["Wo"]
    buf, dx = bc.guarded_out((B, cout, Ho, Wo), DEV)
    dxs = torch.empty((B, cout // 8, 2, Ho, Wo, 8), device=DEV, dtype=torch.bfloat16)
    lib = _lib.get()

    def refused(code, msg, layer=c["preset"], ysave=None, dx1=None, split=cout, s=None, Hg=Hg, Wg=Wg, act=0):
        with pytest.raises(_lib.NlspnError, match=msg) as ei:
            _lib.call("nlspn_gconv_x3_dgrad", dx.device, layer, gs, cg, wpk, ysave, None, None, dx, dx1, split, s, B, Hg, Wg,
                      cout, Ho, Wo, act, 1.0, _lib.STREAM)
        assert ei.value.code == code

    refused(_lib.EINVAL, "not a split-bf16 data-gradient preset", layer=G.GCX3_S2)    # a forward x3 preset
    refused(_lib.EINVAL, "not a split-bf16 data-gradient preset", layer=G.GC_DG_S2)   # an f32 data-gradient preset
    assert lib.nlspn_gconv_x3_dgrad_covers(c["preset"], cg, cout, Hg - 1, Wg, Ho, Wo) == 0
    refused(_lib.EUNSUPPORTED, "stored cropped", Hg=Hg - 1)                           # a cropped stride-2-mode gradient
    refused(_lib.EUNSUPPORTED, "stored cropped", Wg=Wg - 1)
    refused(_lib.EINVAL, "split copy needs one output", dx1=dx, split=cout // 2, s=dxs)  # dxs with two outputs
    refused(_lib.EINVAL, "needs the saved output", act=bc.ACT_RELU)                   # an activation without ysave
    torch.cuda.synchronize()
    assert bool(torch.isnan(dx).all()) and bc.guards_intact(buf)   # nothing was launched
