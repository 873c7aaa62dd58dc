"""GPU: the backward of the GRU-mode convolutions per element against float64, through the C ABI
(nlspn_gconv_dgrad, nlspn_gconv_wgrad, nlspn_gconv_gru_gates_backward): every instantiated kernel
at the grids, crops, channel counts and slices where its tiling can go wrong.  Cases, operands,
references and bars: tests/_gconv_bwd_cases.py (its docstring derives the bars; none comes from
these kernels).  tests/test_gpu_gconv_bwd.py holds the same code by one relative L2 per tensor,
which a few wrong cells at a band edge, a crop or a short last K slice do not move.

Every case asserts, for every element of every output,
    finite  and  |got - ref64| <= c * X + e
on operands that are views into NaN buffers (a read outside an operand poisons an output) and
outputs pre-filled with NaN between sentinel guards (a store outside the output breaks a guard;
an element not written stays NaN).

Which case ids launch which kernel:
    gconv_kernel preset 32 (DG_T2)       dg32-*    33 (DG_T2_C16)  dg33-*
                 preset 34 (DG_S2)       dg34-*    35 (DG_S2_C16)  dg35-*
                 preset 36 (DG_S1)       dg36-*  (dg36-*-convq / -convzr: the ConvGRU's two calls)
    gwgrad_kernel<1,2,2,2>               s1-*
    gwgrad_kernel<2,2,2,2>               s2-24-40-*, s2-72-17-*
    gwgrad_kernel<2,2,4,1>               s2-40-16-*, s2-17-9-*
    gwgrad_kernel<2,1,1,1>               s2-16-1-*, s2-16-9-*, s2-16-8-*, s2-8-16-*
    gwgrad_reduce_kernel                 every wgrad case, for dW and for db
    gbias_partial_kernel  nsb = 1        every wgrad case but *-nsb2 (from the large tensor: *-crop7, *-bias-large-*)
                          nsb = 2        s2-16-8-48x48-bias-small-nsb2, s2-16-8-48x48-bias-large-nsb2
    ggates_kernel stage 1 / 2 / 0        gates-stage1-*, gates-stage2-*, gates-stage0-{relu,tanh,none}

Measured on an MI355X (gconv_bwd_elem/<kind>/<case id>), the worst |got - ref| / X per kind
and the case that gave it (informational: the bars above do not depend on them):
    dgrad 32   3.4e-7  dg32-2x128>64-5x40            dgrad 33   2.8e-7  dg33-2x32>16-27x160
    dgrad 34   3.3e-7  dg34-2x64>128-14x23           dgrad 35   2.3e-7  dg35-2x8>16-7x21-split4
    dgrad 36   3.2e-7  dg36-2x128>128-17x39          (tanh cases: 0 beside e)
    wgrad      1.6e-7  s2-72-17-7x3                  dbias      3.7e-8  s2-72-17-7x3
    gates      1.07e-7 = 1.8 * 2^-24  gates-stage2-3x128x5x7/dh  (du_q 1.4, du_z 1.2, du_r 1.4, stage 0 tanh 1.1)
All 117 cases passed on the first run: no kernel changed.

That the cases can fail (_run_dgrad / _run_wgrad take `perturb`, a change of the reference, and
`shrink`, the operand's last row left NaN as if the view were one row short), observed once each:
    the S1 adjoint's reference with taps (0, 0) and (2, 2) of one channel pair swapped: 1319 of
        169728 elements outside, all in output channel 0 (worst ratio 2.0e-3)
    the wgrad reference without the short last K slice (s1-24-16+24-43x3-last-slice-short): 5220
        of 8640 outside, taps ky = 0 and 1 only (the slice's row is the last: ky = 2 reads below it)
    g one row short (dg34-2x64>128-14x23): the 2944 = 128 x 23 elements of the last image's last
        output row NaN;  l0 one row short (s2-24-40-13x18-odd): the 72 = 24 x 3 elements
        dW[:, 39, 1, :] NaN
"""
import pytest
import torch
import torch.nn as nn

import _gconv_bwd_cases as bc
from nlspn_eccv20_amd import _lib
from nlspn_eccv20_amd.gru import pack_adjoint, pack_adjoint_s1

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# ------------------------------------------------------------------ data gradient
def _pack(c, w):
    """The adjoint-packed weights as the model makes them: pack_adjoint of the forward module,
    pack_adjoint_s1 of the stride-1 conv's weight."""
    wd = w.to(DEV)
    if c["mode"] == bc.S1:
        return pack_adjoint_s1(wd)
    if c["mode"] == bc.T2:   # the forward layer is a stride-2 conv cout -> cg
        mod = nn.Conv2d(c["cout"], c["cg"], 3, 2, 1)
    else:                    # a transposed conv cout -> cg
        mod = nn.ConvTranspose2d(c["cout"], c["cg"], 3, 2, 1, 1)
    with torch.no_grad():
        mod.weight = nn.Parameter(wd)
    dg, adj = pack_adjoint(mod)
    assert dg == c["preset"], (c["id"], dg)
    return adj


def _run_dgrad(cid, record, perturb=None, shrink=None):
    c = bc.DG_BY_ID[cid]
    o = bc.dgrad_operands(cid)
    R = bc.dgrad_reference(cid, perturb)
    B, cout, Ho, Wo, split = c["B"], c["cout"], c["Ho"], c["Wo"], c["split"]
    g = bc.guarded(o["g"], DEV, shrink_rows=1 if shrink == "g" else 0)
    wpk = bc.guarded(_pack(c, o["w"]), DEV)
    ysave = bc.guarded(o["ysave"], DEV)
    adds = [None, None]
    if o["add"] is not None:
        adds = [o["add"][:, :split].contiguous(), o["add"][:, split:].contiguous() if split < cout else None]
    alias = c["add"] == "alias"
    b0, dx0 = bc.guarded_out((B, split, Ho, Wo), DEV, fill=adds[0] if alias else None)
    b1, dx1 = bc.guarded_out((B, cout - split, Ho, Wo), DEV, fill=adds[1] if alias else None) if split < cout else (None, None)
    a0, a1 = (dx0, dx1) if alias else (bc.guarded(adds[0], DEV), bc.guarded(adds[1], DEV))
    _lib.call("nlspn_gconv_dgrad", g.device, c["preset"], g, c["cg"], wpk, ysave, a0, a1, dx0, dx1, split, B, c["Hg"], c["Wg"],
              cout, Ho, Wo, c["act"], c["scale"], _lib.STREAM)
    torch.cuda.synchronize()
    assert bc.guards_intact(b0) and (b1 is None or bc.guards_intact(b1)), "a store outside an output (beyond cout or the stored size)"
    got = (dx0 if dx1 is None else torch.cat([dx0, dx1], 1)).cpu()
    bc.check(f"dgrad/{cid}", got, R["ref"], R["X"], R["c"], R["e"], record=record)
    if c["act"] == bc.ACT_RELU:  # at y <= 0 (+0, -0 and negatives): exactly the add, or +0
        off = ~(o["ysave"] > 0)
        want = o["add"][off] if o["add"] is not None else torch.zeros(int(off.sum()))
        assert int(off.sum()) >= len(bc.RELU_PLANTS) and torch.equal(got[off], want)
        assert o["add"] is not None or not bool(torch.signbit(got[off]).any())


DG_IDS = lambda cases: [c["id"] for c in cases]  # noqa: E731


@pytest.mark.parametrize("cid", DG_IDS(bc.DG_A))
def test_dgrad_uneven_last_band_and_empty_tiles(cid, record_metric):
    """a. Every data-gradient preset at the grid whose narrower last band used to overrun the
    window rows in the forward preset of the same geometry, and with an empty last tile."""
    _run_dgrad(cid, record_metric)


@pytest.mark.parametrize("cid", DG_IDS(bc.DG_BAND))
def test_dgrad_band_and_tile_edges(cid, record_metric):
    """a. One full band, one pixel more, 1x1, one row at full band width, 9x2."""
    _run_dgrad(cid, record_metric)


@pytest.mark.parametrize("cid", DG_IDS(bc.DG_SHAPES))
def test_dgrad_cropped_gradient_and_short_output(cid, record_metric):
    """b. Presets 34 / 35: g stored cropped by 0, 1 and 7 rows / columns (the rest reads as
    zeros); presets 32 / 33: the stored output one row and / or one column short."""
    _run_dgrad(cid, record_metric)


@pytest.mark.parametrize("cid", DG_IDS(bc.DG_CHANNELS))
def test_dgrad_channel_edges(cid, record_metric):
    """b. cg = 20 (padded chunks) and cout not a multiple of the output-channel tile (72 on 64,
    8 on 16): nothing stored past cout."""
    _run_dgrad(cid, record_metric)


@pytest.mark.parametrize("cid", DG_IDS(bc.DG_EPI))
def test_dgrad_epilogue(cid, record_metric):
    """c. ReLU on planted +0, -0, the smallest normal and negatives; tanh on +-1 and within a
    few ulps of them at scale 0.1; two outputs split below cout; add0 / add1 as separate tensors
    and aliased to the outputs (the ConvGRU's [z; r] adjoint adds into dh and dx in place)."""
    _run_dgrad(cid, record_metric)


# ------------------------------------------------------------------ weight and bias gradient
def _run_wgrad(cid, record, perturb=None, shrink=None):
    c = bc.GW_BY_ID[cid]
    s, l = bc.wgrad_operands(cid)
    R = bc.wgrad_case_reference(cid, perturb)
    p = bc.gw_plan_of(c)
    B, Cs, c0, c1 = c["B"], c["Cs"], c["c0"], c["c1"]
    need = _lib.get().nlspn_gconv_wgrad_workspace_bytes(c["stride"], Cs, c0 + c1, B, c["Hs"], c["Ws"], c["Hl"], c["Wl"])
    assert need == 4 * p["floats"]
    sd = bc.guarded(s, DEV)
    l0 = bc.guarded(l[:, :c0].contiguous(), DEV, shrink_rows=1 if shrink == "l0" else 0)
    l1 = bc.guarded(l[:, c0:].contiguous(), DEV) if c1 else None
    bw_, dw = bc.guarded_out((Cs, c0 + c1, 3, 3), DEV)
    bb, db = bc.guarded_out((c0 if c["bfl"] else Cs,), DEV)
    bws, ws = bc.guarded_out((need // 4,), DEV)   # exactly the queried bytes
    _lib.call("nlspn_gconv_wgrad", sd.device, c["stride"], sd, Cs, l0, c0, l1, c1, dw, db, int(c["bfl"]), c["scale"], ws, need,
              B, c["Hs"], c["Ws"], c["Hl"], c["Wl"], _lib.STREAM)
    torch.cuda.synchronize()
    assert bc.guards_intact(bw_) and bc.guards_intact(bb), "a store outside dW / db"
    assert bc.guards_intact(bws), "a store outside the queried workspace"
    bc.check(f"wgrad/{cid}", dw.cpu(), R["dw"], R["Xw"], R["cw"], record=record)
    bc.check(f"dbias/{cid}", db.cpu(), R["db"], R["Xb"], R["cb"], record=record)


@pytest.mark.parametrize("cid", [c["id"] for c in bc.GW_CASES])
def test_wgrad_f32_every_tiling(cid, record_metric):
    """d. dW and db of nlspn_gconv_wgrad per element: the four tilings x one pixel, a padded
    k-step, one full band, two and three bands, Hs = 1, the large tensor full, one short and
    cropped by seven, one slice, one unit per slice, a short last slice, the bias from either
    tensor in one and in two slices."""
    _run_wgrad(cid, record_metric)


# ------------------------------------------------------------------ gate derivatives
def _run_gates(cid, record):
    c = bc.GATE_BY_ID[cid]
    o = bc.gate_operands(cid)
    want = bc.gate_formulas(cid, torch.float64)
    d = {k: bc.guarded(v, DEV) for k, v in o.items()}
    B, hc, H, W, stage = c["B"], c["hc"], c["H"], c["W"], c["stage"]
    shape = (B, hc, H, W)
    outs = {}
    if stage == 0:
        outs["duq"] = bc.guarded_out(shape, DEV)
        args = (d["dhn"], d["z"], None, None, None, None, outs["duq"][1], None, None)
    elif stage == 1:
        outs["duq"], outs["duzr"] = bc.guarded_out(shape, DEV), bc.guarded_out((B, 2 * hc, H, W), DEV)
        args = (d["dhn"], d["z"], None, d["q"], d["h"], None, outs["duq"][1], outs["duzr"][1], None)
    else:
        # as _GruFn.backward: stage 1 writes the [du_z] half of the NaN-filled duzr, stage 2 the rest
        outs["duq"], outs["duzr"], outs["dh"] = bc.guarded_out(shape, DEV), bc.guarded_out((B, 2 * hc, H, W), DEV), bc.guarded_out(shape, DEV)
        _lib.call("nlspn_gconv_gru_gates_backward", torch.device(DEV), 1, d["dhn"], d["z"], None, d["q"], d["h"], None,
                  outs["duq"][1], outs["duzr"][1], None, c["act"], B, hc, H, W, _lib.STREAM)
        want.update(bc.gate_formulas(cid, torch.float64, stage=1))
        args = (d["dhn"], d["z"], d["r"], None, d["h"], d["drh"], None, outs["duzr"][1], outs["dh"][1])
    _lib.call("nlspn_gconv_gru_gates_backward", torch.device(DEV), stage, *args, c["act"], B, hc, H, W, _lib.STREAM)
    torch.cuda.synchronize()
    assert all(bc.guards_intact(b) for b, _ in outs.values()), "a store outside an output"
    got = {k: v.cpu() for k, (_, v) in outs.items()}
    if stage == 1:   # only the [du_z] half of duzr is written
        assert bool(torch.isnan(got["duzr"][:, hc:]).all())
        got["duz"] = got.pop("duzr")[:, :hc]
    elif stage == 2:  # all of it
        duzr = got.pop("duzr")
        got["duz"], got["dur"] = duzr[:, :hc], duzr[:, hc:]
    assert set(got) == set(want)
    for k, (ref, X) in want.items():
        bc.check(f"gates/{cid}/{k}", got[k], ref, X, bc.C_GATES, record=record)
    if stage == 0 and c["act"] != bc.ACT_TANH:  # the kinks are exact: g, or +0 at y <= 0
        assert torch.equal(got["duq"], want["duq"][0].float())
        if c["act"] == bc.ACT_RELU:
            assert not bool(torch.signbit(got["duq"][~(o["z"] > 0)]).any())


@pytest.mark.parametrize("cid", [c["id"] for c in bc.GATE_CASES])
def test_gate_derivatives(cid, record_metric):
    """e. Stages 1 and 2 at B = 3, hc = 128, 5x7 (n no multiple of 256; b > 0: the e + b chw index
    into the (B, 2 hc, H, W) tensor) with exact 0 / 1 gates, q = +-1, q = h and r = 1/2 planted; stage 0
    as GruConvs._act_backward calls it."""
    _run_gates(cid, record_metric)
