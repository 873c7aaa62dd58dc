"""GPU: the split-bf16 data gradients through autograd (GruConvs.dgrad_precision /
NLSPNModel.gru_dgrad_precision = "bf16x3"; nlspn_gconv_x3_dgrad, csrc/nlspn_gconv_x3.h).  Model
and shapes are those of tests/test_gpu_gwgrad16.py: hc = 128, (B, H, W) in {(2, 50, 70),
(1, 24, 320)}, T = 3.

1. Each wide layer kind and the ConvGRU cell with dgrad_precision = "bf16x3": dx (and dh) against
   the torch module in float64 on the CPU, relative L2 <= L2_BAR = min(4 x measured, 1e-4), 1e-4
   being the project's gradient bar; the "fp32" mode's value is recorded beside it.  The forward,
   dW's launches and db are the "fp32" mode's (dW and db of a single layer: its bits, since their
   inputs do not come from a data gradient).
2. The GRU-mode section under gradients: forward bit-equal to the "fp32" mode, every parameter
   and input gradient within 1e-3 relative L2 of it (BAR_SECTION of tests/test_gpu_gwgrad16.py),
   also with gru_wgrad_precision = "bf16x3" and gru_wgrad_narrow = True on top;
   stats["dgrad_x3"] counts the covered data gradients (per update: two of encode_dep, two of the
   ConvGRU, one of decode_aff; once: two of encode_aff) and stats["dgrad"] the rest (per update
   encode_dep's chain-end ReLU launch, the 16 -> 1 and 8 -> 16 adjoints and the 2hc -> 16 decoder
   layer's, which measured slower on the new entry; once encode_aff's Tanh launch and its 16 -> 9
   adjoint).
3. "fp32" set explicitly and left at the default: bit-equal gradients, stats["dgrad_x3"] == 0
   (on the composed backward; the section's gradients differ in the last bits from run to run on
   either path, the propagation backward's scatter using float atomics).
4. The switch launches nothing with native_gru_train = False or under no_grad.
5. Bad values raise ValueError on the model property and on GruConvs.
6. Two backward runs give identical bits.

Measured on an MI355X (gru_x3_dgrad/...), relative L2 against float64, "bf16x3" | "fp32" mode:
    s2_relu (16 -> 2hc)   dx 4.40e-6 .. 4.42e-6 | 3.3e-7        s2_tanh (2hc -> hc)  dx 4.41e-6 .. 4.54e-6 | 6.9e-7
    t2_relu (hc -> 2hc)   dx 4.50e-6 .. 4.53e-6 | 5.9e-7        t2_c16_relu (2hc -> 16): the f32 entry, 1.5e-7
    cell   dh 1.55e-6 .. 1.63e-6 | 3.4e-7   dx 4.40e-6 .. 4.45e-6 | 7.1e-7   convr.weight 4.36e-6 .. 4.45e-6,
           convr.bias 4.02e-6 .. 4.84e-6 (they read d(r h), convq's adjoint) | 6.8e-7; convz / convq: the "fp32" bits
    (4.4e-6 is the split itself: a term is off by up to 2^-15, the weight gradient's "bf16x3" mode measures the same)
    section vs the "fp32" mode: largest 9.6e-6 (encode_dep.0.0.weight), with the weight gradients' switches too 9.6e-6
"""
import copy
import functools

import pytest
import torch

from nlspn_eccv20_amd.gru import GruConvs
from test_gpu_gwgrad16 import BAR_SECTION, DEV, LAYERS, SHAPES, SUBS, T, _act, _half, _model, _rel

pytestmark = pytest.mark.gpu
L2_CAP = 1e-4          # the project's gradient bar
L2_MEASURED = 4.84e-6  # the largest relative L2 measured on an MI355X (the cell's convr.bias at 1x24x320)
L2_BAR = min(4 * L2_MEASURED, L2_CAP)
# the 2hc -> 16 decoder layer's adjoint (a 16-channel gradient) measured slower than the f32 entry
# and stays there (nlspn_gconv_x3_dgrad_covers = 0): its dx is the "fp32" mode's bits
COVERED = {"s2_relu": True, "s2_tanh": True, "t2_relu": True, "t2_c16_relu": False}


# ------------------------------------------------------------------ layers and cell
@pytest.mark.parametrize("B,H,W", SHAPES)
@pytest.mark.parametrize("kind", list(LAYERS))
def test_layer_dx_matches_float64(kind, B, H, W, record_metric):
    """1a. dx of each wide layer kind in "bf16x3" against the float64 CPU module."""
    pick, act, scale = LAYERS[kind]
    m = _model(H, W, seed=1)
    conv = pick(m)
    if scale >= 0:
        hi, wi = _half(H, scale), _half(W, scale)
    else:
        up = 3 + scale
        hi, wi = _half(H, 3) * 2 ** up, _half(W, 3) * 2 ** up
    g = torch.Generator(device="cpu").manual_seed(7)
    x = torch.randn((B, conv.in_channels, hi, wi), generator=g, dtype=torch.float64)
    ref = copy.deepcopy(conv).double().cpu()
    xr = x.clone().requires_grad_(True)
    yr = _act(ref(xr), act)
    up_g = torch.randn(yr.shape, generator=g, dtype=torch.float64)
    (yr * up_g).sum().backward()
    got = {}
    for mode in ("fp32", "bf16x3"):
        gc = GruConvs()
        gc.dgrad_precision = mode
        xn = x.float().to(DEV).requires_grad_(True)
        for p in conv.parameters():
            p.grad = None
        y = gc.layer(conv, xn, act=act, in_div=1.0, crop=None)
        (y * up_g.float().to(DEV)).sum().backward()
        got[mode] = (y.detach(), xn.grad.clone(), conv.weight.grad.clone(), conv.bias.grad.clone(), dict(gc.stats))
    # (the activation's launch is the f32 one in both modes; the gradient then enters in f32: one split)
    n = int(COVERED[kind])
    assert got["bf16x3"][4]["dgrad_x3"] == n and got["bf16x3"][4]["dgrad"] == 2 - n and got["bf16x3"][4]["split_x3"] == n
    assert got["fp32"][4]["dgrad_x3"] == 0 and got["fp32"][4]["dgrad"] == 2 and got["fp32"][4]["split_x3"] == 0
    assert torch.equal(got["fp32"][0], got["bf16x3"][0])
    assert torch.equal(got["fp32"][2], got["bf16x3"][2]) and torch.equal(got["fp32"][3], got["bf16x3"][3])
    assert torch.equal(got["fp32"][1], got["bf16x3"][1]) != COVERED[kind], "the new kernel ran exactly where it covers"
    e, e32 = _rel(got["bf16x3"][1], xr.grad), _rel(got["fp32"][1], xr.grad)
    record_metric(f"gru_x3_dgrad/{kind}/{B}x{H}x{W}/dx", e)
    record_metric(f"gru_x3_dgrad/{kind}/{B}x{H}x{W}/dx_f32", e32)
    print(kind, (B, H, W), "dx rel L2", e, "f32 mode", e32)
    assert e <= L2_BAR, (kind, e, L2_BAR)


def _cell(m, B, H, W, mode):
    hh, ww = _half(H, 3), _half(W, 3)
    g = torch.Generator(device="cpu").manual_seed(8)
    h0 = torch.tanh(torch.randn((B, 128, hh, ww), generator=g, dtype=torch.float64))
    x0 = torch.relu(torch.randn((B, 128, hh, ww), generator=g, dtype=torch.float64))
    up_g = torch.randn((B, 128, hh, ww), generator=g, dtype=torch.float64)

    def run(gru, h, x):
        h, x = h.clone().requires_grad_(True), x.clone().requires_grad_(True)
        for p in gru.parameters():
            p.grad = None
        stats = None
        if mode is None:
            y = gru(h=h, x=x)
        else:
            gc = GruConvs()
            gc.dgrad_precision = mode
            y = gc.gru(gc.pack(m), h, x)
            stats = gc.stats
        (y * up_g.to(y)).sum().backward()
        out = {"dh": h.grad.clone(), "dx": x.grad.clone()}
        out.update({n: p.grad.clone() for n, p in gru.named_parameters()})
        return out, stats

    if mode is None:
        return run(copy.deepcopy(m.GRU).double().cpu(), h0, x0)
    return run(m.GRU, h0.float().to(DEV), x0.float().to(DEV))


@pytest.mark.parametrize("B,H,W", SHAPES)
def test_convgru_cell_dh_dx_match_float64(B, H, W, record_metric):
    """1b. The ConvGRU cell: dh and dx (both adjoints on the new entry) against float64; the
    weight gradients that read a data gradient (convz / convr: their d(r h) comes from convq's
    adjoint) stay under the bar too; convq's dW and db do not pass through the new kernel."""
    m = _model(H, W, seed=2)
    (want, _), (f32, s32), (x3, sx3) = _cell(m, B, H, W, None), _cell(m, B, H, W, "fp32"), _cell(m, B, H, W, "bf16x3")
    assert sx3["dgrad_x3"] == 2 and sx3["dgrad"] == 0 and sx3["split_x3"] == 2 and sx3["gates_bwd"] == 2
    assert s32["dgrad_x3"] == 0 and s32["dgrad"] == 2 and s32["split_x3"] == 0
    assert len(want) == 8
    for k in want:
        e, e32 = _rel(x3[k], want[k]), _rel(f32[k], want[k])
        record_metric(f"gru_x3_dgrad/gru/{B}x{H}x{W}/{k}", e)
        record_metric(f"gru_x3_dgrad/gru/{B}x{H}x{W}/{k}_f32", e32)
        print("gru", (B, H, W), k, "rel L2", e, "f32 mode", e32)
        assert e <= L2_BAR, (k, e, L2_BAR)
        if k.startswith("convq"):
            assert torch.equal(x3[k], f32[k]), k
    assert not torch.equal(x3["dh"], f32["dh"]) and not torch.equal(x3["dx"], f32["dx"]), "the new kernel ran"


def _composed(m, B, H, W, mode):
    """encode_dep, encode_aff, the ConvGRU cell and decode_aff composed from one fixed upstream
    gradient, as test_backward_is_bit_reproducible of tests/test_gpu_gconv_bwd.py composes them
    (inside the section the propagation's own backward precedes them, and its scatter uses float
    atomics: there the last bits differ from run to run on either path).  mode None: the switch
    left at its default.  Every parameter and input gradient, and the launch counts."""
    gc = GruConvs()
    if mode is not None:
        gc.dgrad_precision = mode
    g = torch.Generator(device=DEV).manual_seed(12)
    new_pred = torch.rand((B, 1, H, W), device=DEV, generator=g) * 10
    aff = torch.rand((B, 9, H, W), device=DEV, generator=g)
    up_g = torch.randn((B, 8, H, W), device=DEV, generator=g)
    ins = [new_pred.requires_grad_(True), aff.requires_grad_(True)]
    for p in m.parameters():
        p.grad = None
    P = gc.pack(m)
    h = gc.gru(P, gc.encode_aff(P, ins[1]), gc.encode_dep(P, ins[0], m.args.max_depth))
    (gc.decode_aff(P, h, (H, W)) * up_g).sum().backward()
    out = {f"{s}.{n}": p.grad.clone() for s in SUBS for n, p in getattr(m, s).named_parameters()}
    out.update(new_pred=ins[0].grad.clone(), aff=ins[1].grad.clone())
    return out, dict(gc.stats)


def test_two_backward_runs_give_identical_bits():
    """6. The cell alone and every native backward kernel composed, twice each.  In a chain the
    gradient is split once where it enters in f32 and handed on as c8x2 from then on: per encoder
    two new launches and one split, the ConvGRU two and two, decode_aff one and one; the f32 entry
    keeps the chain-end activations of the encoders, the 16 -> 1, 16 -> 9 and 8 -> 16 adjoints and
    the 2hc -> 16 decoder layer's."""
    B, H, W = SHAPES[0]
    m = _model(H, W, seed=2)
    a, b = _cell(m, B, H, W, "bf16x3")[0], _cell(m, B, H, W, "bf16x3")[0]
    assert all(torch.equal(a[k], b[k]) for k in a), [k for k in a if not torch.equal(a[k], b[k])]
    (r, sr), (s, _) = _composed(m, B, H, W, "bf16x3"), _composed(m, B, H, W, "bf16x3")
    assert sr["dgrad_x3"] == 7 and sr["dgrad"] == 6 and sr["split_x3"] == 5 and sr["gates_bwd"] == 2, sr
    assert len(r) == 26 and all(float(v.abs().max()) > 0 and bool(torch.isfinite(v).all()) for v in r.values())
    assert all(torch.equal(r[k], s[k]) for k in r), [k for k in r if not torch.equal(r[k], s[k])]


def test_fp32_set_explicitly_is_the_default_bit_for_bit():
    """3. On the composed backward (reproducible run to run): "fp32" set explicitly and the switch
    left alone give the same bits and launch nothing new; "bf16x3" gives other bits within the
    section bar."""
    B, H, W = SHAPES[0]
    m = _model(H, W, seed=2)
    (a, sa), (r, sr), (x, _) = _composed(m, B, H, W, "fp32"), _composed(m, B, H, W, None), _composed(m, B, H, W, "bf16x3")
    assert sa == sr and sa["dgrad_x3"] == 0 and sa["split_x3"] == 0 and sa["dgrad"] == 13, sa
    assert all(torch.equal(a[k], r[k]) for k in r), [k for k in r if not torch.equal(a[k], r[k])]
    assert any(not torch.equal(x[k], r[k]) for k in r)
    assert all(_rel(x[k], r[k]) <= BAR_SECTION for k in r), {k: _rel(x[k], r[k]) for k in r}


# ------------------------------------------------------------------ the section
@functools.lru_cache(maxsize=None)
def _section(dgrad, wgrad, narrow, mode):
    B, H, W = 1, 50, 70
    m = _model(H, W, seed=5)
    g = torch.Generator(device=DEV).manual_seed(9)
    pred_init = torch.rand((B, 1, H, W), device=DEV, generator=g) * 10
    dep = pred_init * (torch.rand((B, 1, H, W), device=DEV, generator=g) < 0.02)
    off_aff = torch.randn((B, 24, H, W), device=DEV, generator=g)
    conf = torch.rand((B, 1, H, W), device=DEV, generator=g)
    proj = [torch.randn((B, 1, H, W), device=DEV, generator=g) for _ in range(T + 1)]
    m.native_gru_train = mode != "train_off"
    m.gru_dgrad_precision = dgrad
    m.gru_wgrad_precision = wgrad
    m.gru_wgrad_narrow = narrow
    assert m._gru_convs.dgrad_precision == dgrad
    m._gru_convs.reset_stats()
    if mode == "nograd":
        with torch.no_grad():
            o = m.propagate_heads(pred_init, off_aff, conf, dep)
        return {"pred": o["pred"].clone(), "stats": dict(m._gru_convs.stats)}
    ins = [t.clone().requires_grad_(True) for t in (pred_init, off_aff, conf)]
    o = m.propagate_heads(*ins, dep)
    loss = (o["pred"] * proj[T]).sum() + sum((p * q).sum() for p, q in zip(o["pred_inter"], proj))
    loss.backward()
    grads = {f"{s}.{n}": p.grad.clone() for s in SUBS for n, p in getattr(m, s).named_parameters()}
    grads["aff_scale_const"] = m.aff_scale_const.grad.clone()
    return {"pred_inter": [p.detach().clone() for p in o["pred_inter"]], "pred": o["pred"].detach().clone(),
            "grads": grads, "dins": [t.grad.clone() for t in ins], "stats": dict(m._gru_convs.stats)}


@pytest.mark.parametrize("wgrad,narrow", [("fp32", False), ("bf16x3", True)])
def test_section_bf16x3_against_fp32(wgrad, narrow, record_metric):
    """2. hc = 128, B = 1, 50 x 70, T = 3, native_gru_train; the second case with the weight
    gradients' two switches on top."""
    a, r = _section("bf16x3", wgrad, narrow, "native"), _section("fp32", "fp32", False, "native")
    for p, q in zip(a["pred_inter"] + [a["pred"]], r["pred_inter"] + [r["pred"]]):
        assert torch.equal(p, q)
    U = a["stats"]["gru_fwd"]
    assert U >= 1 and r["stats"]["gru_fwd"] == U
    print("section stats", a["stats"], "fp32", r["stats"])
    assert a["stats"]["dgrad_x3"] == 5 * U + 2, a["stats"]
    assert a["stats"]["dgrad"] == 4 * U + 2, a["stats"]
    assert a["stats"]["split_x3"] == 4 * U + 1, a["stats"]
    assert r["stats"]["dgrad_x3"] == 0 and r["stats"]["split_x3"] == 0
    assert r["stats"]["dgrad"] == a["stats"]["dgrad"] + a["stats"]["dgrad_x3"]
    assert a["stats"]["gates_bwd"] == r["stats"]["gates_bwd"] == 2 * U
    assert len(a["grads"]) >= 6 * 3 + 6 + 1
    errs = {k: _rel(a["grads"][k], r["grads"][k]) for k in r["grads"]}
    errs.update({f"input{i}": _rel(p, q) for i, (p, q) in enumerate(zip(a["dins"], r["dins"]))})
    for k, e in errs.items():
        record_metric(f"gru_x3_dgrad/section/{wgrad}/{k}", e)
    print("section dgrad bf16x3 (wgrad", wgrad, "narrow", narrow, ") vs fp32:", errs)
    for k, e in errs.items():
        assert e <= BAR_SECTION, (k, e)
    assert any(not torch.equal(a["grads"][k], r["grads"][k]) for k in r["grads"]), "the new kernels ran"


@pytest.mark.parametrize("mode", ["train_off", "nograd"])
def test_switch_launches_nothing_outside_the_native_training_path(mode):
    """4. native_gru_train = False, or no_grad: "bf16x3" is ignored."""
    s = _section("bf16x3", "fp32", False, mode)
    assert s["stats"]["dgrad_x3"] == 0 and s["stats"]["split_x3"] == 0 and s["stats"]["dgrad"] == 0, s["stats"]


def test_bad_values_raise():
    """5."""
    m = _model(32, 32)
    assert m.gru_dgrad_precision == "fp32"
    for bad in ("bf16", "fp16", None, True):
        with pytest.raises(ValueError, match="gru_dgrad_precision"):
            m.gru_dgrad_precision = bad
    assert m.gru_dgrad_precision == "fp32"
    m.gru_dgrad_precision = "bf16x3"
    assert m._gru_convs.dgrad_precision == "bf16x3"
    gc = GruConvs()
    gc.dgrad_precision = "bf16"
    conv = m.encode_dep[1][0]
    x = torch.randn((1, conv.in_channels, 8, 8), device=DEV, requires_grad=True)
    y = gc.layer(conv, x)
    with pytest.raises(ValueError, match="dgrad_precision"):
        y.sum().backward()
