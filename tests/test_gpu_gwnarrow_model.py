"""GPU: NLSPNModel.gru_wgrad_narrow / GruConvs.wgrad_narrow, the streaming weight gradient of the
narrow layers (csrc/nlspn_gwnarrow.h) wired through the native training path.  Hidden width 128,
B=2, 50x70, T=3, the section of tests/test_gpu_gconv_bwd.py (its _model, seeds and inputs).

The covered layers are encode_dep's first conv (1 -> 16), encode_aff's first conv (9 -> 16) and
decode_aff's last transposed conv (16 -> 8, bias gradient from the large side, output cropped
56x72 -> 50x70).
 1. Each covered layer alone against the torch module in float64 on the CPU: dW and db within the
    project's gradient bar (relative L2 <= 1e-4); asserted, as tests/test_gpu_gconv_bwd.py does,
    about 4x the largest error measured on an MI355X, rounded up to one digit:
        small_dep     dW 1.44e-7   db 1.48e-7   -> 6e-7   (switch off: 1.73e-7, 1.07e-7)
        small_aff     dW 1.23e-7   db 1.25e-7   -> 5e-7   (switch off: 1.66e-7, 9.8e-8)
        t2_last_crop  dW 1.43e-7   db 1.19e-7   -> 6e-7   (switch off: 1.68e-7, 1.12e-7)
    dx and the output are the switch-off run's bits, and dW / db are the same bits under
    wgrad_precision "fp32" and "bf16x3" (the two switches are apart).
 2. encode_dep, encode_aff, the ConvGRU cell and decode_aff composed under one fixed upstream
    gradient (the chain of test_backward_is_bit_reproducible: every native backward kernel, and
    no float atomics): with the switch on, the output, both input gradients and every parameter
    gradient of the wide layers and the ConvGRU are the switch-off run's bits; only the six
    tensors of the covered layers differ; the launch counts move from "wgrad" to "wgrad_narrow".
 3. propagate_heads under gradients through NLSPNModel: pred and every pred_inter are bit-equal
    (the forward does not change), stats["wgrad_narrow"] > 0 and stats["wgrad"] drops by the
    covered calls' launches; off, nothing is counted under "wgrad_narrow".  The gradients of
    this section are compared by relative L2 <= 1e-5 (the bar of
    test_native_gru_train_off_keeps_the_module_path for "only the summation order may differ"),
    not bit for bit: the propagation backward ahead of these layers scatters with float atomics,
    so the section does not reproduce its own last bits from run to run with the switch off
    either (tests/test_gpu_gconv_bwd.py, test_backward_is_bit_reproducible).  Measured: none of the
    28 gradient tensors is bit-equal between the two runs, the worst relative L2 is 3.8e-7
    ("fp32") and 1.0e-6 ("bf16x3").
 4. At inference and with native_gru_train = False the switch launches nothing.
"""
import copy
import functools

import pytest
import torch

from nlspn_eccv20_amd.gru import ACT_NONE, ACT_RELU, GruConvs
from test_gpu_gconv_bwd import DEV, SUBS, T, _act, _half, _model, _rel, _section_inputs

pytestmark = pytest.mark.gpu
B, H, W = 2, 50, 70
CAP = 1e-4
BARS = {"small_dep": 6e-7, "small_aff": 5e-7, "t2_last_crop": 6e-7}  # ~4x the measured error (module docstring)
assert max(BARS.values()) <= CAP
# kind -> (module picker, activation, input size, in_div, crop)
LAYERS = {
    "small_dep": (lambda m: m.encode_dep[0][0], ACT_RELU, (H, W), 10.0, None),
    "small_aff": (lambda m: m.encode_aff[0][0], ACT_RELU, (H, W), 1.0, None),
    "t2_last_crop": (lambda m: m.decode_aff[2][0], ACT_NONE, (_half(H, 3) * 4, _half(W, 3) * 4), 1.0, (H, W)),
}
COVERED = ("encode_dep.0.0.", "encode_aff.0.0.", "decode_aff.2.0.")


@pytest.mark.parametrize("kind", list(LAYERS))
def test_covered_layer_matches_float64_and_the_rest_is_unchanged(kind, record_metric):
    pick, act, (hi, wi), in_div, crop = LAYERS[kind]
    m = _model(H, W, seed=1)
    conv = pick(m)
    g = torch.Generator(device="cpu").manual_seed(7)
    x = torch.randn((B, conv.in_channels, hi, wi), generator=g, dtype=torch.float64) * (5.0 if in_div != 1.0 else 1.0)
    ref = copy.deepcopy(conv).double().cpu()
    xr = x.clone().requires_grad_(True)
    yr = _act(ref(xr / in_div if in_div != 1.0 else xr), act)
    if crop:
        yr = yr[:, :, :crop[0], :crop[1]]
    up_g = torch.randn(yr.shape, generator=g, dtype=torch.float64)
    (yr * up_g).sum().backward()
    got = {}
    for narrow, prec in ((False, "fp32"), (True, "fp32"), (True, "bf16x3")):
        gc = GruConvs()
        gc.wgrad_narrow, gc.wgrad_precision = narrow, prec
        xn = x.float().to(DEV).requires_grad_(True)
        for p in conv.parameters():
            p.grad = None
        y = gc.layer(conv, xn, act=act, in_div=in_div, crop=crop)
        (y * up_g.float().to(DEV)).sum().backward()
        got[narrow, prec] = (y.detach(), xn.grad.clone(), conv.weight.grad.clone(), conv.bias.grad.clone(), dict(gc.stats))
    off, on, on3 = got[False, "fp32"], got[True, "fp32"], got[True, "bf16x3"]
    assert off[4]["wgrad"] == 4 and off[4]["wgrad_narrow"] == 0
    for r in (on, on3):
        assert r[4]["wgrad_narrow"] == 2 and r[4]["wgrad"] == 0 and r[4]["wgrad_x3"] == 0, r[4]
        assert torch.equal(r[0], off[0]) and torch.equal(r[1], off[1]), "the output and dx do not pass through the new kernel"
    assert torch.equal(on[2], on3[2]) and torch.equal(on[3], on3[3]), "the covered layers do not depend on wgrad_precision"
    ew, eb = _rel(on[2], ref.weight.grad), _rel(on[3], ref.bias.grad)
    ew0, eb0 = _rel(off[2], ref.weight.grad), _rel(off[3], ref.bias.grad)
    record_metric(f"gwnarrow_model/{kind}/dW", ew)
    record_metric(f"gwnarrow_model/{kind}/db", eb)
    print(kind, "dW rel L2", ew, "db", eb, "(switch off:", ew0, eb0, ")")
    assert ew <= BARS[kind] and eb <= BARS[kind], (kind, ew, eb)


@functools.lru_cache(maxsize=None)
def _chain(narrow, precision="fp32"):
    m = _model(H, W, seed=5)
    gc = GruConvs()
    gc.wgrad_narrow, gc.wgrad_precision = narrow, precision
    g = torch.Generator(device=DEV).manual_seed(12)
    new_pred = torch.rand((B, 1, H, W), device=DEV, generator=g) * 10
    aff = torch.rand((B, 9, H, W), device=DEV, generator=g)
    up_g = torch.randn((B, 8, H, W), device=DEV, generator=g)
    ins = [new_pred.clone().requires_grad_(True), aff.clone().requires_grad_(True)]
    P = gc.pack(m)
    h = gc.gru(P, gc.encode_aff(P, ins[1]), gc.encode_dep(P, ins[0], m.args.max_depth))
    y = gc.decode_aff(P, h, (H, W))
    (y * up_g).sum().backward()
    out = {f"{s}.{n}": p.grad.clone() for s in SUBS for n, p in getattr(m, s).named_parameters()}
    out.update(new_pred=ins[0].grad.clone(), aff=ins[1].grad.clone(), y=y.detach().clone())
    return out, dict(gc.stats)


def test_chain_only_the_covered_layers_gradients_change():
    (off, soff), (on, son), (on3, son3) = _chain(False), _chain(True), _chain(True, "bf16x3")
    covered = [k for k in off if k.startswith(COVERED)]
    assert len(covered) == 6 and len(off) == 27
    for k in off:
        if k in covered:
            assert _rel(on[k], off[k]) <= 1e-5, (k, _rel(on[k], off[k]))
            assert torch.equal(on[k], on3[k]), k
        else:
            assert torch.equal(on[k], off[k]), k
    assert soff["wgrad_narrow"] == 0 and son["wgrad_narrow"] == 2 * 3 and soff["wgrad"] - son["wgrad"] == 4 * 3
    assert son3["wgrad_narrow"] == 6 and son3["wgrad"] == 0 and son3["wgrad_x3"] == soff["wgrad"] - 12
    assert {k: v for k, v in son.items() if not k.startswith("wgrad")} == {k: v for k, v in soff.items() if not k.startswith("wgrad")}
    (off2, soff2) = _chain.__wrapped__(False)   # off: the f32 entry alone, and its own bits again
    assert soff2 == soff and all(torch.equal(off[k], off2[k]) for k in off)


@functools.lru_cache(maxsize=None)
def _section(narrow, mode="native", precision="fp32"):
    m = _model(H, W, seed=5)
    pred_init, off_aff, conf, dep, proj = _section_inputs(B, H, W)
    m.native_gru_train = mode != "train_off"
    m.gru_wgrad_precision = precision
    m.gru_wgrad_narrow = narrow
    assert m._gru_convs.wgrad_narrow is narrow
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
    grads.update({n: t.grad.clone() for n, t in zip(("pred_init", "off_aff", "confidence"), ins)})
    return {"pred_inter": [p.detach().clone() for p in o["pred_inter"]], "pred": o["pred"].detach().clone(),
            "grads": grads, "stats": dict(m._gru_convs.stats)}


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_section_through_the_model(precision, record_metric):
    a, r = _section(True, "native", precision), _section(False, "native", precision)
    for p, q in zip(a["pred_inter"] + [a["pred"]], r["pred_inter"] + [r["pred"]]):
        assert torch.equal(p, q)
    assert r["stats"]["wgrad_narrow"] == 0 and a["stats"]["wgrad_narrow"] > 0
    # a covered call: four launches of the f32 entry ("bf16x3" forwards these shapes to it) become two
    assert r["stats"]["wgrad"] + r["stats"]["wgrad_x3"] - a["stats"]["wgrad"] - a["stats"]["wgrad_x3"] == 2 * a["stats"]["wgrad_narrow"]
    if precision == "fp32":
        assert a["stats"]["wgrad"] == r["stats"]["wgrad"] - 2 * a["stats"]["wgrad_narrow"] and a["stats"]["wgrad_x3"] == 0
    # T - 1 passes of encode_dep and decode_aff, one of encode_aff
    assert a["stats"]["wgrad_narrow"] == 2 * (2 * (T - 1) + 1)
    assert {k: v for k, v in a["stats"].items() if not k.startswith("wgrad")} == {k: v for k, v in r["stats"].items() if not k.startswith("wgrad")}
    errs = {k: _rel(a["grads"][k], r["grads"][k]) for k in r["grads"]}
    same = sum(torch.equal(a["grads"][k], r["grads"][k]) for k in r["grads"])
    print(f"section narrow vs off ({precision}): {same} of {len(errs)} tensors bit-equal; worst", max(errs.values()))
    record_metric(f"gwnarrow_model/section/{precision}/worst_rel_l2", max(errs.values()))
    for k, e in errs.items():
        assert float(r["grads"][k].abs().max()) > 0 and e <= 1e-5, (k, e)


@pytest.mark.parametrize("mode", ["train_off", "nograd"])
def test_switch_launches_nothing_outside_the_native_training_path(mode):
    s, r = _section(True, mode), _section(False, mode)
    assert s["stats"]["wgrad_narrow"] == 0 and s["stats"]["wgrad"] == 0 and s["stats"] == r["stats"], s["stats"]
    if mode == "nograd":
        assert torch.equal(s["pred"], r["pred"])
