"""GPU: the native backward of the GRU-mode convolutions (nlspn_eccv20_amd/gru.py,
csrc/nlspn_gconv_bwd.h): data, weight and bias gradients of every layer kind and of the
ConvGRU cell against the torch modules in float64 on the CPU, and the whole GRU-mode section
under gradients against the module path.

Bars.  Both sides form exact f32 products with f32 accumulation; only the summation order
differs.  Per layer and for the cell the cap is the project's gradient bar, relative L2 <=
1e-4 (README, parity paragraph); the MIOpen fp32 modules' error against the same float64
reference is recorded beside the native one (record_metric).  Under that cap each asserted
bar is about 4x the largest native error measured on an MI355X (worst of dx / dW / db over both
shapes; the MIOpen module's own error against the same reference in brackets), rounded up to
one digit:
    s2_relu       3.4e-7 [2.1e-7] -> 2e-6      t2_relu       5.9e-7 [3.0e-7] -> 3e-6
    s2_tanh       6.9e-7 [4.1e-7] -> 3e-6      t2_c16_relu   1.5e-7 [2.5e-7] -> 7e-7
    small_dep     2.0e-7 [2.0e-7] -> 9e-7      t2_last_crop  1.8e-7 [5.6e-7] -> 8e-7
    small_aff     1.7e-7 [4.0e-7] -> 7e-7      ConvGRU cell  7.1e-7 [4.1e-7] -> 3e-6
The section (measured 1.4e-6 at worst, aff_scale_const) uses the bar
tests/test_backward_golden.py::test_gru_offset_matches_reference uses for GRU-mode gradients,
1e-3 relative L2.

Shapes (hidden width 128, the smallest supported): B=2 50x70 (every scale odd somewhere:
25x35, 13x18, 7x9; decode_aff crops 56x72 -> 50x70; two column bands in the stride-2 layers)
and B=1 24x320 (a 3x40 1/8-scale grid: two column bands and tiles spanning several rows in
the stride-1 kernels); B=1 136x312, whose adjoint grids 34x78 and 17x39 split into uneven
column bands (12 | 11 ... and 20 | 19): the narrower last band's tiles span one row more, which
the planner once did not size the LDS window for (csrc/nlspn_gconv_plan.h gc_tile,
tests/test_gconv_plan_cpu.py) — the data-gradient presets share the forward body and planner.
The bars are unchanged by that shape."""
import copy
import functools
import types

import pytest
import torch

from nlspn_eccv20_amd import NLSPNModel
from nlspn_eccv20_amd.gru import ACT_NONE, ACT_RELU, ACT_TANH, GruConvs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(2, 50, 70), (1, 24, 320), (1, 136, 312)]
CAP = 1e-4          # per layer / cell: the project's gradient bar, relative L2 against float64
BARS = {"s2_relu": 2e-6, "s2_tanh": 3e-6, "small_dep": 9e-7, "small_aff": 7e-7, "t2_relu": 3e-6, "t2_c16_relu": 7e-7,
        "t2_last_crop": 8e-7, "gru": 3e-6}  # ~4x the measured native error (module docstring), all under CAP
assert max(BARS.values()) <= CAP
BAR_SECTION = 1e-3  # section: native path against the module path
T = 3


def _model(H, W, seed=0, hc=128):
    args = types.SimpleNamespace(prop_kernel=3, affinity="TGASS", affinity_gamma=0.5, prop_time=T,
                                 preserve_input=True, always_clip=False, conf_prop=True, offset=True,
                                 network="resnet34", from_scratch=True, zero_init_aff=False, use_GRU=True,
                                 use_S2D=False, GRU_hidden_dim=hc, GRU_input_dim=hc, lr=1e-3, max_depth=10.0,
                                 patch_height=H, patch_width=W, model_name="NLSPN")
    torch.manual_seed(seed)
    m = NLSPNModel(args).to(DEV).eval()
    with torch.no_grad():  # weights and biases of a trained scale
        for mod in (m.encode_dep, m.encode_aff, m.GRU, m.decode_aff):
            for p in mod.parameters():
                p.add_(0.02 * torch.randn_like(p))
    return m


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def _half(n, k):  # the size after k stride-2 convs
    for _ in range(k):
        n = (n - 1) // 2 + 1
    return n


# kind -> (module picker, activation, the input's scale: stride-2 steps down from full size, or for
# the decoder -(steps left up to full size), cropped to the patch)
LAYERS = {
    "s2_relu": (lambda m: m.encode_dep[1][0], ACT_RELU, 1, False),
    "s2_tanh": (lambda m: m.encode_aff[2][0], ACT_TANH, 2, False),
    "small_dep": (lambda m: m.encode_dep[0][0], ACT_RELU, 0, False),
    "small_aff": (lambda m: m.encode_aff[0][0], ACT_RELU, 0, False),
    "t2_relu": (lambda m: m.decode_aff[0][0], ACT_RELU, 3, False),
    "t2_c16_relu": (lambda m: m.decode_aff[1][0], ACT_RELU, -2, False),
    "t2_last_crop": (lambda m: m.decode_aff[2][0], ACT_NONE, -1, True),
}


def _act(y, act):
    return torch.relu(y) if act == ACT_RELU else torch.tanh(y) if act == ACT_TANH else y


@pytest.mark.parametrize("B,H,W", SHAPES)
@pytest.mark.parametrize("kind", list(LAYERS))
def test_layer_gradients_match_float64(kind, B, H, W, record_metric):
    """1. dx, dW, db of each layer kind from the native Function against the torch module in
    float64 on the CPU: the same weights, input and upstream gradient.  Asserted: relative L2
    <= BARS[kind] (<= 1e-4); the MIOpen fp32 module against the same reference is recorded beside it."""
    pick, act, scale, cropped = LAYERS[kind]
    m = _model(H, W, seed=1)
    conv = pick(m)
    if scale >= 0:
        hi, wi = _half(H, scale), _half(W, scale)
    else:  # decoder layers: 1/8 scale doubled
        up = 3 + scale
        hi, wi = _half(H, 3) * 2 ** up, _half(W, 3) * 2 ** up
    in_div = 10.0 if kind == "small_dep" else 1.0
    crop = (H, W) if cropped else None
    g = torch.Generator(device="cpu").manual_seed(7)
    x = torch.randn((B, conv.in_channels, hi, wi), generator=g, dtype=torch.float64) * (5.0 if in_div != 1.0 else 1.0)

    def run(module, xin, native):
        xin = xin.clone().requires_grad_(True)
        for p in module.parameters():
            p.grad = None
        if native:
            y = GruConvs().layer(module, xin, act=act, in_div=in_div, crop=crop)
        else:
            y = _act(module(xin / in_div if in_div != 1.0 else xin), act)
            if crop:
                y = y[:, :, :crop[0], :crop[1]]
        return xin, y

    ref = copy.deepcopy(conv).double().cpu()
    xr, yr = run(ref, x, False)
    up_g = torch.randn(yr.shape, generator=g, dtype=torch.float64)
    (yr * up_g).sum().backward()
    want = {"dx": xr.grad, "dW": ref.weight.grad, "db": ref.bias.grad}
    errs = {}
    for name, native in (("native", True), ("miopen", False)):
        xn, yn = run(conv, x.float().to(DEV), native)
        assert yn.shape == yr.shape
        (yn * up_g.float().to(DEV)).sum().backward()
        got = {"dx": xn.grad, "dW": conv.weight.grad, "db": conv.bias.grad}
        errs[name] = {k: _rel(got[k], want[k]) for k in want}
        for k, e in errs[name].items():
            record_metric(f"gconv_bwd/{kind}/{B}x{H}x{W}/{name}/{k}", e)
    print(kind, (B, H, W), errs)
    for k, e in errs["native"].items():
        assert e <= BARS[kind], (kind, k, e, errs)


@pytest.mark.parametrize("B,H,W", SHAPES)
def test_convgru_cell_gradients_match_float64(B, H, W, record_metric):
    """2. dh, dx and the six parameter gradients of GruConvs.gru against ConvGRU in float64 on
    the CPU.  Asserted: relative L2 <= 3e-6 (<= 1e-4); the MIOpen fp32 module is recorded beside it."""
    m = _model(H, W, seed=2)
    hh, ww = _half(H, 3), _half(W, 3)
    g = torch.Generator(device="cpu").manual_seed(8)
    h0 = torch.tanh(torch.randn((B, 128, hh, ww), generator=g, dtype=torch.float64))
    x0 = torch.relu(torch.randn((B, 128, hh, ww), generator=g, dtype=torch.float64))
    up_g = torch.randn((B, 128, hh, ww), generator=g, dtype=torch.float64)
    names = [n for n, _ in m.GRU.named_parameters()]
    assert len(names) == 6

    def run(gru, h, x, native):
        h, x = h.clone().requires_grad_(True), x.clone().requires_grad_(True)
        for p in gru.parameters():
            p.grad = None
        if native:
            gc = GruConvs()
            y = gc.gru(gc.pack(m), h, x)
        else:
            y = gru(h=h, x=x)
        (y * up_g.to(y)).sum().backward()
        out = {"dh": h.grad, "dx": x.grad}
        out.update({n: p.grad for n, p in gru.named_parameters()})
        return y, out

    ref = copy.deepcopy(m.GRU).double().cpu()
    yr, want = run(ref, h0, x0, False)
    errs = {}
    for name, native in (("native", True), ("miopen", False)):
        yn, got = run(m.GRU, h0.float().to(DEV), x0.float().to(DEV), native)
        assert _rel(yn, yr) <= 1e-5
        errs[name] = {k: _rel(got[k], want[k]) for k in want}
        for k, e in errs[name].items():
            record_metric(f"gconv_bwd/gru/{B}x{H}x{W}/{name}/{k}", e)
    print("gru", (B, H, W), errs)
    for k, e in errs["native"].items():
        assert e <= BARS["gru"], (k, e, errs)


# ------------------------------------------------------------------ the section under gradients
SUBS = ("encode_dep", "encode_aff", "GRU", "decode_aff")


def _section_inputs(B, H, W):
    g = torch.Generator(device=DEV).manual_seed(9)
    pred_init = torch.rand((B, 1, H, W), device=DEV, generator=g) * 10
    dep = pred_init * (torch.rand((B, 1, H, W), device=DEV, generator=g) < 0.02)
    off_aff = torch.randn((B, 24, H, W), device=DEV, generator=g)
    conf = torch.rand((B, 1, H, W), device=DEV, generator=g)
    proj = [torch.randn((B, 1, H, W), device=DEV, generator=g) for _ in range(T + 1)]
    return pred_init, off_aff, conf, dep, proj


@functools.lru_cache(maxsize=None)
def _section(B, H, W, mode, rep=0):
    """One training step of propagate_heads (T = 3): outputs, gradients and launch counts.
    mode: native | modules (native_gru = False) | train_off (native_gru_train = False) |
    no_modules (native, the torch submodules' forward raising) | nograd (native, inference)."""
    m = _model(H, W, seed=5)
    pred_init, off_aff, conf, dep, proj = _section_inputs(B, H, W)
    m.native_gru = mode != "modules"
    m.native_gru_train = mode != "train_off"
    if mode == "no_modules":
        def refuse(*a, **k):
            raise AssertionError("a torch GRU-mode module ran")
        for s in SUBS:
            getattr(m, s).forward = refuse
    m._gru_convs.reset_stats()
    calls = {s: 0 for s in SUBS}
    if mode != "no_modules":
        for s in SUBS:
            getattr(m, s).register_forward_hook(lambda mod, i, o, s=s: calls.__setitem__(s, calls[s] + 1))
    if mode == "nograd":
        with torch.no_grad():
            o = m.propagate_heads(pred_init, off_aff, conf, dep)
        return {"pred_inter": [p.clone() for p in o["pred_inter"]], "pred": o["pred"].clone()}
    ins = [t.clone().requires_grad_(True) for t in (pred_init, off_aff, conf)]
    o = m.propagate_heads(*ins, dep)
    loss = (o["pred"] * proj[T]).sum() + sum((p * q).sum() for p, q in zip(o["pred_inter"], proj))
    fwd_stats = dict(m._gru_convs.stats)
    loss.backward()
    grads = {f"{s}.{n}": p.grad.clone() for s in SUBS for n, p in getattr(m, s).named_parameters()}
    grads["aff_scale_const"] = m.aff_scale_const.grad.clone()
    grads.update({n: t.grad.clone() for n, t in zip(("pred_init", "off_aff", "confidence"), ins)})
    return {"pred_inter": [p.detach().clone() for p in o["pred_inter"]], "pred": o["pred"].detach().clone(),
            "grads": grads, "stats": dict(m._gru_convs.stats), "fwd_stats": fwd_stats, "module_calls": calls}


@pytest.mark.parametrize("B,H,W", SHAPES)
def test_section_gradients_native_vs_modules(B, H, W, record_metric):
    """3. propagate_heads (T = 3) under gradients, native against native_gru = False on the
    same model and inputs, the loss a fixed random projection of pred and every pred_inter:
    every GRU-mode parameter gradient, aff_scale_const's and the input gradients within 1e-3
    relative L2; the forward outputs within the 1e-4 RMSE bar."""
    n, r = _section(B, H, W, "native"), _section(B, H, W, "modules")
    assert n["stats"]["dgrad"] > 0 and r["stats"]["dgrad"] == 0
    for a, b in zip(n["pred_inter"] + [n["pred"]], r["pred_inter"] + [r["pred"]]):
        assert float(torch.sqrt(torch.mean((a.double() - b.double()) ** 2))) <= 1e-4
    assert len(n["grads"]) == len(r["grads"]) >= 6 * 3 + 6 + 4
    errs = {k: _rel(n["grads"][k], r["grads"][k]) for k in r["grads"]}
    for k, e in errs.items():
        record_metric(f"gconv_bwd/section/{B}x{H}x{W}/{k}", e)
    print("section", (B, H, W), errs)
    for k, e in errs.items():
        assert float(r["grads"][k].abs().max()) > 0, k
        assert e <= BAR_SECTION, (k, e)


def test_native_training_step_runs_without_the_torch_modules():
    """4. With the four torch submodules' forward raising, the native training step completes;
    the counters show T - 1 ConvGRU forwards and data / weight / gate gradient launches."""
    B, H, W = SHAPES[0]
    s = _section(B, H, W, "no_modules")
    assert s["stats"]["gru_fwd"] == T - 1
    assert s["stats"]["dgrad"] > 0 and s["stats"]["wgrad"] > 0 and s["stats"]["gates_bwd"] == 2 * (T - 1)
    assert s["fwd_stats"]["dgrad"] == 0 and s["fwd_stats"]["fwd"] > 0


def test_forward_under_gradients_is_the_inference_forward():
    """5. pred_inter of the native path under gradients is bit-identical to the native path
    under torch.no_grad(): the same kernels, and the fused normalisation is bit-equal to the
    two-launch form."""
    B, H, W = SHAPES[0]
    a, b = _section(B, H, W, "native"), _section(B, H, W, "nograd")
    assert len(a["pred_inter"]) == len(b["pred_inter"]) == T
    for i, (p, q) in enumerate(zip(a["pred_inter"], b["pred_inter"])):
        assert torch.equal(p, q), (i, float((p - q).abs().max()))


def test_backward_is_bit_reproducible():
    """6. Two backward passes on the same inputs give bit-identical gradients (fixed slab order,
    no atomics): encode_dep, encode_aff, the ConvGRU cell and decode_aff composed, i.e. every
    native backward kernel, from one fixed upstream gradient.  (Inside the section the
    propagation step's own backward precedes them, and its scatter uses float atomics: there
    the last bits differ from run to run on either path.)"""
    B, H, W = SHAPES[0]
    m = _model(H, W, seed=5)
    gc = GruConvs()
    g = torch.Generator(device=DEV).manual_seed(12)
    new_pred = torch.rand((B, 1, H, W), device=DEV, generator=g) * 10
    aff = torch.rand((B, 9, H, W), device=DEV, generator=g)
    up_g = torch.randn((B, 8, H, W), device=DEV, generator=g)

    def run():
        ins = [new_pred.clone().requires_grad_(True), aff.clone().requires_grad_(True)]
        for p in m.parameters():
            p.grad = None
        P = gc.pack(m)
        h = gc.gru(P, gc.encode_aff(P, ins[1]), gc.encode_dep(P, ins[0], m.args.max_depth))
        (gc.decode_aff(P, h, (H, W)) * up_g).sum().backward()
        out = {f"{s}.{n}": p.grad.clone() for s in SUBS for n, p in getattr(m, s).named_parameters()}
        out.update(new_pred=ins[0].grad.clone(), aff=ins[1].grad.clone())
        return out

    a, b = run(), run()
    assert len(a) == 26 and all(float(v.abs().max()) > 0 for v in a.values())
    diff = {k: _rel(a[k], b[k]) for k in a if not torch.equal(a[k], b[k])}
    assert not diff, diff


def test_native_gru_train_off_keeps_the_module_path():
    """7. native_gru_train = False: no native launch of any kind under gradients, the torch
    modules run exactly as often as with native_gru = False, and the gradients are the module
    path's.  "Exactly" cannot be asserted bit for bit: the module path does not reproduce
    itself (MIOpen's kernels and the propagation backward's float atomics; measured here,
    native_gru = False against a second run of itself: forward outputs differ in the last
    bits, gradients by 1.3e-7 .. 5.4e-7 relative L2, and native_gru_train = False against it
    by 2.7e-8 .. 3.3e-7).  Asserted instead: the same module calls, zero native counters, and
    the bar the project uses where only the summation order may differ, relative L2 <= 1e-5
    (tests/test_gpu_gru.py)."""
    B, H, W = SHAPES[0]
    a, r = _section(B, H, W, "train_off"), _section(B, H, W, "modules")
    assert all(v == 0 for v in a["stats"].values()), a["stats"]
    assert a["module_calls"] == r["module_calls"] == {"encode_dep": T - 1, "encode_aff": 1, "GRU": T - 1,
                                                      "decode_aff": T - 1}
    errs = {k: _rel(a["grads"][k], r["grads"][k]) for k in r["grads"]}
    print("train_off vs modules:", errs)
    for k, e in errs.items():
        assert e <= 1e-5, (k, e)
