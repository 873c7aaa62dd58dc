"""GPU: prop_step and affinity_normalization train in float16 storage.

Each half call runs under autograd, through the Python function and through torch.ops.nlspn.*,
against its float32 entry (propagation._step_backward / _affnorm_backward) on the widened
operands.  A half gradient element is the float32 value rounded once, so:

  * the step's affinity and offset gradients and the normalisation's gradients are sums one
    thread forms in a fixed order, the same in both storage types: g16 == half(g32) bit for
    bit, and the normalisation's dL/dgamma (float32, fixed-order partial sums) is equal;
  * the step's feat and confidence gradients pass through dL/df, whose tile halos meet in float
    atomics: |float(g16) - g32| <= 2^-11 |g32| + 2^-25 + 2 (c X + Q), the section tests' form.
    X and Q come from the float64 oracle: a step on normalised affinities a with sum |a| < 1 is
    the section at T = 1, kind ASS, without the prologue, so the oracle runs it with
    preserve_input and always_clip off and the upstream gradient (1 - m) g (the step's own
    blend; the clamp's gate can only remove terms, so leaving it out keeps X a bound).
    c is the operation-count ceiling at T = 1.

Shapes: 2x24x40 (3x3: offsets, no offsets, always_clip, no confidence) and 2x16x48 (1x17).
"""
import numpy as np
import pytest
import torch

import _bwd_cases as bc
import _bwd_fp16 as hf
from nlspn_eccv20_amd import affinity_normalization, ops, prop_step, propagation

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _operator_layer():
    ops.load()  # torch.ops.nlspn.*

# name -> (case of tests/_bwd_cases.py whose inputs it takes, overrides)
STEP_CASES = {
    "k3_offsets": ("res_ASS", {}),
    "k3_noffset": ("noffset", {}),
    "k3_clip": ("res_ASS", {"clip": True}),
    "k3_noconf": ("res_ASS", {"conf": False}),
    "k17": ("k17", {}),
}


def _h(x, rg=False):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV).half().requires_grad_(rg)


def _w(t):
    return None if t is None else t.detach().float().contiguous()


@pytest.mark.parametrize("api", ["python", "ops"])
@pytest.mark.parametrize("case", list(STEP_CASES))
def test_prop_step_half_matches_f32_entry(oracle, record_metric, case, api):
    name, over = STEP_CASES[case]
    c = dict(bc.CASES[name], **over)
    kh, kw = c["kh"], c["kw"]
    s, _ = hf.anchor_inputs(name)  # float16 values, raw affinities scaled to sum |a| <= 0.5
    with torch.no_grad():
        aff_n = affinity_normalization(_h(s["aff"]), torch.ones(1, device=DEV), "ASS")
    assert aff_n.dtype == torch.float16
    feat, conf, dep = _h(s["pred_init"], True), _h(s["conf"], True) if c["conf"] else None, _h(s["dep"])
    dep_in = dep if c["preserve"] else None
    aff_n = aff_n.requires_grad_(True)
    off = _h(s["off"], True)
    g_out = _h(s["grad_inter"][0])
    if api == "python":
        out = prop_step(feat, conf, dep_in, aff_n, off, kernel=(kh, kw), offset_layout="raw",
                        preserve_input=c["preserve"], always_clip=c["clip"])
    else:
        out = torch.ops.nlspn.prop_step(feat, conf, dep_in, aff_n, off, kh, kw, True, c["preserve"], c["clip"])
    leaves = {"feat": feat, "aff": aff_n}
    if conf is not None:
        leaves["conf"] = conf
    if off is not None:
        leaves["off"] = off
    got = dict(zip(leaves, torch.autograd.grad(out, list(leaves.values()), g_out)))
    r_feat, r_conf, r_aff, r_off = propagation._step_backward(_w(feat), _w(conf), _w(dep_in), _w(aff_n), _w(off),
                                                              _w(g_out), kh, kw, c["preserve"], c["clip"])
    torch.cuda.synchronize()
    assert all(g.dtype == torch.float16 for g in got.values())
    # per-thread sums in a fixed order: the float32 values, rounded once
    assert torch.equal(got["aff"].view(torch.int16), r_aff.half().view(torch.int16))
    if off is not None:
        assert torch.equal(got["off"].view(torch.int16), r_off.half().view(torch.int16))
    # dL/df: float atomics at the tile halos
    f64 = lambda x: None if x is None else np.asarray(x, np.float64)  # noqa: E731
    m = (s["dep"] > 0).astype(np.float64) if c["preserve"] else 0.0
    go = (1.0 - m) * f64(s["grad_inter"][0])
    oracle.set_threads(16)
    _g, X, info = oracle.propagate_backward_bound(
        f64(s["pred_init"]), f64(s["dep"]), f64(s["conf"]) if c["conf"] else None, f64(s["aff"]), f64(s["off"]), 1.0,
        np.zeros_like(go), go[None], kind="ASS", kh=kh, kw=kw, prop_time=1, preserve_input=False, always_clip=False)
    cbar = hf.anchor_ceiling(name)
    failures = []
    for t, ref, xk in (("feat", r_feat, "pred_init"), ("conf", r_conf, "confidence")):
        if t not in got:
            continue
        x = np.asarray(X[xk], np.float64).ravel()
        ref = ref.cpu().numpy()
        g = got[t].float().cpu().numpy()
        allowed = hf.half_bar(ref, 2.0 * (cbar * x + hf.quantum(info, 1, np.shape(X[xk]))))
        r, i = hf.worst(g, ref, allowed)
        record_metric(f"step_bwd_fp16/{case}/{api}/{t}", r)
        print(f"step_bwd_fp16 {case} {api} {t}: worst |g16 - g32| / bar = {r:.3f}")
        if not np.all(g.ravel()[x == 0] == 0):
            failures.append(f"{t}: an element whose bound is 0 is not exactly 0")
        if not r <= 1.0:
            failures.append(f"{t}: |g16 - g32| / bar = {r:.3f} at flat index {i}")
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("api", ["python", "ops"])
@pytest.mark.parametrize("kind", ["AS", "ASS", "TC", "TGASS"])
def test_affinity_normalization_half_matches_f32_entry(kind, api):
    s = hf.rounded_inputs("res_TC")  # 2x24x40, K = 8, a quarter of the raw affinities negative
    K = s["aff"].shape[1]
    aff = _h(s["aff"], True)
    g = torch.tensor([bc._gamma(kind, K)], device=DEV, requires_grad=kind == "TGASS")
    rng = np.random.default_rng(77)
    g_out = _h(rng.standard_normal((s["aff"].shape[0], K + 1) + s["aff"].shape[2:]).astype(np.float32))
    out = affinity_normalization(aff, g, kind) if api == "python" else torch.ops.nlspn.affinity_normalization(aff, g, kind)
    assert out.dtype == torch.float16
    grads = torch.autograd.grad(out, [aff, g] if kind == "TGASS" else [aff], g_out)
    r_raw, r_gamma = propagation._affnorm_backward(_w(aff), g.detach(), _w(g_out), kind)
    torch.cuda.synchronize()
    assert grads[0].dtype == torch.float16
    assert torch.equal(grads[0].view(torch.int16), r_raw.half().view(torch.int16))
    if kind == "TGASS":
        assert grads[1].dtype == torch.float32 and grads[1].item() == r_gamma.item()


def _composed_half(pi, dep, cf, aff_raw, off, g, T, kind, kern, preserve, clip):
    """test_gpu_step_backward.composed_section with the blend's mask in the storage dtype."""
    aff = affinity_normalization(aff_raw, g, kind)
    conf_eff, p = cf, pi
    if preserve:
        m = (dep > 0).to(pi.dtype)
        conf_eff = (1 - m) * cf + m
        p = (1 - m) * pi + m * dep
    if clip:
        p = torch.clamp(p, min=0)
    p = p.contiguous()
    inter = []
    for _ in range(T):
        p = prop_step(p, conf_eff, dep if preserve else None, aff, off, kernel=kern, offset_layout="raw",
                      preserve_input=preserve, always_clip=clip)
        inter.append(p)
    return (p if clip else torch.clamp(p, min=0)), torch.stack(inter, 0)


def test_composed_section_half_trains():
    """T = 5 differentiable half steps and normalisations through autograd: finite half gradients."""
    s = hf.rounded_inputs("res_tiny_parts")
    K = 8
    oa = _h(np.concatenate([s["off"], s["aff"]], 1), True)
    pi, cf, dep = _h(s["pred_init"], True), _h(s["conf"], True), _h(s["dep"])
    g = torch.tensor([4.0], device=DEV, requires_grad=True)
    pred, inter = _composed_half(pi, dep, cf, oa[:, 2 * K:], oa[:, :2 * K], g, 5, "TGASS", (3, 3), True, False)
    assert pred.dtype == torch.float16 and inter.dtype == torch.float16
    loss = (pred * _h(s["grad_pred"])).sum() + (inter * _h(s["grad_inter"][:5])).sum()
    loss.backward()
    torch.cuda.synchronize()
    for t in (oa, pi, cf):
        assert t.grad.dtype == torch.float16 and torch.isfinite(t.grad).all() and t.grad.abs().sum() > 0
    assert g.grad.dtype == torch.float32 and torch.isfinite(g.grad).all()
