"""GPU: every entry on views that start a few elements into a buffer, and on packed head outputs
with an odd batch stride: which build the host picks for the pointers it is handed.

The host chooses between vector and scalar builds and between resident and step launches from
pointer values and strides (`vec` / `ptrs_ok` / `first_ok` / `l2ok` / `copy_off` in
nlspn_prop_fwd.hip, `c.vec` / `vec` in nlspn_prop_bwd.hip, `vec` of both head kernels and of the
affinity normalisation in nlspn_seam.hip).  The per-element tests hand every entry freshly
allocated, 16-byte aligned tensors, so the "pointer not aligned, W % 4 == 0" side of each gate
never ran, and a pointer that a gate forgets would be read with 16-byte loads from an address
that is not a multiple of 16.

shifted() puts a tensor m elements into a larger flat buffer (f32: m = 1, 2, 3; f16: m = 1, 2, 4:
4, 8 and 12 bytes / 2, 4 and 8 bytes past a 16-byte boundary).  Each pointer argument of an entry
is misaligned alone, then all together, at shapes the vector and resident builds take (W % 4 == 0).

Bars.
  * Forward entries: BIT-EQUAL to the all-aligned call.  Every propagation form issues the same
    per-pixel IEEE sequence (pinned bit-equal to the oracle's loop, tests/test_gpu_forward_elem.py);
    affnorm_kernel's PX only widens the loads; in heads_kernel and headsx3_kernel the VEC parameter
    changes HdWin<VEC>::load alone (one 16-byte load or four 4-byte loads of the same cells into the
    same registers; nlspn_heads.h, nlspn_heads_x3.h), the sums are untouched; the S2D kernel has one
    build.
  * The propagation backward is not bit-reproducible (its dL/df windows are flushed with float
    atomics, nlspn_backward.h) and its scalar build has another tile: its gradients are held by the
    existing per-element bar of tests/test_gpu_backward_elem.py against the float64 oracle
    (_bwd_cases "res_tiny_parts"), for every misalignment and stride.
  * The stand-alone normalisation's backward has one build and fixed-order sums: bit-equal.

Outputs and the workspace are allocated by the wrappers, so they are misaligned once through the
raw C ABI (a non-PyTorch host may pass exactly that): pred_inter, pred, aff_out,
off_out, conf_out by 4 bytes each and together, and pred_inter by 64 bytes (16-byte aligned, not
128: the `l2ok` gate of the per-line hand-offs).
"""
import numpy as np
import pytest
import torch

import _big_cases as big
import _big_checks as chk
import _bwd_cases as bc
from nlspn_eccv20_amd import PropagationPlan, _lib, affinity_normalization, prop_step, propagate, propagate_normalized
from nlspn_eccv20_amd.heads import HeadWeights, head_epilogue, head_epilogue_prologue
from nlspn_eccv20_amd.propagation import _affnorm_backward
from nlspn_eccv20_amd.s2d import s2d_front
from nlspn_eccv20_amd.synthetic import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHIFTS = {torch.float32: (1, 2, 3), torch.float16: (1, 2, 4)}
B, H, W, K, T = 2, 40, 64, 8, 3


def shifted(t, m):
    """A view of t's shape and values that starts m elements into a larger flat buffer."""
    if t is None:
        return None
    buf = torch.empty(t.numel() + m + 64, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 128 == 0
    v = buf[m:m + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == (m * t.element_size()) % 16 and v.is_contiguous() and torch.equal(_bits(v), _bits(t))
    return v


def _bits(x):
    return x.view(torch.int32 if x.element_size() == 4 else torch.int16)


def _same(a, b, what):
    assert (a is None) == (b is None), what
    if a is not None:
        assert a.shape == b.shape and torch.equal(_bits(a), _bits(b)), what


def _same_dict(a, b, what, keys=("pred", "pred_inter_tensor", "aff", "offset", "confidence")):
    for k in keys:
        if k in a:
            _same(a[k], b[k], f"{what}: {k}")


def _variants(args, dtype):
    """(label, shifted args): each tensor of `args` (a dict) misaligned alone by every shift, then
    all together by every shift."""
    for m in SHIFTS[dtype]:
        for n in args:
            if args[n] is not None:
                yield f"{n} + {m}", {k: (shifted(v, m) if k == n else v) for k, v in args.items()}
        yield f"all + {m}", {k: shifted(v, m) for k, v in args.items()}


def _inputs(dtype, seed=5):
    s = synth(B, H, W, K, seed=seed)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV, dtype)  # noqa: E731
    oa = t(s["off_aff"])
    return {"pred_init": t(s["pred_init"]), "dep": t(s["dep"]), "confidence": t(s["conf"]),
            "aff": oa[:, 2 * K:].contiguous(), "offset": oa[:, :2 * K].contiguous()}


GAMMA = None


def _gamma():
    global GAMMA
    if GAMMA is None:
        GAMMA = torch.tensor([4.0], device=DEV)
    return GAMMA


def _prop(a, **kw):
    with torch.no_grad():
        return propagate(a["pred_init"], a["dep"], a["confidence"], a["aff"], a["offset"], _gamma(), prop_time=T, **kw)


def _assert_aligned_call_is_resident(dtype):
    """The all-aligned reference call of this shape takes the resident kernel (and, W % 4 == 0 with
    aligned planes, the vector step build in front of or instead of it): the comparisons below are
    resident / vector against what a misaligned pointer falls back to, not steps against steps."""
    code = _lib.DTYPE_F32 if dtype == torch.float32 else _lib.DTYPE_F16
    assert _lib.get().nlspn_resident_config(code, B, H, W, 3, 3, T, 1, None, None, None) == 1
    assert W % 4 == 0


# ------------------------------------------------------------------ the forward entries
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_propagate(dtype):
    _assert_aligned_call_is_resident(dtype)
    a = _inputs(dtype)
    ref = _prop(a)
    assert torch.isfinite(ref["pred"]).all()
    n = 0
    for label, v in _variants(a, dtype):
        _same_dict(_prop(v), ref, label)
        n += 1
    assert n == 3 * 6
    torch.cuda.synchronize()
    _lib.check_resident(torch.device(DEV))


def _step_args(dtype):
    a = _inputs(dtype)
    o = _prop(a)
    return {"feat": a["pred_init"], "confidence": o["confidence"], "dep": a["dep"], "aff": o["aff"], "offset": o["offset"]}


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("layout", ["inserted", "raw"])
def test_prop_step(dtype, layout):
    a = _step_args(dtype)
    if layout == "raw":
        a["offset"] = _inputs(dtype)["offset"]
    run = lambda v, **kw: prop_step(v["feat"], v["confidence"], v["dep"], v["aff"], v["offset"], offset_layout=layout,  # noqa: E731
                                    **kw)
    with torch.no_grad():
        ref, ref_pred = run(a), torch.empty_like(a["feat"])
        _same(run(a, out=torch.empty_like(ref), pred_out=ref_pred), ref, "out=")  # the ctypes path
        for label, v in _variants(a, dtype):
            _same(run(v), ref, label)
            # out and pred_out misaligned as well
            out, pred = shifted(torch.empty_like(ref), SHIFTS[dtype][0]), shifted(torch.empty_like(ref), SHIFTS[dtype][1])
            _same(run(v, out=out, pred_out=pred), ref, label + " (out=)")
            _same(pred, ref_pred, label + " (pred_out=)")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_propagate_normalized(dtype):
    a = _step_args(dtype)
    run = lambda v: propagate_normalized(v["feat"], v["dep"], v["confidence"], v["aff"], v["offset"], T, 3)  # noqa: E731
    with torch.no_grad():
        ref = run(a)
        for label, v in _variants(a, dtype):
            _same_dict(run(v), ref, label)
    torch.cuda.synchronize()
    _lib.check_resident(torch.device(DEV))


def test_propagation_plan():
    a = _inputs(torch.float32)
    ref = _prop(a)
    for label, v in _variants(a, torch.float32):
        plan = PropagationPlan(v["pred_init"], v["dep"], v["confidence"], v["aff"], v["offset"], _gamma(), prop_time=T)
        for _ in range(2):
            o = plan.replay()
        plan.check()
        _same_dict(o, ref, label)
        plan.close()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_affinity_normalization(dtype):
    aff = _inputs(dtype)["aff"]
    ref = affinity_normalization(aff, _gamma(), "TGASS")
    for m in SHIFTS[dtype]:
        _same(affinity_normalization(shifted(aff, m), _gamma(), "TGASS"), ref, f"aff + {m}")
    # a batch stride that is no multiple of 4: K * H * W + 1 and + 2, + 4 (a multiple: the vector build)
    n = K * H * W
    for pad in (1, 2, 4):
        buf = torch.zeros(B * (n + pad) + 8, dtype=dtype, device=DEV)
        v = buf.as_strided((B, K, H, W), (n + pad, H * W, W, 1))
        v.copy_(aff)
        assert v.stride(0) % 4 == pad % 4
        _same(affinity_normalization(v, _gamma(), "TGASS"), ref, f"aff batch stride + {pad}")


def test_affinity_normalization_backward():
    aff = _inputs(torch.float32)["aff"]
    g = torch.randn((B, K + 1, H, W), device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
    gr, gg = _affnorm_backward(aff, _gamma(), g, "TGASS")
    for label, v in _variants({"aff": aff, "grad": g}, torch.float32):
        r, q = _affnorm_backward(v["aff"], _gamma(), v["grad"], "TGASS")
        _same(r, gr, label)
        _same(q, gg, label + " (gamma)")
    n = K * H * W
    buf = torch.zeros(B * (n + 1) + 8, device=DEV)
    v = buf.as_strided((B, K, H, W), (n + 1, H * W, W, 1))
    v.copy_(aff)
    r, q = _affnorm_backward(v, _gamma(), g, "TGASS")
    _same(r, gr, "aff batch stride + 1")
    _same(q, gg, "aff batch stride + 1 (gamma)")


# ------------------------------------------------------------------ heads and S2D
def _heads(prologue):
    if prologue:
        from test_gpu_heads_prologue import _case
        oa, idc, cfc, src, dep = _case(B, 16, H, W, seed=3)
    else:
        from test_gpu_heads import _case
        (oa, idc, cfc, src), dep = _case(B, 16, H, W, 24, seed=3), None
    a = dict(zip(("fe1", "fd_oa", "fd_id", "fd_cf"), src))
    if prologue:
        a["dep"] = dep
    return oa, idc, cfc, a


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_head_epilogue(precision):
    oa, idc, cfc, a = _heads(False)
    hw = HeadWeights()
    run = lambda v: head_epilogue(v["fe1"], v["fd_oa"], oa, v["fd_id"], idc, v["fd_cf"], cfc, weights=hw,  # noqa: E731
                                  precision=precision)
    with torch.no_grad():
        ref = run(a)
        for label, v in _variants(a, torch.float32):
            for got, want, n in zip(run(v), ref, ("pred_init", "off_aff", "confidence")):
                _same(got, want, f"{label}: {n}")


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_head_epilogue_prologue(precision):
    oa, idc, cfc, a = _heads(True)
    hw = HeadWeights()
    run = lambda v: head_epilogue_prologue(v["fe1"], v["fd_oa"], oa, v["fd_id"], idc, v["dep"], _gamma(), "TGASS",  # noqa: E731
                                           v["fd_cf"], cfc, True, False, weights=hw, precision=precision)
    with torch.no_grad():
        ref = run(a)
        for label, v in _variants(a, torch.float32):
            _same_dict(run(v), ref, label, ("pred_init", "offset", "aff", "confidence", "p0"))


def test_s2d_front():
    from test_gpu_s2d import _case
    dep, w1, b1, w2, b2 = (t.to(DEV) for t in _case(B, H, W, 0.05, seed=4))
    with torch.no_grad():
        ref = s2d_front(dep, w1, b1, w2, b2)
        for m in SHIFTS[torch.float32]:
            _same(s2d_front(shifted(dep, m), w1, b1, w2, b2), ref, f"dep + {m}")
            _same(s2d_front(dep, shifted(w1, m), shifted(b1, m), shifted(w2, m), shifted(b2, m)), ref, f"weights + {m}")


# ------------------------------------------------------------------ outputs and workspace: the raw C ABI
def _raw_propagate(a, outs):
    """nlspn_propagate on caller-made outputs (dict pred_inter, pred, aff, offset, confidence, workspace)."""
    _lib.call("nlspn_propagate", torch.device(DEV), _lib.DTYPE_F32, a["pred_init"], a["dep"], a["confidence"], a["aff"],
              K * H * W, a["offset"], 2 * K * H * W, _gamma(), outs["pred_inter"], outs["pred"], outs["aff"], outs["offset"],
              outs["confidence"], outs["workspace"], B, H, W, 3, 3, T, _lib.AFF_KINDS["TGASS"], _lib.flags(True, False),
              _lib.STREAM, resident=True)
    torch.cuda.synchronize()
    _lib.check_resident(torch.device(DEV))


def test_misaligned_outputs_raw_abi():
    _assert_aligned_call_is_resident(torch.float32)  # (the 64-byte pred_inter case reaches l2ok only on a resident call)
    a = _inputs(torch.float32)
    ref = _prop(a)
    e = lambda *sh: torch.full(sh, float("nan"), device=DEV)  # noqa: E731
    ws_words = _lib.get().nlspn_workspace_bytes(_lib.DTYPE_F32, B, H, W) // 4
    cases = [(n, 1) for n in ("pred_inter", "pred", "aff", "offset", "confidence")] + [("all", 1), ("pred_inter", 16),
                                                                                         ("workspace", 1), ("workspace", 4)]
    for which, m in cases:
        outs = {"pred_inter": e(T, B, 1, H, W), "pred": e(B, 1, H, W), "aff": e(B, K + 1, H, W),
                "offset": e(B, 2 * (K + 1), H, W), "confidence": e(B, 1, H, W),
                "workspace": torch.zeros(ws_words, dtype=torch.int32, device=DEV)}
        for n in outs:
            if which == n or (which == "all" and n != "workspace"):
                outs[n] = shifted(outs[n], m)
        if which == "pred_inter" and m == 16:
            assert outs["pred_inter"].data_ptr() % 128 == 64
        _raw_propagate(a, outs)
        got = dict(outs, pred_inter_tensor=outs["pred_inter"])
        _same_dict(got, ref, f"{which} + {m}")


# ------------------------------------------------------------------ batch strides of the packed head output
def _packed_view(oa, pad):
    n = 3 * K * H * W
    buf = torch.zeros(B * (n + pad) + 8, dtype=oa.dtype, device=DEV)
    v = buf.as_strided((B, 3 * K, H, W), (n + pad, H * W, W, 1))
    v.copy_(oa)
    return v


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_packed_batch_stride_forward(dtype):
    a = _inputs(dtype)
    oa = torch.cat([a["offset"], a["aff"]], 1)
    ref = _prop(a)
    for pad in (1, 4):
        v = _packed_view(oa, pad)
        assert v.stride(0) == 3 * K * H * W + pad
        _same_dict(_prop(dict(a, aff=v[:, 2 * K:], offset=v[:, :2 * K])), ref, f"batch stride 3K HW + {pad}")
    torch.cuda.synchronize()
    _lib.check_resident(torch.device(DEV))


# ------------------------------------------------------------------ the propagation backward
BWD = "res_tiny_parts"


@pytest.fixture(scope="module")
def bwd_ref(oracle):
    oracle.set_threads(16)
    s = bc.grid_inputs(BWD)
    return (s,) + tuple(bc.oracle_bound(oracle, BWD, s))


def _bwd_grads(s, shift=None, pad=None, name=BWD):
    """The kernels' gradients for the case through autograd; shift: {tensor: m} of the inputs and
    upstream gradients to misalign; pad: the packed head output's extra batch stride."""
    c = bc.CASES[name]
    Kc, shift = c["kh"] * c["kw"] - 1, shift or {}

    def t(n, x):
        x = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
        return shifted(x, shift[n]) if n in shift else x

    oa = t("off_aff", np.concatenate([s["off"], s["aff"]], 1))
    if pad is not None:
        n = 3 * Kc * c["H"] * c["W"]
        buf = torch.zeros(c["B"] * (n + pad) + 8, device=DEV)
        v = buf.as_strided(tuple(oa.shape), (n + pad, c["H"] * c["W"], c["W"], 1))
        v.copy_(oa)
        oa = v
    oa.requires_grad_(True)
    pi, cf = t("pred_init", s["pred_init"]).requires_grad_(True), t("confidence", s["conf"]).requires_grad_(True)
    g = torch.tensor([bc.gamma_of(name)], device=DEV, requires_grad=True)
    if c["form"] == "step_op":  # the section composed of prop_step calls: nlspn_prop_step_backward per iteration
        from test_gpu_step_backward import composed_section
        pred, inter = composed_section(pi, t("dep", s["dep"]), cf, oa[:, 2 * Kc:], oa[:, :2 * Kc], g, c["T"], c["kind"],
                                       (c["kh"], c["kw"]), c["preserve"], c["clip"])
    else:
        o = propagate(pi, t("dep", s["dep"]), cf, oa[:, 2 * Kc:], oa[:, :2 * Kc], g, prop_time=c["T"])
        pred, inter = o["pred"], o["pred_inter_tensor"]
    torch.autograd.backward([pred, inter], [t("grad_pred", s["grad_pred"]), t("grad_inter", s["grad_inter"])])
    torch.cuda.synchronize()
    ga = oa.grad.cpu().numpy()
    return {"pred_init": pi.grad.cpu().numpy(), "aff": ga[:, 2 * Kc:], "offset": ga[:, :2 * Kc],
            "confidence": cf.grad.cpu().numpy(), "gamma": np.float32(g.grad.item())}


BWD_RUNS = ([({n: m}, None) for n, m in (("pred_init", 1), ("dep", 2), ("confidence", 3), ("off_aff", 1), ("grad_pred", 1),
                                         ("grad_inter", 3))]
            + [({n: m for n in ("pred_init", "dep", "confidence", "off_aff", "grad_pred", "grad_inter")}, None) for m in (1, 2, 3)]
            + [(None, 1), (None, 4)])


@pytest.mark.parametrize("shift,pad", BWD_RUNS,
                         ids=["+".join(f"{n}{m}" for n, m in (s or {}).items()) or f"stride+{p}" for s, p in BWD_RUNS])
def test_propagate_backward(bwd_ref, shift, pad):
    s, g64, X, info = bwd_ref
    failures = chk.backward_failures(BWD, _bwd_grads(s, shift, pad), g64, X, info)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("m", [1, 2, 3])
def test_prop_step_backward(oracle, m):
    """nlspn_prop_step_backward's own `vec` gate (feat, conf, dep): the section composed of prop_step
    calls (_bwd_cases "step_op", W % 4 == 0) with a misaligned dep, the one operand that reaches every
    step as the caller's own tensor (feat and conf are fresh tensors of the blends); so every
    iteration's forward and backward take the scalar builds.  The bar of the case, unchanged."""
    oracle.set_threads(16)
    s = bc.grid_inputs("step_op")
    g64, X, info = bc.oracle_bound(oracle, "step_op", s)
    assert bc.CASES["step_op"]["W"] % 4 == 0 and bc.CASES["step_op"]["preserve"]
    failures = chk.backward_failures("step_op", _bwd_grads(s, {"dep": m, "off_aff": m}, name="step_op"), g64, X, info)
    assert not failures, "\n".join(failures)
