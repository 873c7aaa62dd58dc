"""GPU: the float16 backward of the propagation section, every element of every gradient.

test_section_matches_f32_entry: propagate() on half tensors under autograd against the float32
entry (propagation._section_backward, pinned to float64 by tests/test_gpu_backward_elem.py) on
the float32 widenings of the same inputs and of the tensors the half forward returned.  Bar per
element (tests/_bwd_fp16.py): |float(g16) - g32| <= 2^-11 |g32| + 2^-25 + 2 (c X + Q), gamma
(float32) 2 (c X + Q); X == 0 => exactly 0.  Worst |d| / bar is recorded as
bwd_fp16_elem/<case>/<tensor>.

test_anchor_float64: kind ASS, T = 1, affinities scaled below the normaliser's clamp, against
the float64 oracle alone: |float(g16) - g64| <= 2^-11 |g64| + 2^-25 + c X + Q, recorded as
bwd_fp16_anchor/<case>/<tensor>.

Measured on an MI355X, worst |d| / bar over the cases: section 0.96 (pred_init), 0.98 (aff), 0.99
(offset), 0.97 (confidence), 0.03 (gamma); anchor 0.98, 0.99, 0.98, 0.98.  The one float16
rounding is what fills the bar: the float32 paths' own distance is a few percent of it.
"""
import numpy as np
import pytest
import torch

import _bwd_cases as bc
import _bwd_fp16 as hf
from nlspn_eccv20_amd import propagate, propagation

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _h(x, rg=False):
    """A float16 device tensor of the (float16-valued) float32 array x."""
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV).half().requires_grad_(rg)


def _w(t):
    return None if t is None else t.detach().float()


def run_half(c, s, T, kind, gamma):
    """The half section under autograd on inputs s.  Returns (gradients as float64 numpy, their
    dtypes, the float32 entry's gradients on the widened operands)."""
    K = c["kh"] * c["kw"] - 1
    off_aff = _h(np.concatenate([s["off"], s["aff"]], 1) if c["offset"] else s["aff"], True)
    aff = off_aff[:, 2 * K:] if c["offset"] else off_aff
    off = off_aff[:, :2 * K] if c["offset"] else None
    pi, cf, dep = _h(s["pred_init"], True), _h(s["conf"], True) if c["conf"] else None, _h(s["dep"])
    g = torch.tensor([gamma], device=DEV, requires_grad=kind == "TGASS")
    gp, gi = _h(s["grad_pred"]), _h(s["grad_inter"])
    o = propagate(pi, dep, cf, aff, off, g, prop_time=T, affinity=kind, kernel=(c["kh"], c["kw"]),
                  preserve_input=c["preserve"], always_clip=c["clip"])
    assert o["pred"].dtype == torch.float16 and o["pred_inter_tensor"].dtype == torch.float16
    leaves = {"oa": off_aff, "pred_init": pi}
    if c["conf"]:
        leaves["confidence"] = cf
    if kind == "TGASS":
        leaves["gamma"] = g
    grads = torch.autograd.grad((o["pred"], o["pred_inter_tensor"]), list(leaves.values()), (gp, gi))
    torch.cuda.synchronize()
    got = dict(zip(leaves, grads))
    dtypes = {k: v.dtype for k, v in got.items()}
    ga = got.pop("oa").float().cpu().numpy()
    out = {k: v.float().cpu().numpy() for k, v in got.items()}
    out["aff"] = ga[:, 2 * K:] if c["offset"] else ga
    if c["offset"]:
        out["offset"] = ga[:, :2 * K]
    if kind == "TGASS":
        out["gamma"] = np.float32(out["gamma"].item())
    # the float32 entry on the widened operands and the half forward's saved tensors
    r_pi, r_cf, r_aff, r_off, r_g, _ = propagation._section_backward(
        _w(pi), _w(dep), _w(cf), _w(aff).contiguous(), None if off is None else _w(off).contiguous(), g.detach(),
        _w(o["pred_inter_tensor"]), _w(o["aff"]), _w(o["confidence"]), _w(gp), _w(gi), c["kh"], c["kw"], T, kind,
        c["preserve"], c["clip"])
    torch.cuda.synchronize()
    ref = {"pred_init": r_pi.cpu().numpy(), "aff": r_aff.cpu().numpy()}
    if c["offset"]:
        ref["offset"] = r_off.cpu().numpy()
    if c["conf"]:
        ref["confidence"] = r_cf.cpu().numpy()
    if kind == "TGASS":
        ref["gamma"] = np.float32(r_g.item())
    return out, dtypes, ref


@pytest.mark.parametrize("name", hf.CHAIN)
def test_section_matches_f32_entry(oracle, record_metric, monkeypatch, tmp_path, name):
    c = bc.CASES[name]
    s = hf.rounded_inputs(name)
    _g64, X, info = hf.chain_oracle(oracle, name)
    for k, v in c["env"].items():
        monkeypatch.setenv(k, v)
    if name.startswith("res_"):
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        assert bc.backward_form(name, cus, str(tmp_path))[0] == "resident"
    got, dtypes, ref = run_half(c, s, c["T"], c["kind"], bc.gamma_of(name))
    assert dtypes["oa"] == torch.float16 and dtypes["pred_init"] == torch.float16
    assert dtypes.get("confidence", torch.float16) == torch.float16
    assert dtypes.get("gamma", torch.float32) == torch.float32
    failures = []
    for t in bc.tensors_of(name):
        cbar = min(4.0 * bc.R32[name][t], bc.ceiling(name, t))
        x = np.asarray(X[t], np.float64).ravel()
        Q = hf.quantum(info, c["T"]) if t == "gamma" else hf.quantum(info, c["T"], np.shape(X[t]))
        if t == "aff":
            Q = Q + bc.aff_slack(name, info)
        allowed = hf.half_bar(ref[t], 2.0 * (cbar * x + Q), gamma=t == "gamma")
        r, i = hf.worst(got[t], ref[t], allowed)
        record_metric(f"bwd_fp16_elem/{name}/{t}", r)
        print(f"bwd_fp16_elem {name} {t}: worst |g16 - g32| / bar = {r:.3f}")
        g = np.asarray(got[t], np.float64).ravel()
        if not np.all(g[x == 0] == 0):
            failures.append(f"{t}: an element whose bound is 0 is not exactly 0")
        if not r <= 1.0:
            failures.append(f"{t}: |g16 - g32| / bar = {r:.3f} at flat index {i} "
                            f"(g16 {g[i]!r}, g32 {float(np.ravel(ref[t])[i])!r}, X {x[i]!r})")
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("name", hf.ANCHOR)
def test_anchor_float64(oracle, record_metric, name):
    c = bc.CASES[name]
    s, _scale = hf.anchor_inputs(name)
    g64, X, info = hf.anchor_oracle(oracle, name)
    got, dtypes, _ref = run_half(c, s, 1, "ASS", 1.0)
    assert all(d == torch.float16 for d in dtypes.values())
    cbar = hf.anchor_ceiling(name)
    failures = []
    for t in (t for t in bc.tensors_of(name) if t != "gamma"):
        x = np.asarray(X[t], np.float64).ravel()
        allowed = hf.half_bar(g64[t], cbar * x + hf.quantum(info, 1, np.shape(X[t])))
        r, i = hf.worst(got[t], g64[t], allowed)
        record_metric(f"bwd_fp16_anchor/{name}/{t}", r)
        print(f"bwd_fp16_anchor {name} {t}: worst |g16 - g64| / bar = {r:.3f}")
        if not r <= 1.0:
            failures.append(f"{t}: |g16 - g64| / bar = {r:.3f} at flat index {i}")
    assert not failures, "\n".join(failures)
