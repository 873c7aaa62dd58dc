"""CPU: the conditions the float16 backward tests rest on, and the float16 backward's C ABI.

For every case the GPU tests run on float16-rounded inputs (tests/_bwd_fp16.py), with the
float64 oracle:

  * every kink margin stays >= bc.GUARD, so the float16 rounding of the inputs moved no value
    across a floor, a clamp or the normaliser's clamp;
  * max |g64| <= 2^14: no gradient overflows float16, no loss scale is needed;
  * at most 5 % of any gradient tensor's elements lie in (0, 2^-14), float16's subnormal range
    (the bar's absolute term 2^-25 is half a subnormal step: a condition, not a measurement);
  * the anchor cases' normaliser stays below its clamp: max sum |a| + 1e-4 <= 0.51.

ABI: the dtype-aware workspace sizes equal the float32 functions for float32, match the
documented float16 formula and return 0 on bad arguments; dtype 7 is refused with
NLSPN_EUNSUPPORTED by all three backward entries; null-pointer and stride refusals are the
same for float16 as for float32.
"""
import ctypes

import numpy as np
import pytest

import _bwd_cases as bc
import _bwd_fp16 as hf
from nlspn_eccv20_amd import _lib


def _conditions(name, g64, info, tensors):
    assert min(info["min_pre"], info["min_s1"], info["min_u"]) >= bc.GUARD, (name, info["min_pre"], info["min_s1"],
                                                                             info["min_u"])
    for t in tensors:
        g = np.abs(np.asarray(g64[t], np.float64)).ravel()
        assert g.max() <= 2.0 ** 14, (name, t, g.max())
        share = float(np.mean((g > 0) & (g < 2.0 ** -14)))
        print(f"{name} {t}: max |g64| {g.max():.3g}, subnormal share {share:.4f}")
        assert share <= 0.05, (name, t, share)


@pytest.mark.parametrize("name", hf.CHAIN)
def test_chain_case_conditions(oracle, name):
    g64, _X, info = hf.chain_oracle(oracle, name)
    _conditions(name, g64, info, bc.tensors_of(name))


@pytest.mark.parametrize("name", hf.ANCHOR)
def test_anchor_case_conditions(oracle, name):
    s, scale = hf.anchor_inputs(name)
    assert float(np.abs(s["aff"].astype(np.float64)).sum(1).max()) + 1e-4 <= 0.51
    assert scale == {"res_ASS": 2.0 ** -5, "noffset": 2.0 ** -5, "k17": 2.0 ** -6, "k5x5": 2.0 ** -6}[name]
    g64, _X, info = hf.anchor_oracle(oracle, name)
    _conditions(name, g64, info, [t for t in bc.tensors_of(name) if t != "gamma"])


def test_rounding_keeps_tap_classes():
    """Integer tap coordinates stay integer and fractional ones fractional under the rounding."""
    for name in hf.CHAIN:
        raw, s = bc.grid_inputs(name), hf.rounded_inputs(name)
        if raw["off"] is None:
            continue
        assert np.array_equal(raw["off"] == np.floor(raw["off"]), s["off"] == np.floor(s["off"])), name


# ------------------------------------------------------------------ ABI
def _base_bytes(B, H, W, kh, kw):
    return _lib.get().nlspn_backward_workspace_bytes(B, H, W, kh, kw)


@pytest.mark.parametrize("B,H,W,kh,kw,T,planes", [
    (8, 228, 304, 3, 3, 18, 18),    # two-pass with T > 2K: the dL/dout store, T planes
    (8, 228, 304, 3, 3, 6, 16),     # T <= 2K: 2K planes cover either form
    (2, 24, 40, 3, 3, 26, 16),      # T > 3K: one-pass, 2K offset accumulators
    (16, 228, 304, 1, 17, 36, 32),  # 1x17: one-pass
    (2, 16, 32, 5, 5, 4, 48),
])
def test_section_workspace_sizes(B, H, W, kh, kw, T, planes):
    lib = _lib.get()
    f = lib.nlspn_backward_workspace_bytes_dtype
    assert f(_lib.DTYPE_F32, B, H, W, kh, kw, T) == _base_bytes(B, H, W, kh, kw)
    assert f(_lib.DTYPE_F16, B, H, W, kh, kw, T) == _base_bytes(B, H, W, kh, kw) + 4 * B * H * W * planes


def test_documented_extra_workspace():
    """40 MB at C2 (two-pass, T = 18), about 142 MB at C5 (one-pass, 2K = 32)."""
    f = _lib.get().nlspn_backward_workspace_bytes_dtype
    c2 = f(_lib.DTYPE_F16, 8, 228, 304, 3, 3, 18) - _base_bytes(8, 228, 304, 3, 3)
    c5 = f(_lib.DTYPE_F16, 16, 228, 304, 1, 17, 36) - _base_bytes(16, 228, 304, 1, 17)
    assert c2 == 4 * 18 * 8 * 228 * 304 and 39.5e6 < c2 < 40.5e6
    assert c5 == 4 * 32 * 16 * 228 * 304 and 141e6 < c5 < 143e6


def test_workspace_sizes_bad_arguments():
    lib = _lib.get()
    f, g = lib.nlspn_backward_workspace_bytes_dtype, lib.nlspn_prop_step_backward_workspace_bytes_dtype
    for dt in (_lib.DTYPE_F32, _lib.DTYPE_F16):
        assert f(dt, 2, 24, 40, 3, 3, 6) > 0 and g(dt, 2, 24, 40, 3, 3) > 0
        for bad in ((0, 24, 40, 3, 3, 6), (2, 0, 40, 3, 3, 6), (2, 24, 0, 3, 3, 6), (2, 24, 40, 0, 3, 6),
                    (2, 24, 40, 3, 0, 6), (2, 24, 40, 3, 3, 0), (2, 24, 40, 1, 1, 6)):
            assert f(dt, *bad) == 0, bad
        for bad in ((0, 24, 40, 3, 3), (2, 0, 40, 3, 3), (2, 24, 0, 3, 3), (2, 24, 40, 0, 3), (2, 24, 40, 1, 1)):
            assert g(dt, *bad) == 0, bad
    for dt in (_lib.DTYPE_F64, 7, -1):
        assert f(dt, 2, 24, 40, 3, 3, 6) == 0 and g(dt, 2, 24, 40, 3, 3) == 0


@pytest.mark.parametrize("kh,kw", [(3, 3), (1, 17), (5, 5)])
def test_step_workspace_sizes(kh, kw):
    lib = _lib.get()
    g = lib.nlspn_prop_step_backward_workspace_bytes_dtype
    B, H, W, K = 2, 24, 40, kh * kw - 1
    assert g(_lib.DTYPE_F32, B, H, W, kh, kw) == lib.nlspn_prop_step_backward_workspace_bytes(B, H, W)
    assert g(_lib.DTYPE_F16, B, H, W, kh, kw) == 4 * B * H * W * (3 * K + 4)


P = ctypes.c_void_p(64)  # never dereferenced: validation fails first
HW = 16


def _section(dtype, **over):
    a = dict(dtype=dtype, pred_init=P, dep=P, conf=P, aff_raw=P, aff_bs=8 * HW, off_raw=P, off_bs=16 * HW, gamma=P,
             pred_inter=P, aff_norm=P, conf_eff=P, grad_pred=P, grad_pred_inter=P, grad_pred_init=P, grad_conf=P,
             grad_aff_raw=P, grad_aff_bs=0, grad_off_raw=P, grad_off_bs=0, grad_gamma=P, workspace=P, B=1, H=4, W=4,
             kh=3, kw=3, T=3, kind=3, flags=1, stream=None)
    a.update(over)
    lib = _lib.get()
    return lib.nlspn_propagate_backward(*a.values()), lib.nlspn_last_error().decode()


def _step(dtype, **over):
    a = dict(dtype=dtype, feat=P, conf=P, dep=P, aff=P, aff_bs=9 * HW, off_raw=P, off_bs=16 * HW, grad_out=P,
             grad_feat=P, grad_conf=P, grad_aff=P, grad_off=P, workspace=P, B=1, H=4, W=4, kh=3, kw=3, flags=1,
             stream=None)
    a.update(over)
    lib = _lib.get()
    return lib.nlspn_prop_step_backward(*a.values()), lib.nlspn_last_error().decode()


def _affnorm(dtype, **over):
    a = dict(dtype=dtype, aff_raw=P, aff_bs=8 * HW, gamma=P, grad_aff=P, grad_aff_raw=P, grad_gamma=P, workspace=P, B=1,
             K=8, H=4, W=4, kind=3, stream=None)
    a.update(over)
    lib = _lib.get()
    return lib.nlspn_affinity_normalize_backward(*a.values()), lib.nlspn_last_error().decode()


@pytest.mark.parametrize("entry", [_section, _step, _affnorm])
def test_unknown_dtype_is_refused(entry):
    for dt in (7, _lib.DTYPE_F64):
        rc, msg = entry(dt)
        assert rc == _lib.EUNSUPPORTED and "float32 or float16" in msg, (rc, msg)


REFUSALS = [
    (_section, dict(pred_init=None)), (_section, dict(workspace=None)), (_section, dict(grad_aff_raw=None)),
    (_section, dict(grad_conf=None)), (_section, dict(grad_off_raw=None)), (_section, dict(dep=None)),
    (_section, dict(aff_bs=8 * HW - 1)), (_section, dict(off_bs=16 * HW - 1)), (_section, dict(grad_aff_bs=8 * HW - 1)),
    (_section, dict(grad_off_bs=-1)), (_section, dict(T=0)), (_section, dict(kind=9)), (_section, dict(kh=2)),
    (_section, dict(B=0)), (_section, dict(kh=7, kw=7)),
    (_step, dict(feat=None)), (_step, dict(workspace=None)), (_step, dict(grad_conf=None)), (_step, dict(grad_off=None)),
    (_step, dict(aff_bs=9 * HW - 1)), (_step, dict(off_bs=16 * HW - 1)), (_step, dict(W=0)),
    (_affnorm, dict(aff_raw=None)), (_affnorm, dict(workspace=None)), (_affnorm, dict(aff_bs=8 * HW - 1)),
    (_affnorm, dict(kind=-1)), (_affnorm, dict(K=7)),
]


@pytest.mark.parametrize("i", range(len(REFUSALS)))
def test_refusals_do_not_depend_on_dtype(i):
    entry, over = REFUSALS[i]
    rc32, msg32 = entry(_lib.DTYPE_F32, **over)
    rc16, msg16 = entry(_lib.DTYPE_F16, **over)
    assert rc32 != 0 and (rc16, msg16) == (rc32, msg32), (over, rc32, msg32, rc16, msg16)
