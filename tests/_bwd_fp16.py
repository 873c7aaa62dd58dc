"""Inputs, references and bars of the float16 backward tests (tests/test_bwd_fp16_cases_cpu.py,
tests/test_gpu_backward_fp16_elem.py, tests/test_gpu_step_backward_fp16.py,
tests/test_gpu_backward_fp16_api.py).

Inputs are those of tests/_bwd_cases.py with every array rounded to float16, the upstream
gradients included.  Offsets are multiples of 1/64 below 128: exact in float16 below 32, and the CPU
test checks that beyond that the rounding still leaves every integer offset an integer and every
fractional one fractional, and that the kink margins of the rounded inputs stay above the guard.

Bars.  A float16 gradient element is the float32 value rounded once, so against the float32
entry on the same (widened) operands

    |float(g16) - g32| <= 2^-11 |g32| + 2^-25 + 2 (c X + Q)

one float16 rounding, half a subnormal step, and twice the float32 path's own allowed distance
from float64 (two float32 runs differ by the order of their float atomics): c, X and Q are
tests/test_gpu_backward_elem.py's.  gamma stays float32: |gg16 - gg32| <= 2 (c X + Q).
Elements whose bound X is 0 must be exactly 0.

The anchor cases take no float32 kernel for a reference: kind ASS at T = 1 with the raw
affinities scaled by a power of two until max sum |a| + 1e-4 < 1, so that the normalised
affinity equals the raw one, conf' is exact and no stored float16 intermediate enters the
gradient; the float64 oracle on the same inputs is then exact and the bar is
2^-11 |g64| + 2^-25 + c X + Q with c the operation-count ceiling at T = 1.
"""
import numpy as np

import _bwd_cases as bc

CHAIN = ["res_tiny_parts", "res_far", "res_odd", "res_T2", "res_noconf", "res_nopreserve", "res_AS", "res_ASS",
         "res_TC", "steps_split_clip", "onepass_longT", "onepass_env", "k17", "k5x5", "noffset"]
ANCHOR = ["res_ASS", "k17", "k5x5", "noffset"]
ARRAYS = ("pred_init", "dep", "conf", "aff", "off", "grad_pred", "grad_inter")
H_EPS, H_SUB = 2.0 ** -11, 2.0 ** -25  # one float16 rounding (relative), half a subnormal step

_cache = {}


def rounded_inputs(name):
    """grid_inputs(name) rounded to float16 and widened back to float32 (cls unchanged)."""
    key = ("in", name)
    if key not in _cache:
        s = bc.grid_inputs(name)
        _cache[key] = {k: (v if k == "cls" or v is None else v.astype(np.float16).astype(np.float32))
                       for k, v in s.items()}
    return _cache[key]


def chain_oracle(oracle, name):
    """(g64, X, info) of the float64 oracle on the rounded inputs of chain case `name`."""
    key = ("chain", name)
    if key not in _cache:
        oracle.set_threads(16)
        _cache[key] = bc.oracle_bound(oracle, name, rounded_inputs(name))
    return _cache[key]


def anchor_inputs(name):
    """The rounded inputs of `name` as the anchor runs them: T = 1 and the raw affinities times
    the power of two that brings max sum |a| to <= 0.5.  Returns (inputs, scale)."""
    key = ("ain", name)
    if key not in _cache:
        s = dict(rounded_inputs(name))
        m = float(np.abs(s["aff"].astype(np.float64)).sum(1).max())
        scale = 2.0 ** -int(np.ceil(np.log2(m / 0.5)))
        s["aff"] = (s["aff"] * np.float32(scale)).astype(np.float32)
        assert np.array_equal(s["aff"], s["aff"].astype(np.float16).astype(np.float32))  # still float16 values
        s["grad_inter"] = np.ascontiguousarray(s["grad_inter"][:1])
        _cache[key] = (s, scale)
    return _cache[key]


def anchor_kwargs(name):
    c = bc.CASES[name]
    return dict(kind="ASS", kh=c["kh"], kw=c["kw"], prop_time=1, preserve_input=c["preserve"], always_clip=c["clip"])


def anchor_oracle(oracle, name):
    """(g64, X, info) of the float64 oracle on the anchor inputs (gamma 1, kind ASS, T = 1)."""
    key = ("anchor", name)
    if key not in _cache:
        oracle.set_threads(16)
        c = bc.CASES[name]
        s, _ = anchor_inputs(name)
        f = lambda x: None if x is None else x.astype(np.float64)  # noqa: E731
        _cache[key] = oracle.propagate_backward_bound(
            f(s["pred_init"]), f(s["dep"]), f(s["conf"]) if c["conf"] else None, f(s["aff"]), f(s["off"]), 1.0,
            f(s["grad_pred"]), f(s["grad_inter"]), **anchor_kwargs(name))
    return _cache[key]


def anchor_ceiling(name):
    """bc.ceiling's operation count at T = 1."""
    c = bc.CASES[name]
    K = c["kh"] * c["kw"] - 1
    return ((4 * (K + 1) + 6) + 4 * K + 24 + 2) * 2.0 ** -24


def quantum(info, T, shape=None):
    """Q of tests/test_gpu_backward_elem.py: the scatter windows' fixed-point quantum, per image
    (broadcast to `shape`) or its maximum (gamma)."""
    Qb = 2.0 ** -50 * info["mass"].max(0) * T * max(1.0, info["amax"]) ** T
    if shape is None:
        return float(Qb.max())
    return np.broadcast_to(Qb.reshape(-1, 1, 1, 1), shape).ravel()


def worst(got, ref, allowed):
    """max |got - ref| / allowed over all elements (allowed > 0 everywhere), and its flat index."""
    got, ref, allowed = (np.asarray(a, np.float64).ravel() for a in (got, ref, allowed))
    with np.errstate(invalid="ignore"):
        r = np.abs(got - ref) / allowed
    r[np.isnan(r)] = np.inf
    i = int(np.argmax(r))
    return float(r[i]), i


def half_bar(ref, slack, gamma=False):
    """The allowed |float(g16) - ref| per element: one float16 rounding of `ref` plus `slack`
    (gamma stays float32: the slack alone)."""
    ref = np.abs(np.asarray(ref, np.float64).ravel())
    return np.asarray(slack, np.float64) + (0.0 if gamma else H_EPS * ref + H_SUB)
