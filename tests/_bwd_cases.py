"""Inputs and bars of the per-element backward tests, shared by tests/test_oracle_backward.py
(CPU: guard, bounds, the reference's own float32 error) and tests/test_gpu_backward_elem.py /
tests/test_gpu_dcn_elem.py (GPU: every element of every gradient against the float64 oracle).

Inputs.  grid_inputs() draws what synth() draws, on purpose at the places a float kernel and a
float64 reference can disagree about a branch:

  * offsets are multiples of 1/64 (|offset| < 128), so ``(y - ph + i) + off`` is exact in float32
    and float64 alike: the two never disagree on a floor or an in/out-of-image test;
  * most taps have a fractional part in [1/8, 7/8]; SHARE (5 %) of the taps each is forced onto
    integer coordinates in both axes / integer in one axis / exactly -1 / exactly H-1 (W-1) /
    exactly H (W) / inside (-1, 0) or (H-1, H) / far outside the image (one random axis for the
    border classes, the other axis stays a common tap);
  * pred_init has ~20 % exact zeros and ~10 % values <= -0.01 (clamp gates at equality and
    active with a margin);
  * raw affinities are |N(0,1)| + 0.01 (no |u_k| below the guard), a quarter of them negative in
    the `signed` cases (T = 4, so that max(1, sum |a|)^T keeps Q negligible), and pixels whose normaliser
    s lands within 1e-3 of the ASS/TGASS clamp at 1 have their affinities scaled by 1.25;
  * dep is sparse as in synth(); grad_pred and grad_inter are standard normal.

Every image is drawn from its own generator ``default_rng([seed, b, attempt])``; ``retry`` names
the images whose first draws put a pre-clamp value within the guard (found with the float64
oracle one image at a time, hard-coded below).  Guard (tests/test_oracle_backward.py): all
kink margins of every case >= GUARD.  No element is excluded from any comparison.

Bars.  R32[case][tensor] is the float32 oracle's own worst ``|g32 - g64| / X`` (X the
magnitude bound of oracle.propagate_backward_bound), measured on the CPU and asserted there
not to grow; the GPU bar is c = min(4 * r32, ceiling(case, tensor)).  The tanh kinds' affinity
gradient gets aff_slack() per element on top (the subtraction 1 - th^2, which X carries as one
factor), on the CPU and on the GPU alike.
"""
import numpy as np

GUARD = 1e-4
NONEXACT_GRAD = 3.2e38  # finite in float32 (max 3.4e38), 6 % above the exact-path limit 3.0e38
SHARE = 0.05
CLASSES = ("int2", "int1", "m1", "last", "end", "rim", "far")
TENSORS = ("pred_init", "aff", "offset", "confidence", "gamma")


def _gamma(kind, K):
    return {"TGASS": 0.5 * K, "TC": float(K)}.get(kind, 1.0)


def _case(B, H, W, T, kh=3, kw=3, kind="TGASS", conf=True, preserve=True, clip=False, offset=True, seed=0, retry=None,
          far20=False, env=None, form="fused", special=None, signed=False):
    return dict(B=B, H=H, W=W, T=T, kh=kh, kw=kw, kind=kind, conf=conf, preserve=preserve, clip=clip, offset=offset,
                seed=seed, retry=retry or {}, far20=far20, env=env or {}, form=form, special=special, signed=signed)


# name -> case.  All 3x3, K = 8, TGASS, confidence and preserve_input on unless noted.
CASES = {
    "res_tiny_parts": _case(2, 24, 40, 6, seed=1),
    "res_far": _case(2, 40, 64, 4, seed=2, far20=True),
    "res_one_part": _case(256, 48, 64, 3, seed=3),
    "res_two_parts": _case(128, 48, 64, 3, seed=4),
    "res_T2": _case(2, 48, 64, 2, seed=5),
    "res_T24": _case(2, 48, 64, 24, seed=6),
    "res_odd": _case(3, 19, 45, 5, seed=7),
    "res_noconf": _case(2, 24, 40, 4, seed=8, conf=False),
    "res_nopreserve": _case(2, 24, 40, 4, seed=9, preserve=False, signed=True),
    "res_AS": _case(2, 24, 40, 4, seed=10, kind="AS", signed=True),
    "res_ASS": _case(2, 24, 40, 4, seed=11, kind="ASS", signed=True),
    "res_TC": _case(2, 24, 40, 4, seed=12, kind="TC", signed=True),
    "steps_split_clip": _case(2, 24, 40, 6, seed=13, clip=True),
    "steps_split_manyB": _case(257, 8, 16, 3, seed=14),
    "onepass_longT": _case(1, 16, 32, 26, seed=15),
    "onepass_env": _case(2, 24, 40, 6, seed=16, env={"NLSPN_BWD_ONEPASS": "1"}),
    "k17": _case(2, 16, 48, 4, kh=1, kw=17, seed=17, signed=True),
    "k5x5": _case(2, 16, 32, 4, kh=5, kw=5, seed=18, clip=True),
    "k7x7": _case(1, 19, 24, 4, kh=7, kw=7, seed=19),
    "noffset": _case(2, 24, 40, 4, seed=20, offset=False),
    "step_op": _case(2, 24, 40, 5, seed=21, form="step_op"),
    "range": _case(2, 48, 64, 2, seed=22, special="range"),
    "nonexact": _case(2, 24, 40, 3, seed=23, special="nonexact"),
    # the compact batch of tests/_big_cases.py: the non-zero images of its periodic and sparse batches
    "big_compact": _case(4, 24, 32, 3, seed=24),
}
# images whose first draw(s) fall inside the guard: case -> {image: attempt}
RETRY = {
    "res_tiny_parts": {0: 2, 1: 1},
    "res_one_part": {6: 2, 7: 1, 13: 2, 16: 1, 24: 1, 26: 1, 31: 1, 32: 2, 50: 1, 54: 1, 68: 1, 71: 3, 78: 1,
        79: 1, 82: 1, 87: 2, 96: 1, 100: 1, 105: 1, 106: 1, 111: 1, 134: 1, 140: 2, 144: 2, 145: 1, 149: 1,
        150: 2, 153: 1, 157: 1, 161: 1, 164: 1, 167: 1, 177: 2, 178: 1, 179: 2, 183: 1, 190: 2, 193: 1, 205: 1,
        211: 2, 219: 1, 222: 1, 228: 1, 236: 1, 238: 6, 239: 1, 240: 1, 243: 2, 244: 1, 252: 2},
    "res_two_parts": {4: 1, 10: 1, 24: 1, 27: 1, 32: 1, 34: 1, 36: 1, 45: 1, 47: 2, 48: 1, 53: 1, 56: 1, 59: 1,
        65: 1, 71: 3, 79: 1, 80: 1, 81: 1, 99: 1, 108: 1, 111: 2, 115: 1},
    "res_T24": {0: 1, 1: 1},
    "res_odd": {0: 1},
    "res_nopreserve": {0: 3, 1: 6},
    "res_ASS": {0: 1},
    "steps_split_manyB": {4: 1, 22: 1, 25: 1, 38: 1, 47: 1, 54: 1, 56: 1, 69: 1, 77: 1, 79: 1, 97: 1, 105: 1,
        134: 1, 135: 2, 148: 1, 157: 1, 191: 1, 192: 1, 214: 1, 229: 1, 254: 1},
    "range": {0: 1, 1: 2},
    "big_compact": {1: 1},
}
for _n, _r in RETRY.items():
    CASES[_n]["retry"] = _r
# not a GPU case: the CPU pin "every term non-negative => bound == gradient" (kind AS)
AUX_CASES = {"nonneg": _case(2, 12, 14, 3, kind="AS", seed=99)}


def case_of(name):
    return CASES[name] if name in CASES else AUX_CASES[name]


def br_plan(B, H, W, cus, tmpdir):
    """The resident backward's partition (nlspn_plan.h br_plan) for a batch and a CU count:
    dict ok, Bl, py, px, PR, PC.  Host only: compiles tests/br_plan_query.cpp into `tmpdir`."""
    import os
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(tmpdir, "br_plan_query")
    if not os.path.exists(exe):
        cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
        assert cxx, "no host C++ compiler"
        out = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-I", os.path.join(root, "nlspn_eccv20_amd", "csrc"),
                              os.path.join(root, "tests", "br_plan_query.cpp"), "-o", exe],
                             capture_output=True, text=True)
        assert out.returncode == 0, out.stderr[-2000:]
    out = subprocess.run([exe, str(B), str(H), str(W), str(cus)], capture_output=True, text=True, env={})
    assert out.returncode == 0, out.stderr[-2000:]
    return dict(zip(("ok", "Bl", "py", "px", "PR", "PC"), (int(v) for v in out.stdout.split())))


def backward_form(name, cus, tmpdir):
    """The form nlspn_propagate_backward selects for a case on a device of `cus` CUs, restated
    from its rule (nlspn_prop_bwd.hip): "onepass" | "steps" (two-pass step launches) |
    ("resident", parts per image, pixels per thread)."""
    c = CASES[name]
    K = c["kh"] * c["kw"] - 1
    split = (c["env"].get("NLSPN_BWD_ONEPASS") != "1" and c["offset"] and (c["kh"], c["kw"]) == (3, 3)
             and c["T"] <= 3 * K)
    if not split:
        return "onepass"
    P = br_plan(c["B"], c["H"], c["W"], cus, tmpdir)
    if c["clip"] or c["T"] < 2 or not P["ok"] or P["Bl"] < c["B"]:
        return "steps"
    return ("resident", P["py"] * P["px"], -(-P["PR"] * P["PC"] // 1024))


def _axis_offsets(rng, base, n, cls, sel, sigma):
    """Offsets of one axis (multiples of 1/64) for base coordinates `base` (integers, any
    shape), image extent n; `cls` the tap class, `sel` True where the border classes act on
    this axis."""
    shape = base.shape
    whole = np.floor(rng.standard_normal(shape) * sigma)
    frac = rng.integers(8, 57, shape) / 64.0
    off = whole + frac                                            # common tap
    off = np.where((cls == 1) | ((cls == 2) & sel), whole, off)   # int2; int1 on the chosen axis
    lo = rng.random(shape) < 0.5
    tgt = np.where(cls == 3, -1.0, np.where(cls == 4, n - 1.0, float(n)))
    off = np.where(((cls >= 3) & (cls <= 5)) & sel, tgt - base, off)
    rim = np.where(lo, -1.0 + frac, n - 1.0 + frac)
    off = np.where((cls == 6) & sel, rim - base, off)
    dist = rng.integers(2, 11, shape) + frac
    far = np.where(lo, -1.0 - dist, n + dist)
    off = np.where((cls == 7) & sel, far - base, off)
    return off


def _image(c, b, attempt):
    H, W, kh, kw = c["H"], c["W"], c["kh"], c["kw"]
    K = kh * kw - 1
    rng = np.random.default_rng([c["seed"], b, attempt])
    f32 = np.float32
    pi = rng.uniform(0, 10.0, (1, H, W))
    r = rng.random((1, H, W))
    pi = np.where(r < 0.2, 0.0, np.where(r < 0.3, -(0.01 + rng.uniform(0, 2.0, (1, H, W))), pi)).astype(f32)
    dep = (rng.uniform(0, 10.0, (1, H, W)) * (rng.random((1, H, W)) < 0.05)).astype(f32)
    conf = rng.random((1, H, W)).astype(f32)
    aff = (np.abs(rng.standard_normal((K, H, W))) + 0.01).astype(f32)
    if c["signed"]:  # a quarter of the raw affinities negative: sign(u_k) = -1 in the normalisation backward
        aff = np.where(rng.random((K, H, W)) < 0.25, -aff, aff).astype(f32)
    if c["kind"] in ("ASS", "TGASS"):
        g = np.float64(np.float32(_gamma(c["kind"], K)))
        for _ in range(8):
            u = np.tanh(aff.astype(np.float64)) / (g + 1e-8) if c["kind"] == "TGASS" else aff.astype(np.float64)
            near = np.abs(np.abs(u).sum(0) + 1e-4 - 1.0) < 1e-3
            if not near.any():
                break
            aff = np.where(near[None], aff * f32(1.25), aff).astype(f32)
    out = {"pred_init": pi, "dep": dep, "conf": conf, "aff": aff, "off": None, "cls": None}
    if c["offset"]:
        ph, pw, ref = (kh - 1) // 2, (kw - 1) // 2, K // 2
        tap = np.array([k if k < ref else k + 1 for k in range(K)])
        by = (np.arange(H)[None, :, None] - ph + (tap // kw)[:, None, None]) + np.zeros((K, H, W))
        bx = (np.arange(W)[None, None, :] - pw + (tap % kw)[:, None, None]) + np.zeros((K, H, W))
        r = rng.random((K, H, W))
        cls = np.where(r < len(CLASSES) * SHARE, np.floor(r / SHARE).astype(int) + 1, 0)  # 0: common tap
        axis = rng.random((K, H, W)) < 0.5
        oh = _axis_offsets(rng, by, H, cls, axis, 2.0)
        ow = _axis_offsets(rng, bx, W, cls, ~axis, 2.0)
        if c["far20"]:
            r = rng.random((K, H, W))
            oh = oh + np.where(r < 0.05, 20.0, np.where(r < 0.10, -20.0, 0.0))
            r = rng.random((K, H, W))
            ow = ow + np.where(r < 0.05, 20.0, np.where(r < 0.10, -20.0, 0.0))
        off = np.stack([oh, ow], 1).reshape(2 * K, H, W)
        assert np.abs(off).max() < 128 and np.array_equal(off * 64, np.round(off * 64))
        out["off"] = off.astype(f32)
        out["cls"] = cls.astype(np.int8)
    return out


def grid_inputs(name):
    """The inputs of case `name`: dict of float32 arrays pred_init, dep, conf (B,1,H,W), aff
    (B,K,H,W), off (B,2K,H,W) or None, grad_pred (B,1,H,W), grad_inter (T,B,1,H,W), and
    cls (B,K,H,W) int8, the class of every tap (0 common, 1.. = CLASSES)."""
    c = case_of(name)
    B, H, W, T = c["B"], c["H"], c["W"], c["T"]
    imgs = [_image(c, b, c["retry"].get(b, 0)) for b in range(B)]
    s = {k: (None if imgs[0][k] is None else np.ascontiguousarray(np.stack([im[k] for im in imgs], 0)))
         for k in ("pred_init", "dep", "conf", "aff", "off", "cls")}
    rng = np.random.default_rng([c["seed"], 1 << 20])
    gp = rng.standard_normal((B, 1, H, W)).astype(np.float32)
    gi = rng.standard_normal((T, B, 1, H, W)).astype(np.float32)
    if c["special"] == "range":      # image 0's left half: upstream gradients 2^30 times the rest
        gp[0, :, :, :W // 2] *= np.float32(2.0 ** 30)
        gi[:, 0, :, :, :W // 2] *= np.float32(2.0 ** 30)
    if c["special"] == "nonexact":
        # one upstream gradient that takes its window's mass past the kernels' 3e38 threshold with
        # margin: the pixel scatters |go| (|a_ref| + sum |a_k|) >= |go| (a_ref + sum a_k = 1)
        gp[0, 0, H // 2, W // 2] = np.float32(NONEXACT_GRAD)
    s["grad_pred"], s["grad_inter"] = gp, gi
    return s


def oracle_kwargs(name):
    c = case_of(name)
    return dict(kind=c["kind"], kh=c["kh"], kw=c["kw"], prop_time=c["T"], preserve_input=c["preserve"],
                always_clip=c["clip"])


def gamma_of(name):
    c = case_of(name)
    return float(np.float32(_gamma(c["kind"], c["kh"] * c["kw"] - 1)))


def oracle_bound(oracle, name, s, dtype=np.float64):
    """(grads, bounds, info) of the oracle's backward with the magnitude pass, in `dtype`, on
    the float32 inputs `s` of grid_inputs(name)."""
    c = case_of(name)
    cv = lambda x: None if x is None else x.astype(dtype)  # noqa: E731
    return oracle.propagate_backward_bound(
        cv(s["pred_init"]), cv(s["dep"]), cv(s["conf"]) if c["conf"] else None, cv(s["aff"]), cv(s["off"]),
        gamma_of(name), cv(s["grad_pred"]), cv(s["grad_inter"]), **oracle_kwargs(name))


TANH_ULP = 2  # float tanhf: within 2 ulp (glibc's is within 1; the HIP device library documents 2)


def ceiling(name, tensor):
    """(n + 2) * 2^-24, n the rounded operations on the longest path to one element:
    T * (4 (K+1) + 6) through the recurrence [per iteration and tap: the tap's product, its
    two bilinear weights and the accumulation; per iteration the blend, gate, confidence
    product and upstream add] plus 4 K + 24 through the normalisation backward.  gamma is in
    addition one sequential float sum over every pixel's K terms, + B H W K: a worst-case count
    that is far above what a sum of mixed signs loses, so for gamma c = 4 * R32 is what binds."""
    c = case_of(name)
    K = c["kh"] * c["kw"] - 1
    n = c["T"] * (4 * (K + 1) + 6) + 4 * K + 24
    if tensor == "gamma":
        n += c["B"] * c["H"] * c["W"] * K
    return (n + 2) * 2.0 ** -24


def aff_slack(name, info):
    """Per-element allowance for the one subtraction the magnitude pass cannot see: the tanh
    kinds' raw-affinity gradient ends in the factor 1 - th^2, carried in X as |1 - th^2|.  With th
    good to TANH_ULP ulp and th^2 rounded once, the factor is off by (2 TANH_ULP + 1) 2^-24 th^2,
    so the element by that times b_gu / d = info["aff_cond"] (the float64 oracle's).  It matters
    only where tanh saturates (|a| > 3: 1 - th^2 < 1e-2); elsewhere it is below c * X, and c
    stays the operation count's for every element.  0 for AS / ASS."""
    if case_of(name)["kind"] not in ("TGASS", "TC"):
        return 0.0
    return (2 * TANH_ULP + 1) * 2.0 ** -24 * np.asarray(info["aff_cond"], np.float64).ravel()


def tensors_of(name):
    c = case_of(name)
    return [t for t in TENSORS if not ((t == "offset" and not c["offset"]) or (t == "confidence" and not c["conf"])
                                       or (t == "gamma" and c["kind"] != "TGASS"))]


def checked_mask(name, tensor, got):
    """Elements of `got` (float32 results: the kernels', or the float32 oracle's) that enter the
    comparison.  Everything, except in `nonexact`: there the 3.2e38 gradient takes float32 itself
    to inf / NaN in parts of image 0 and possibly in gamma (one sum over both images), so image 0
    and gamma are compared where `got` is finite; image 1 is compared whole and must be finite."""
    if case_of(name)["special"] != "nonexact":
        return None
    m = np.isfinite(np.asarray(got))
    if tensor != "gamma":
        assert np.all(m[1:]), f"{tensor}: non-finite values in the image without the 3.2e38 gradient"
    return m


def ratio(got, g64, bound, mask=None, Q=0.0):
    """max_e (|got - g64| - Q) / X over X > 0, and whether every X == 0 element is exactly 0
    in both.  Returns (ratio, zeros_ok, flat index of the worst element)."""
    got, g64, bound = (np.asarray(a, np.float64).ravel() for a in (got, g64, bound))
    sel = np.ones(bound.shape, bool) if mask is None else np.asarray(mask).ravel()
    pos = sel & (bound > 0)
    zero = sel & (bound == 0)
    zeros_ok = bool(np.all(got[zero] == 0) and np.all(g64[zero] == 0))
    if not pos.any():
        return 0.0, zeros_ok, -1
    r = np.full(bound.shape, -np.inf)
    q = Q[pos] if np.ndim(Q) else Q  # one quantum, or one per element
    with np.errstate(invalid="ignore", over="ignore"):
        r[pos] = (np.abs(got[pos] - g64[pos]) - q) / bound[pos]
    r[np.isnan(r)] = np.inf
    i = int(np.argmax(r))
    return float(max(r[i], 0.0)), zeros_ok, i


# The float32 oracle's own worst (|g32 - g64| - aff_slack) / X per case and tensor (measured on the CPU,
# asserted not to grow by tests/test_oracle_backward.py::test_reference_float32_meets_bar).
R32 = {
    "res_tiny_parts": {"pred_init": 5.9e-07, "aff": 2.3e-07, "offset": 4.0e-07, "confidence": 4.2e-07, "gamma": 6.4e-10},
    "res_far": {"pred_init": 1.3e-06, "aff": 2.5e-07, "offset": 4.1e-07, "confidence": 1.1e-06, "gamma": 1.2e-08},
    "res_one_part": {"pred_init": 2.8e-06, "aff": 1.1e-06, "offset": 1.6e-06, "confidence": 1.8e-06, "gamma": 1.1e-09},
    "res_two_parts": {"pred_init": 8.1e-06, "aff": 6.0e-07, "offset": 8.4e-07, "confidence": 2.2e-06, "gamma": 4.0e-09},
    "res_T2": {"pred_init": 7.8e-07, "aff": 3.1e-07, "offset": 5.6e-07, "confidence": 7.4e-07, "gamma": 5.2e-09},
    "res_T24": {"pred_init": 9.7e-07, "aff": 1.8e-07, "offset": 3.0e-07, "confidence": 5.8e-07, "gamma": 1.6e-09},
    "res_odd": {"pred_init": 1.3e-06, "aff": 1.9e-07, "offset": 3.9e-07, "confidence": 7.9e-07, "gamma": 4.1e-09},
    "res_noconf": {"pred_init": 5.5e-07, "aff": 2.2e-07, "offset": 1.9e-07, "gamma": 5.9e-10},
    "res_nopreserve": {"pred_init": 2.8e-07, "aff": 4.5e-07, "offset": 6.3e-07, "confidence": 4.7e-07, "gamma": 9.8e-10},
    "res_AS": {"pred_init": 6.7e-07, "aff": 2.4e-07, "offset": 5.1e-07, "confidence": 3.1e-07},
    "res_ASS": {"pred_init": 5.6e-07, "aff": 2.6e-07, "offset": 3.9e-07, "confidence": 3.8e-07},
    "res_TC": {"pred_init": 2.7e-07, "aff": 7.8e-07, "offset": 3.0e-07, "confidence": 9.1e-07},
    "steps_split_clip": {"pred_init": 9.2e-07, "aff": 2.5e-07, "offset": 4.3e-07, "confidence": 7.9e-07, "gamma": 9.6e-09},
    "steps_split_manyB": {"pred_init": 5.9e-06, "aff": 3.5e-07, "offset": 1.3e-06, "confidence": 6.0e-06, "gamma": 4.3e-09},
    "onepass_longT": {"pred_init": 6.5e-07, "aff": 1.4e-07, "offset": 2.0e-07, "confidence": 3.6e-07, "gamma": 1.2e-09},
    "onepass_env": {"pred_init": 1.2e-06, "aff": 2.6e-07, "offset": 2.9e-07, "confidence": 7.7e-07, "gamma": 1.7e-09},
    "k17": {"pred_init": 2.0e-07, "aff": 6.0e-07, "offset": 4.6e-07, "confidence": 2.5e-07, "gamma": 2.4e-09},
    "k5x5": {"pred_init": 1.7e-06, "aff": 5.6e-07, "offset": 4.0e-07, "confidence": 7.4e-07, "gamma": 2.1e-09},
    "k7x7": {"pred_init": 1.3e-06, "aff": 4.1e-07, "offset": 9.3e-07, "confidence": 1.1e-06, "gamma": 4.5e-09},
    "noffset": {"pred_init": 3.3e-07, "aff": 1.7e-07, "confidence": 2.5e-07, "gamma": 4.6e-09},
    "step_op": {"pred_init": 2.2e-06, "aff": 3.1e-07, "offset": 3.7e-07, "confidence": 1.7e-06, "gamma": 2.2e-10},
    "range": {"pred_init": 7.7e-07, "aff": 8.9e-07, "offset": 1.6e-06, "confidence": 9.2e-07, "gamma": 3.2e-09},
    "nonexact": {"pred_init": 2.2e-06, "aff": 3.2e-07, "offset": 4.3e-07, "confidence": 8.9e-07, "gamma": 8.0e-08},
    "big_compact": {"pred_init": 2.4e-06, "aff": 3.7e-07, "offset": 4.0e-07, "confidence": 2.0e-06, "gamma": 4.2e-09},
}

# ------------------------------------------------------------------ DCN (seam 2)
DCN_TENSORS = ("input", "offset", "mask", "weight", "bias")


def dcn_cases():
    from test_gpu_dcn import CASES as dcn  # the six geometries of the norm test, unchanged
    return dcn


def dcn_inputs(seed, C, Cout, group, dg, kh, kw, stride, pad, dil, B=2, H=13, W=17):
    """test_gpu_dcn._case() with offsets on the 1/64 grid and the tap classes above (the sampling
    position is ho*s - pad + i*d + off: integers plus the offset, so exact in both precisions)."""
    rng = np.random.default_rng(seed)
    Ho = (H + 2 * pad[0] - (dil[0] * (kh - 1) + 1)) // stride[0] + 1
    Wo = (W + 2 * pad[1] - (dil[1] * (kw - 1) + 1)) // stride[1] + 1
    f32 = np.float32
    KK = kh * kw
    t = np.arange(KK)
    shape = (B, dg, KK, Ho, Wo)
    by = (np.arange(Ho)[:, None] * stride[0] - pad[0] + (t // kw)[:, None, None] * dil[0]) + np.zeros(shape)
    bx = (np.arange(Wo)[None, :] * stride[1] - pad[1] + (t % kw)[:, None, None] * dil[1]) + np.zeros(shape)
    r = rng.random(shape)
    cls = np.where(r < len(CLASSES) * SHARE, np.floor(r / SHARE).astype(int) + 1, 0)
    axis = rng.random(shape) < 0.5
    oh = _axis_offsets(rng, by, H, cls, axis, 2.0)
    ow = _axis_offsets(rng, bx, W, cls, ~axis, 2.0)
    off = np.stack([oh, ow], 3).reshape(B, dg * 2 * KK, Ho, Wo)
    assert np.abs(off).max() < 128 and np.array_equal(off * 64, np.round(off * 64))
    return (rng.standard_normal((B, C, H, W)).astype(f32), rng.standard_normal((Cout, C // group, kh, kw)).astype(f32),
            rng.standard_normal((Cout,)).astype(f32), off.astype(f32),
            rng.random((B, dg * KK, Ho, Wo)).astype(f32), rng.standard_normal((B, Cout, Ho, Wo)).astype(f32))


def dcn_ceiling(case, tensor, B=2, H=13, W=17):
    """(n + 2) * 2^-24 with n the longest sum of that gradient: grad_weight and grad_bias
    B Ho Wo terms; grad_input Cout/group kh kw 4 terms (every tap's corners into one cell, each
    a column of Cout/group products); grad_offset and grad_mask C/dg terms of a Cout/group
    column, plus the 8 operations of the bilinear / coordinate weight."""
    C, Cout, group, dg, kh, kw, stride, pad, dil = case
    Ho = (H + 2 * pad[0] - (dil[0] * (kh - 1) + 1)) // stride[0] + 1
    Wo = (W + 2 * pad[1] - (dil[1] * (kw - 1) + 1)) // stride[1] + 1
    opg = Cout // group
    n = {"weight": B * Ho * Wo + 8, "bias": B * Ho * Wo, "input": opg * kh * kw * 4 + 8,
         "offset": (C // dg) * (opg + 2) + 8, "mask": (C // dg) * (opg + 1) + 8}[tensor]
    return (n + 2) * 2.0 ** -24


# float32 oracle's own worst |g32 - g64| / X for the six CASES of tests/test_gpu_dcn.py, in order
DCN_R32 = [
    {"input": 1.5e-07, "offset": 2.1e-07, "mask": 1.7e-07, "weight": 4.7e-08, "bias": 1.7e-08},
    {"input": 1.6e-07, "offset": 2.0e-07, "mask": 1.8e-07, "weight": 7.9e-08, "bias": 1.1e-08},
    {"input": 1.4e-07, "offset": 2.0e-07, "mask": 1.7e-07, "weight": 9.8e-08, "bias": 2.1e-08},
    {"input": 1.3e-07, "offset": 1.7e-07, "mask": 1.6e-07, "weight": 4.5e-08, "bias": 2.5e-08},
    {"input": 1.8e-07, "offset": 2.4e-07, "mask": 2.0e-07, "weight": 9.5e-08, "bias": 5.8e-09},
    {"input": 2.5e-07, "offset": 2.3e-07, "mask": 1.5e-07, "weight": 1.2e-07, "bias": 4.8e-08},
]
