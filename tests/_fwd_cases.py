"""Inputs and the reference of the per-element forward tests, shared by tests/test_fwd_cases_cpu.py
(CPU: the reference is the oracle's loop, the inputs are not degenerate, the affinity bar),
tests/test_gpu_forward_elem.py (GPU: every iterate of every forward form bit for bit) and
tests/test_gpu_step_fp16.py (one fp16 step on the same inputs).

Inputs.  Every input set is B images of tests/_bwd_cases.py (_image, unchanged: offsets on the
1/64 grid with the tap classes int2, int1, m1, last, end, rim, far; pred_init with exact zeros and
negative values) and, where the set has offsets, ONE MORE batch item, the ramp image (its other
planes are _bwd_cases._image(c, B, 0), an image index no _bwd_cases case draws).

The ramp.  For tap k (raw index, the reference tap left out) at pixel (y, x) one axis - rows for
even k, columns for odd k - gets the offset

    d = ((x + 3 y + 5 k) mod (4 D + 1)) / 2 - D          (half-integer steps from -D to +D)

and the other axis a common tap: a whole part in -2..2 plus a fraction in [8/64, 56/64], both
deterministic in (x, y, k).  So along the ramp axis a tap lands on integers and half-integers at
every distance up to D from its base cell: exactly on, half a cell inside and a cell beyond every
edge of every LDS window, whatever the build's tile or part geometry, without this file knowing it.
The cycle 4 D + 1 is odd, hence coprime to every tile width, part width and the quad lanes: every
lane position meets every distance.  |offset| < 128 and multiples of 1/64 hold as in _bwd_cases.

D = 30.  The window rims of the forward builds, in cells beyond the tile or part that owns the
pixel (nlspn_eccv20_amd/csrc):
  * step kernels (nlspn_prop_fwd.hip select_step, RY / RX of prop_step_kernel): 3x3, 5x5, 7x7
    8 / 8; 1x17 scalar 8 / 16; 1x17 vector 10 / 20 - the largest;
  * resident kernel, fixed halo (nlspn_plan.h): rows res_ry(kh) = kResRY + (kh - 3) / 2 = 8 (3x3,
    1x17), 9 (5x5); columns 4 res_rxq(kw) = 4 (kResRXQ + ((kw - 3) / 2 + 3) / 4) = 8 (3x3), 12 (5x5),
    16 (1x17), plus kResPadX = 4 zero columns: at most 20;
  * resident kernel, dynamic window: the taps' own extent, no fixed rim (a ramp makes it the whole
    image, or too large for LDS: then the fixed halo and the general path).
A tap's base cell is up to PW = 8 columns (1x17) on the other side of its pixel, so a ramp offset
must reach 20 + 8 to arrive at the widest rim from the far side, and 2 more to pass it by two
cells: D = 20 + 8 + 2 = 30, cycle 121.

The reference.  reference() composes, in float32, exactly what oracle.propagate runs (checked bit
for bit on the CPU, tests/test_fwd_cases_cpu.py): the prologue blends in numpy float32, then T
times oracle.mdcn_c1 (oracle.prop_noffset without offsets), the preserve blend and the clamp.  It
takes the normalised affinities as an argument: fed the GPU's own `aff` output it says what every
iterate must be bit for bit, whatever tanhf the device has (the kernels are built with
-ffp-contract=off and issue the oracle's IEEE sequence).

The affinity bar.  A32[kind][K] is the float32 oracle's own worst |a32 - a64| / X over every input
set of that kind and K (X = |a_k| for the K taps, 1 + sum |a_k| for the reference tap), measured on the
CPU and asserted there not to grow and to stay under aff_ceiling(K) = (TANH_ULP + K + 4) 2^-24
[per tap: tanh, the division by gamma, the division by the sum of K rounded terms plus 1e-4; the
reference tap: K additions and the subtraction].  The GPU bar is min(4 A32, ceiling).
"""
import numpy as np

import _bwd_cases as bc

D = 30
CYCLE = 4 * D + 1
RAMP = -1  # the ramp image's entry in `cls`


# name -> the _bwd_cases case its images are drawn from (T: the most iterations any run takes).
# B counts the _bwd_cases images; with offsets the ramp image comes on top (B + 1 on the device).
INPUTS = {
    "g24x40": bc._case(2, 24, 40, 6, seed=101),                       # W % 4 == 0: vector kernels, resident
    "g19x45": bc._case(3, 19, 45, 6, seed=102),                       # W % 4 != 0: the scalar step kernel
    "k17": bc._case(2, 16, 48, 4, kh=1, kw=17, seed=103, signed=True),
    "k5x5": bc._case(2, 16, 32, 4, kh=5, kw=5, seed=104, clip=True),
    "k7x7": bc._case(1, 19, 24, 4, kh=7, kw=7, seed=105),
    "noffset": bc._case(2, 24, 40, 4, seed=106, offset=False),
    "rt32x128": bc._case(2, 32, 128, 5, seed=107),                    # the run-time-thread-count build
    "c48x192": bc._case(1, 48, 192, 5, seed=108),                     # the 576-thread build
    "split100x120": bc._case(1, 100, 120, 4, seed=109),               # the split-quad builds
    "wide28x160": bc._case(1, 28, 160, 5, kh=1, kw=17, seed=110),     # 1x17, two threads per quad
    "r5x5_24x64": bc._case(1, 24, 64, 4, kh=5, kw=5, seed=111),       # the resident 5x5 build
    "groups240x1216": bc._case(3, 240, 1216, 3, seed=112),            # two image groups in one launch
    "far40x64": bc._case(2, 40, 64, 4, seed=113, far20=True),         # taps leave the LDS window
    "AS": bc._case(2, 24, 40, 4, seed=114, kind="AS", signed=True),
    "ASS": bc._case(2, 24, 40, 4, seed=115, kind="ASS", signed=True),
    "TC": bc._case(2, 24, 40, 4, seed=116, kind="TC", signed=True),
    "noconf": bc._case(2, 24, 40, 4, seed=117, conf=False),
    "nopreserve": bc._case(2, 24, 40, 4, seed=118, preserve=False, signed=True),
    "clip": bc._case(2, 24, 40, 4, seed=119, clip=True),
    "T24": bc._case(2, 48, 64, 24, seed=120),
}


def gamma_of(name):
    c = INPUTS[name]
    return float(np.float32(bc._gamma(c["kind"], c["kh"] * c["kw"] - 1)))


def ramp_offsets(H, W, kh, kw):
    """(off (2K, H, W), dist (K, H, W)) of the ramp image, float64: the raw offsets (dh plane 2k,
    dw plane 2k + 1) and the ramp distance d of every tap."""
    K = kh * kw - 1
    k = np.arange(K)[:, None, None]
    y = np.arange(H)[None, :, None]
    x = np.arange(W)[None, None, :]
    d = ((x + 3 * y + 5 * k) % CYCLE) / 2.0 - D
    common = ((2 * x + y + 3 * k) % 5 - 2) + (8 + (7 * x + 11 * y + 13 * k) % 49) / 64.0
    rows = (k % 2 == 0) & np.ones((K, H, W), bool)
    oh = np.where(rows, d, common)
    ow = np.where(rows, common, d)
    off = np.stack([oh, ow], 1).reshape(2 * K, H, W)
    assert np.abs(off).max() < 128 and np.array_equal(off * 64, np.round(off * 64))
    return off, d + np.zeros((K, H, W))


TILE = 64  # _bwd_cases._image keeps |offset| < 128 up to about this extent


def _drawn_image(c, b):
    """Image b of case c from _bwd_cases._image.  Its border classes put a tap as far as the whole
    image away, so an image above TILE rows or columns is drawn as TILE x TILE tiles, each a
    _bwd_cases image of its own generator (image index 1000 (tile + 1) + b), laid side by side:
    offsets are relative, so every tile keeps its taps; the border classes of an outer tile land on
    the image's border, those of an inner tile on a tile seam (integer coordinates inside the
    image).  classify() names what a tap is from where it lands."""
    H, W = c["H"], c["W"]
    if H <= TILE and W <= TILE:
        return bc._image(c, b, 0)
    rows = []
    n = 0
    for y0 in range(0, H, TILE):
        row = []
        for x0 in range(0, W, TILE):
            n += 1
            row.append(bc._image(dict(c, H=min(TILE, H - y0), W=min(TILE, W - x0)), 1000 * n + b, 0))
        rows.append({k: (None if row[0][k] is None else np.concatenate([t[k] for t in row], 2)) for k in row[0]})
    return {k: (None if rows[0][k] is None else np.concatenate([r[k] for r in rows], 1)) for k in rows[0]}


def classify(h, w, H, W):
    """The _bwd_cases classes a tap at (h, w) belongs to, from where it lands: an int array of bit
    masks, bit i = _bwd_cases.CLASSES[i]."""
    ih, iw = h == np.floor(h), w == np.floor(w)
    valid = (h > -1) & (h < H) & (w > -1) & (w < W)
    rim = lambda a, n: ((a > -1) & (a < 0)) | ((a > n - 1) & (a < n))  # noqa: E731
    far = lambda a, n: (a <= -3) | (a >= n + 2)  # noqa: E731
    flags = (ih & iw & valid, ih ^ iw, (h == -1) | (w == -1), (h == H - 1) | (w == W - 1), (h == H) | (w == W),
             rim(h, H) | rim(w, W), far(h, H) | far(w, W))
    return sum(f.astype(np.int32) << i for i, f in enumerate(flags))


def class_names(mask):
    return [n for i, n in enumerate(bc.CLASSES) if int(mask) >> i & 1]


_cache = {}


def inputs(name):
    """The inputs of set `name` (computed once, shared, never written): float32 pred_init, dep,
    conf (Bt, 1, H, W), aff (Bt, K, H, W), off (Bt, 2K, H, W) or None; cls (Bt, K, H, W) int8, the
    class every tap was drawn as (0 common, 1.. = _bwd_cases.CLASSES, RAMP in the ramp image); dist
    (K, H, W), the ramp image's distances, or None.  Bt = B + 1 with offsets (the ramp image is
    the last item), else B."""
    if name in _cache:
        return _cache[name]
    c = INPUTS[name]
    imgs = [_drawn_image(c, b) for b in range(c["B"])]
    dist = None
    if c["offset"]:
        r = _drawn_image(c, c["B"])
        off, dist = ramp_offsets(c["H"], c["W"], c["kh"], c["kw"])
        r["off"] = off.astype(np.float32)
        r["cls"] = np.full(r["cls"].shape, RAMP, np.int8)
        imgs.append(r)
    s = {k: (None if imgs[0][k] is None else np.ascontiguousarray(np.stack([im[k] for im in imgs], 0)))
         for k in ("pred_init", "dep", "conf", "aff", "off", "cls")}
    for v in s.values():
        if v is not None:
            v.setflags(write=False)
    s["dist"] = dist
    _cache[name] = s
    return s


def tap_coords(name, s):
    """(h_im, w_im), each (Bt, K, H, W) float64 (exact: integers plus multiples of 1/64)."""
    c = INPUTS[name]
    kh, kw = c["kh"], c["kw"]
    K = kh * kw - 1
    tap = np.array([k if k < K // 2 else k + 1 for k in range(K)])
    by = np.arange(c["H"])[None, :, None] - (kh - 1) // 2 + (tap // kw)[:, None, None]
    bx = np.arange(c["W"])[None, None, :] - (kw - 1) // 2 + (tap % kw)[:, None, None]
    off = s["off"].astype(np.float64)
    return by[None] + off[:, 0::2], bx[None] + off[:, 1::2]


def prologue(name, s):
    """The section's prologue in numpy float32 (nlspnmodel.py:328-348, as oracle.propagate):
    (p0, blended confidence or None)."""
    c = INPUTS[name]
    one = np.float32(1.0)
    p = s["pred_init"].copy()
    conf = s["conf"].copy() if c["conf"] else None
    if c["preserve"]:
        m = (s["dep"] > 0).astype(np.float32)
        p = (one - m) * p + m * s["dep"]
        if conf is not None:
            conf = (one - m) * conf + m
    if c["clip"]:
        p = np.where(p < 0, np.float32(0), p)
    return p, conf


def reference(oracle, name, s, aff_norm, off_ins, conf_b, T=None, p0=None):
    """The oracle's loop, composed: (iterates (T, Bt, 1, H, W), pred), float32.  aff_norm
    (Bt, K+1, H, W), off_ins (Bt, 2(K+1), H, W) or None and conf_b (the blended confidence, or
    None) are the prologue's outputs as the caller has them (the oracle's, or the GPU's own)."""
    c = INPUTS[name]
    T = c["T"] if T is None else T
    one = np.float32(1.0)
    f32 = lambda a: None if a is None else np.ascontiguousarray(a, np.float32)  # noqa: E731
    aff_norm, off_ins, conf_b = f32(aff_norm), f32(off_ins), f32(conf_b)
    p = prologue(name, s)[0] if p0 is None else f32(p0)
    m = (s["dep"] > 0).astype(np.float32) if c["preserve"] else None
    inter = np.empty((T,) + p.shape, np.float32)
    for t in range(T):
        f = p * conf_b if conf_b is not None else p
        if off_ins is not None:
            p = oracle.mdcn_c1(f, off_ins, aff_norm, c["kh"], c["kw"])
        else:
            p = oracle.prop_noffset(f, aff_norm)
        if m is not None:
            p = (one - m) * p + m * s["dep"]
        if c["clip"]:
            p = np.where(p < 0, np.float32(0), p)
        inter[t] = p
    pred = p if c["clip"] else np.where(p < 0, np.float32(0), p)
    return inter, pred


def oracle_propagate(oracle, name, s, dtype=np.float32, T=None):
    c = INPUTS[name]
    cv = lambda x: None if x is None else x.astype(dtype)  # noqa: E731
    return oracle.propagate(cv(s["pred_init"]), cv(s["dep"]), cv(s["conf"]) if c["conf"] else None, cv(s["aff"]),
                            cv(s["off"]), gamma_of(name), kind=c["kind"], kh=c["kh"], kw=c["kw"],
                            prop_time=c["T"] if T is None else T, preserve_input=c["preserve"], always_clip=c["clip"])


# ------------------------------------------------------------------ the affinity bar
def aff_ceiling(K):
    return (bc.TANH_ULP + K + 4) * 2.0 ** -24


def aff_ratios(name, got, a64):
    """Per element |got - a64| / X of normalised affinities `got` (Bt, K+1, H, W) against the
    float64 normalisation a64 of the same raw planes: (ratio array, worst over the K taps, worst
    over the reference tap).  An element whose X is 0 must be exactly 0 (ratio inf otherwise)."""
    c = INPUTS[name]
    K = c["kh"] * c["kw"] - 1
    ref = K // 2
    a64 = np.asarray(a64, np.float64)
    X = np.abs(a64)
    taps = np.arange(K + 1) != ref
    X[:, ref] = 1.0 + X[:, taps].sum(1)
    err = np.abs(np.asarray(got, np.float64) - a64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(X > 0, err / X, np.where(err == 0, 0.0, np.inf))
    return r, float(r[:, taps].max()), float(r[:, ref].max())


def aff_float64(oracle, name, s):
    c = INPUTS[name]
    return oracle.affinity_normalization(s["aff"].astype(np.float64), c["kind"], gamma_of(name))


def aff_bar(name):
    """(c for the K taps, c for the reference tap) of the GPU check: min(4 A32, ceiling)."""
    c = INPUTS[name]
    K = c["kh"] * c["kw"] - 1
    return tuple(min(4.0 * v, aff_ceiling(K)) for v in A32[c["kind"]][K])


# The float32 oracle's own worst |a32 - a64| / X per affinity kind and K, (K taps, reference tap), over
# every input set of that kind and K (measured on the CPU; tests/test_fwd_cases_cpu.py::test_affinity_bar
# asserts it does not grow and stays under aff_ceiling).
A32 = {
    "TGASS": {8: (3.7e-07, 1.6e-07), 16: (3.8e-07, 1.8e-07), 24: (4.1e-07, 1.9e-07), 48: (5.5e-07, 2.1e-07)},
    "TC": {8: (1.6e-07, 5.8e-08)},
    "AS": {8: (2.3e-07, 1.2e-07)},
    "ASS": {8: (2.3e-07, 1.4e-07)},
}
