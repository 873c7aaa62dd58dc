"""Cases, seeded operands, float64 references and bars of the head epilogue's backward
(csrc/nlspn_heads_bwd.h; include/nlspn_prop.h: nlspn_head_backward_pre, the nlspn_gconv_dgrad
launch of the two wide data gradients, nlspn_head_dgrad_single, nlspn_head_wgrad), shared by
tests/test_heads_bwd_cpu.py (CPU: the references against torch's double autograd of the
reference's op sequence, the plan mirror against the library) and
tests/test_gpu_heads_bwd_elem.py (GPU: every element of every output through the C ABI).

Notation: C channels per source, R = nout + 2 rows in the forward kernel's column order
(0..nout-1 off_aff_dec0, nout id_dec0, nout + 1 cf_dec0).

References: explicit float64 sums on the exact f32 values the device gets (shifted slices, one
einsum per tap), written from the definitions, never from the packing helpers.

Bars (the project's, tests/_gconv_bwd_cases.py; none is derived from the kernels under test):
    gpre    rows < nout and the ReLU row bit-equal; the sigmoid row |got - ref| <= 8 * 2^-24 |ref|
    dgrad   |got - ref| <= c sum |w||gpre|, c = min(2e-6, (n + 4) 2^-24), n = 9 R (d_fe1),
            9 nout (d_fd_oa), 9 (d_fd_id, d_fd_cf)
    dW      |got - ref| <= c sum |gpre||src|, c = min(2e-6, (n + nsl + 2) 2^-24), n = B H W, nsl the
            slice count of the plan (the matrix-core slices; the VALU slices for the id / cf rows'
            decoder halves);  db likewise with sum |gpre| and the bias slices
Every element of every output is compared.

Incoming gradients are zero-mean (randn): a legal one-slice sequential f32 sum of 5,120 signed
products stays at 1.4e-7 of the sum of |terms|, the same sum over all-positive terms reaches
2.7e-6 (1.7e-5 at 69 k terms) and would miss the dW bar with a correct kernel.

No case lies past 2^31 bytes (tests/test_gpu_big_offsets.py is not extended): the 64-bit
per-image bases (ptr + (long long)b * stride) are held by review.
"""
import functools
import math
import zlib

import torch
import torch.nn.functional as F

from _gconv_bwd_cases import C_GATES, C_MFMA, GUARD, SENT, U, guarded_out, guards_intact, ratio  # noqa: F401

# (B, C, H, W, nout, id, cf) and what the case is for; flags: "unaligned" (the sources are views
# one element into their buffers), "no_g_conf" (the incoming confidence gradient is NULL)
CASES = [
    dict(id="base-2x64x40x64-24", B=2, C=64, H=40, W=64, nout=24, hid=True, hcf=True),
    dict(id="partial-2x64x37x50-24", B=2, C=64, H=37, W=50, nout=24, hid=True, hcf=True),         # partial tiles, W % 4 != 0
    dict(id="short-band-1x64x9x8-8-nocf", B=1, C=64, H=9, W=8, nout=8, hid=True, hcf=False),      # a band shorter than a k-step
    dict(id="two-m-tiles-2x32x24x96-48-noid", B=2, C=32, H=24, W=96, nout=48, hid=False, hcf=True),  # two M tiles, two bands
    dict(id="three-m-tiles-1x64x20x36-72", B=1, C=64, H=20, W=36, nout=72, hid=True, hcf=True),
    dict(id="five-m-tiles-1x16x13x40-144", B=1, C=16, H=13, W=40, nout=144, hid=True, hcf=True),  # 2C = 32
    dict(id="seams-3x16x5x70-24", B=3, C=16, H=5, W=70, nout=24, hid=True, hcf=True),             # image seams in a K slice, uneven bands
    dict(id="one-row-1x16x1x3-24", B=1, C=16, H=1, W=3, nout=24, hid=True, hcf=True),             # nearly every tap outside
    dict(id="unaligned-2x16x40x64-24", B=2, C=16, H=40, W=64, nout=24, hid=True, hcf=True, unaligned=True),
    dict(id="no-g-conf-2x16x40x64-24", B=2, C=16, H=40, W=64, nout=24, hid=True, hcf=True, no_g_conf=True),
]
BY_ID = {c["id"]: c for c in CASES}
IDS = [c["id"] for c in CASES]
assert len(BY_ID) == len(CASES)

# ---------------------------------------------------------------------------- plan mirror
MT, NT, BW, TARGET, MAX_VEC, MAX_BIAS, VEC_PIXELS = 32, 64, 64, 512, 64, 64, 16384


def hb_plan(B, C, H, W, nout):
    """hb_plan (csrc/nlspn_heads_bwd_plan.h): tiles, bands, units, slices, workspace floats."""
    R = nout + 2
    mtiles, ntiles = -(-R // MT), -(-2 * C // NT)
    nbands = -(-W // BW)
    bw = -(-W // nbands)
    units = B * H * nbands
    tiles = mtiles * ntiles
    nsl = max(1, min(units, -(-TARGET // tiles)))
    ups = -(-units // nsl)
    nsl = -(-units // ups)
    per = max(1, -(-B * H * W // VEC_PIXELS))
    nvs, nsb = min(MAX_VEC, per), min(MAX_BIAS, per)
    slab = tiles * MT * NT * 9
    floats = slab * nsl + nvs * 2 * C * 9 + nsb * R
    return dict(R=R, mtiles=mtiles, ntiles=ntiles, nbands=nbands, bw=bw, units=units, ups=ups, nsl=nsl, nvs=nvs, nsb=nsb,
                slab=slab, floats=floats)


def plan_of(c):
    return hb_plan(c["B"], c["C"], c["H"], c["W"], c["nout"])


# ---------------------------------------------------------------------------- operands
RELU_PLANTS = (0.0, -0.0, 2.0 ** -126, 1.5, 0.0, -0.0)
CONF_PLANTS = (2.0 ** -21, 1.0 - 2.0 ** -21, 2.0 ** -24, 1.0 - 2.0 ** -24, 0.5)


def _plant(t, values):
    f = t.view(-1)
    n = min(len(values), f.numel())
    f[:n] = torch.tensor(values[:n], dtype=t.dtype)
    return t


@functools.lru_cache(maxsize=None)
def operands(cid):
    """The f32 operands of a case (CPU): sources, the modules' weights, incoming gradients (None
    where the case passes NULL), the saved outputs."""
    c = BY_ID[cid]
    gen = torch.Generator().manual_seed(zlib.crc32(cid.encode()) & 0x7fffffff)
    B, C, H, W, nout = c["B"], c["C"], c["H"], c["W"], c["nout"]
    r = lambda *s: torch.randn(s, generator=gen)  # noqa: E731
    o = dict(fe1=r(B, C, H, W), fd_oa=r(B, C, H, W), fd_id=r(B, C, H, W) if c["hid"] else None,
             fd_cf=r(B, C, H, W) if c["hcf"] else None)
    k = 1.0 / math.sqrt(4.0 * 2 * C)
    o.update(w_oa=r(nout, 2 * C, 3, 3) * k, w_id=r(1, 2 * C, 3, 3) * k if c["hid"] else None,
             w_cf=r(1, 2 * C, 3, 3) * k if c["hcf"] else None)
    o.update(g_oa=r(B, nout, H, W), g_pi=r(B, 1, H, W) if c["hid"] else None,
             g_cf=r(B, 1, H, W) if c["hcf"] and not c.get("no_g_conf") else None)
    # saved outputs: exact zeros, positives and -0.0; conf in (0, 1), within 2^-20 of both ends
    o["pred_init"] = _plant(torch.relu(r(B, 1, H, W)), RELU_PLANTS) if c["hid"] else None
    o["conf"] = _plant(torch.sigmoid(2.0 * r(B, 1, H, W)).clamp(2.0 ** -24, 1.0 - 2.0 ** -24), CONF_PLANTS) if c["hcf"] else None
    return o


# ---------------------------------------------------------------------------- references (float64)
def gpre_reference(g_oa, g_pi, g_cf, pred_init, conf, B, H, W, nout):
    """gpre (B, R, H, W) in float64: rows < nout g_off_aff, row nout g_pred_init where pred_init > 0
    else 0 (a select), row nout + 1 g_conf conf (1 - conf); a missing gradient gives zero rows."""
    gp = torch.zeros((B, nout + 2, H, W), dtype=torch.float64)
    if g_oa is not None:
        gp[:, :nout] = g_oa.double()
    if g_pi is not None:
        gp[:, nout] = torch.where(pred_init[:, 0] > 0, g_pi[:, 0].double(), torch.zeros((), dtype=torch.float64))
    if g_cf is not None:
        cf = conf[:, 0].double()
        gp[:, nout + 1] = g_cf[:, 0].double() * cf * (1 - cf)
    return gp


def _adjoint(g, w):
    """sum over rows r and taps of w[r, c] flipped (*) g[r]: d[b, c, y, x] = sum w[r, c, ky, kx]
    g[b, r, y + 1 - ky, x + 1 - kx], zero outside the image.  g (B, R', H, W), w (R', Cw, 3, 3)."""
    B, _, H, W = g.shape
    gp = F.pad(g, (1, 1, 1, 1))
    d = torch.zeros((B, w.shape[1], H, W), dtype=torch.float64)
    for ky in range(3):
        for kx in range(3):
            d += torch.einsum("brhw,rc->bchw", gp[:, :, 2 - ky:2 - ky + H, 2 - kx:2 - kx + W], w[:, :, ky, kx])
    return d


def dgrad_reference(gpre, w_oa, w_id, w_cf, C):
    """name -> (ref, X, c) of the four data gradients from gpre (float64 (B, R, H, W)); a head
    without weights is left out (and its rows do not enter d_fe1)."""
    nout = w_oa.shape[0]
    R = nout + 2
    wst = torch.zeros((R, 2 * C, 3, 3), dtype=torch.float64)  # rows against [decoder half | fe1]
    wst[:nout] = w_oa.double()
    for k, w in enumerate((w_id, w_cf)):
        if w is not None:
            wst[nout + k] = w[0].double()
    gabs, wabs = gpre.abs(), wst.abs()
    cc = lambda n: min(C_MFMA, (n + 4) * U)  # noqa: E731
    out = {"d_fe1": (_adjoint(gpre, wst[:, C:]), _adjoint(gabs, wabs[:, C:]), cc(9 * R)),
           "d_fd_oa": (_adjoint(gpre[:, :nout], wst[:nout, :C]), _adjoint(gabs[:, :nout], wabs[:nout, :C]), cc(9 * nout))}
    for k, (name, w) in enumerate((("d_fd_id", w_id), ("d_fd_cf", w_cf))):
        if w is not None:
            r = nout + k
            out[name] = (_adjoint(gpre[:, r:r + 1], wst[r:r + 1, :C]), _adjoint(gabs[:, r:r + 1], wabs[r:r + 1, :C]), cc(9))
    return out


def _corr(s, l):
    """dW[r, c, ky, kx] = sum over b, y, x of s[b, r, y, x] l[b, c, y - 1 + ky, x - 1 + kx], zero outside."""
    B, _, H, W = s.shape
    lp = F.pad(l, (1, 1, 1, 1))
    dw = torch.zeros((s.shape[1], l.shape[1], 3, 3), dtype=torch.float64)
    for ky in range(3):
        for kx in range(3):
            dw[:, :, ky, kx] = torch.einsum("brhw,bchw->rc", s, lp[:, :, ky:ky + H, kx:kx + W])
    return dw


def wgrad_reference(gpre, fe1, fd_oa, fd_id, fd_cf, plan):
    """name -> (ref, X, c) of dw_oa / db_oa and, per present head, dw_id / db_id, dw_cf / db_cf, in
    the modules' layouts ((rows, 2C, 3, 3), the decoder half first), from gpre (float64)."""
    B, R, H, W = gpre.shape
    nout, C = R - 2, fe1.shape[1]
    n = B * H * W
    cm, cv, cb = (min(C_MFMA, (n + plan[k] + 2) * U) for k in ("nsl", "nvs", "nsb"))
    gabs = gpre.abs()
    out = {}
    for name, rows, dec in (("oa", slice(0, nout), fd_oa), ("id", slice(nout, nout + 1), fd_id),
                            ("cf", slice(nout + 1, nout + 2), fd_cf)):
        if dec is None:
            continue
        l = torch.cat((dec, fe1), 1).double()
        cw = torch.full((rows.stop - rows.start, 2 * C, 3, 3), cm, dtype=torch.float64)
        if name != "oa":
            cw[:, :C] = cv  # the VALU sums' slices
        out["dw_" + name] = (_corr(gpre[:, rows], l), _corr(gabs[:, rows], l.abs()), cw)
        out["db_" + name] = (gpre[:, rows].sum((0, 2, 3)), gabs[:, rows].sum((0, 2, 3)), cb)
    return out


def autograd_reference(o, nout):
    """torch double autograd of the reference's op sequence (torch.cat, F.conv2d, ReLU, sigmoid;
    nlspnmodel.py:296-315) on a case's sources and weights (zero biases), under its incoming
    gradients: the saved outputs of THAT forward and every gradient, for the CPU comparison."""
    d = {k: (None if v is None else v.double().requires_grad_(k[0] in "fw")) for k, v in o.items()}
    outs, gouts = [], []
    off = F.conv2d(torch.cat((d["fd_oa"], d["fe1"]), 1), d["w_oa"], padding=1)
    outs.append(off)
    gouts.append(d["g_oa"])
    pred = conf = None
    if d["fd_id"] is not None:
        pred = torch.relu(F.conv2d(torch.cat((d["fd_id"], d["fe1"]), 1), d["w_id"], padding=1))
        outs.append(pred)
        gouts.append(d["g_pi"])
    if d["fd_cf"] is not None:
        conf = torch.sigmoid(F.conv2d(torch.cat((d["fd_cf"], d["fe1"]), 1), d["w_cf"], padding=1))
        if d["g_cf"] is not None:
            outs.append(conf)
            gouts.append(d["g_cf"])
    names = [k for k in ("fe1", "fd_oa", "fd_id", "fd_cf", "w_oa", "w_id", "w_cf") if d[k] is not None]
    grads = torch.autograd.grad(outs, [d[k] for k in names], gouts, allow_unused=True)
    return dict(pred_init=None if pred is None else pred.detach(), conf=None if conf is None else conf.detach(),
                grads=dict(zip(names, grads)))


# ---------------------------------------------------------------------------- the comparison
def check(name, got, ref, X, c, record=None):
    """Every element: finite and |got - ref| <= c X.  Returns the worst err / X."""
    got = got.detach().double().cpu()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    worst = ratio(got, ref, X)
    if record:
        record(f"heads_bwd_elem/{name}", worst)
    print(f"heads_bwd_elem/{name}: worst err / X = {worst:.3g} (c = {float(torch.as_tensor(c).max()):.3g})")
    ok = torch.isfinite(got) & ((got - ref).abs() <= c * X)
    if not bool(ok.all()):
        idx = (~ok).nonzero()
        raise AssertionError(f"{name}: {idx.shape[0]} of {ok.numel()} elements outside c = {float(torch.as_tensor(c).max()):g} "
                             f"(worst ratio {worst:.3g}, {int((~torch.isfinite(got)).sum())} not finite), first at {idx[:6].tolist()}")
    return worst


def guarded(t, dev, shift=0):
    """t on the device as a view into a NaN buffer, GUARD (+ shift) NaNs before and GUARD after it
    (shift = 1: the view starts one element off its 16-byte alignment)."""
    if t is None:
        return None
    n = t.numel()
    buf = torch.full((n + 2 * GUARD + shift,), float("nan"), device=dev, dtype=torch.float32)
    v = buf[GUARD + shift:GUARD + shift + n].view(t.shape)
    v.copy_(t)
    return v
