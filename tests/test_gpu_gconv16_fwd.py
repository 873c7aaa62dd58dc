"""GPU: the forward of the f16-operand GRU-mode convolutions (csrc/nlspn_gconv16.h) per element
against float64, every preset of NLSPN_GC16_CONFIGS and the VALU kernel, at the grids where
the tiling can go wrong.

Each case calls nlspn_gconv16 through _lib.call on weights packed by pack_conv16 / pack_convt16
and c8 inputs (to_c8).  Inputs and weights are drawn as tests/test_gpu_gconv_fwd.py draws them
and rounded to f16 IN THE TEST, so the reference — torch's float64 convolution of those rounded
values on the CPU — sees the operands the matrix cores see: products of two halves are exact
in f32, and what is measured is the accumulation alone.  Per element
    f32 output:   |got - ref| <= c * bound [+ e_act]
    f16 output:   ... + 2^-11 (|ref| + c * bound) + 2^-24       (the store's own rounding)
bound = the same convolution on absolute values (sum |w||x| + |b|).  ReLU and tanh are
1-Lipschitz and sigmoid' <= 1/4, so the pre-activation bound carries over; e_act is the f32
family's measured 4e-7 (cap 16 * 2^-24): the device functions are the same.

Bars.  c per kind is 4x the worst ratio measured on an MI355X over every case of the kind
(recorded per run as gconv16_fwd/*), rounded up to one digit, and must be <= 2^-13 = 1.2e-4: one
stray f16 rounding of a partial sum or operand costs 2^-11, a bf16 rounding 2^-9, a layout
error O(1); an honest f32 accumulation of exact products is orders of magnitude lower.
    kind    measured (worst case)                                  bar
    s2      9.3e-8  16 -> 128, 14x23, odd input                            4e-7
    t2      1.2e-7  id 51, 56 -> 64 from two sources, 7x21                 5e-7
    gru1    1.7e-7  qx, hc 256, 17x39 (z 5.6e-9 beside e_act; r*h 0:       7e-7
            its f16 store's rounding covers the rest)
    gru2    2.3e-8  h', hc 256, 17x39 (beside z e_act and the blend's      9e-8
            four roundings; 0 at hc 128)
    small   the f32 family's VALU arithmetic unchanged: its bar 7e-7 under its cap (9 cin + 3) 2^-24
            (the output is f16 only, whose store rounding hides a ratio this small: measured 0; the
            test also requires the output to be the f32 kernel's, rounded once, bit for bit)
So the 16x16x32 f16 MFMA sums exact products in f32 about as tightly as the f32 family's own
kernels do (theirs: 2e-7 .. 4e-7 at the same term counts): no sign of a narrower internal sum.
The two-launch cell end to end, relative L2 against the float64 cell with r*h rounded to f16
where the contract rounds it: 2.6e-6 at worst (hc 256, 17x39: device and reference round a few
r*h elements to different neighbours); bar 2e-5, on condition <= 1e-4 (one f16 rounding
of every element of h' would be 2^-11 / sqrt(3) = 2.8e-4).

Grids are computed from each preset's own geometry (GEO mirrors NLSPN_GC16_CONFIGS for the
case arithmetic only; what is launched is the library's own plan): the smallest grid whose
narrower last band spans an extra window row under the tile the widest band alone would allow,
the smallest grid with an empty last tile, one full band and one pixel more, 9x2, 1x1 and a
single row; stride 2 at both input parities.
"""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from nlspn_eccv20_amd import _lib
from nlspn_eccv20_amd.gru import (ACT_NONE, ACT_RELU, ACT_TANH, GC16_GRU1, GC16_GRU2, GC16_S2, GC16_S2_SMALL, GC16_T2,
                                  GC16_T2_C16, from_c8, pack_conv16, pack_convt16, to_c8)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
H11 = 2.0 ** -11
SENT = -7777.0
GUARD = 4096
CAP = 2.0 ** -13   # the condition on every asserted c

S1, S2, T2 = 0, 1, 2
# id -> (mode, NPX, XR, XP, co tile)
GEO = {GC16_S2: (S2, 64, 12, 40, 64), GC16_GRU1: (S1, 64, 6, 40, 64), GC16_GRU2: (S1, 64, 6, 40, 64),
       GC16_T2: (T2, 64, 6, 40, 64), GC16_T2_C16: (T2, 128, 6, 80, 16)}
C = {"s2": 4e-7, "t2": 5e-7, "gru1": 7e-7, "gru2": 9e-8, "small": 7e-7}
E_TANH = 4e-7
E_SIG = 4e-7
BAR_CELL = 2e-5


def test_bars_meet_their_condition():
    assert all(c <= CAP for c in C.values()) and BAR_CELL <= 1e-4 and max(E_TANH, E_SIG) <= 16 * U


# ------------------------------------------------------------------ grids from the geometry
def _bwmax(mode, xp):
    return xp - 2 if mode == S1 else (xp - 3) // 2 + 1 if mode == S2 else xp - 1


def _rows(mode, n, w):
    dr = (n + w - 2) // w
    return dr + 3 if mode == S1 else 2 * dr + 3 if mode == S2 else dr + 2


def _bands(layer, gw):
    mode, npx, xr, xp, _ = GEO[layer]
    nbands = -(-gw // _bwmax(mode, xp))
    bw = -(-gw // nbands)
    return nbands, bw, gw - (nbands - 1) * bw


def _npx_for(layer, w):
    mode, npx, xr, xp, _ = GEO[layer]
    while npx > 1 and _rows(mode, npx, w) > xr:
        npx -= 1
    return npx


def _span(mode, f0, n, w, gh):
    """Window rows of the run of n pixels from flat pixel f0 in a band of width w."""
    ra, rb = f0 // w, min(gh - 1, (f0 + n - 1) // w)
    return (2 if mode == S2 else 1) * (rb - ra) + (2 if mode == T2 else 3)


@functools.lru_cache(maxsize=None)
def grid_extra_row(layer):
    """The smallest grid (by width, then height) at which a tile sized for the widest band alone
    would span more than XR window rows in the narrower last band; None when no grid up to 400
    columns has one (the transposed presets: six rows hold a full tile in any band that has a
    neighbour)."""
    mode, _, xr, _, _ = GEO[layer]
    for gw in range(2, 401):
        nbands, bw, bwl = _bands(layer, gw)
        if nbands < 2 or bwl == bw:
            continue
        n = _npx_for(layer, bw)
        if _rows(mode, n, bwl) <= xr:
            continue
        for gh in range(1, 65):
            if any(_span(mode, f0, n, bwl, gh) > xr for f0 in range(0, gh * bwl, n)):
                return gh, gw
    return None


@functools.lru_cache(maxsize=None)
def grid_uneven(layer):
    """The smallest width with a narrower last band, at 17 rows (more than one tile per band)."""
    for gw in range(2, 401):
        nbands, bw, bwl = _bands(layer, gw)
        if nbands >= 2 and bwl < bw:
            return 17, gw
    raise AssertionError(layer)


@functools.lru_cache(maxsize=None)
def grid_empty_tile(layer):
    """The smallest grid (by pixels) whose last band has fewer tiles than the widest."""
    best = None
    for gw in range(2, 200):
        nbands, bw, bwl = _bands(layer, gw)
        if nbands < 2 or bwl == bw:
            continue
        n = _npx_for(layer, bwl)
        for gh in range(1, 33):
            if -(-gh * bwl // n) < -(-gh * bw // n):
                if best is None or gh * gw < best[0] * best[1]:
                    best = (gh, gw)
                break
    assert best, layer
    return best


def grids_a(layer):
    return [grid_extra_row(layer) or grid_uneven(layer), grid_empty_tile(layer)]


def grids_b(layer):
    mode, _, _, xp, _ = GEO[layer]
    bm = _bwmax(mode, xp)
    return [(5, bm), (5, bm + 1), (9, 2), (1, 1), (1, 2 * bm + 3)]


def test_computed_grids_have_their_property():
    for layer in GEO:
        mode, _, xr, _, _ = GEO[layer]
        g = grid_extra_row(layer)
        assert (g is None) == (mode == T2), (layer, g)
        if g:
            _, bw, bwl = _bands(layer, g[1])
            assert _npx_for(layer, bwl) < _npx_for(layer, bw)
        gh, gw = grid_empty_tile(layer)
        _, bw, bwl = _bands(layer, gw)
        n = _npx_for(layer, bwl)
        assert -(-gh * bwl // n) < -(-gh * bw // n)


# ------------------------------------------------------------------ helpers
def _h(t):
    return t.half().float()


def _conv64(mode, x, w, b, absval=False):
    x, w, b = x.double(), w.double(), None if b is None else b.double()
    if absval:
        x, w, b = x.abs(), w.abs(), None if b is None else b.abs()
    if mode == T2:
        return F.conv_transpose2d(x, w, b, stride=2, padding=1, output_padding=1)
    return F.conv2d(x, w, b, stride=2 if mode == S2 else 1, padding=1)


def _act64(y, act):
    return torch.relu(y) if act == ACT_RELU else torch.tanh(y) if act == ACT_TANH else y


def _out(shape, dtype=torch.float32):
    n = math.prod(shape)
    buf = torch.full((n + GUARD,), SENT, device=DEV, dtype=dtype)
    return buf, buf[:n].view(*shape)


def _guard_ok(buf):
    return bool((buf[-GUARD:] == SENT).all())


def _check(name, got, ref, bound, c, e_abs=0.0, extra=0.0, half=False, record=None):
    """Every element: |got - ref| <= c * bound + e_abs + extra (+ the f16 store's rounding).
    Returns the worst (err - e_abs - extra - store) / bound: the measured c."""
    got = got.detach().double().cpu()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    err = (got - ref).abs()
    store = H11 * (ref.abs() + c * bound + e_abs + extra) + U if half else 0.0
    ratio = float(((err - e_abs - extra - store).clamp(min=0) / (bound + 1e-300)).nan_to_num(nan=float("inf")).max())
    if record:
        record(f"gconv16_fwd/{name}", ratio)
    ok = err <= c * bound + e_abs + extra + store
    if not bool(ok.all()):
        idx = (~ok).nonzero()
        raise AssertionError(f"{name}: {idx.shape[0]} of {ok.numel()} elements outside c = {c:g} (worst ratio {ratio:.3g}, "
                             f"largest error {float(err.max()):.3g}), first at {idx[:6].tolist()}")
    return ratio


def _c8_out(B, cout, oh, ow):
    buf, y = _out((B, (cout + 7) // 8, oh, ow, 8), torch.float16)
    return buf, y


def _check_c8_pad(y16, cout):
    flat = y16.permute(0, 1, 4, 2, 3).reshape(y16.shape[0], -1, y16.shape[2], y16.shape[3])
    assert not bool(flat[:, cout:].any()), "pad channels of a c8 output must be zero"


# ------------------------------------------------------------------ plain layers (stride 2, transposed)
def _plain(layer, B, cin, cout, Hi, Wi, act, seed, crop=None, split=None, nan_at=(), fmt="both"):
    mode = GEO[layer][0]
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((B, cin, Hi, Wi), generator=g)
    for idx in nan_at:
        x[idx] = float("nan")
    wshape = (cin, cout, 3, 3) if mode == T2 else (cout, cin, 3, 3)
    w = torch.randn(wshape, generator=g) / math.sqrt(4.0 * cin)
    b = torch.randn(cout, generator=g) * 0.3
    x, w = _h(x), _h(w)     # the operands are halves; the bias stays f32
    Ho, Wo = (2 * Hi, 2 * Wi) if mode == T2 else ((Hi - 1) // 2 + 1, (Wi - 1) // 2 + 1)
    ohs, ows = crop or (Ho, Wo)
    pre = _conv64(mode, x, w, b)[:, :, :ohs, :ows]
    bound = _conv64(mode, x, w, b, True)[:, :, :ohs, :ows]
    wpk, bpk = (pack_convt16 if mode == T2 else pack_conv16)(w.to(DEV), b.to(DEV), layer)
    xs = [to_c8(x.to(DEV))] if split is None else [to_c8(x[:, :split].to(DEV)), to_c8(x[:, split:].to(DEV))]
    b16, y16 = _c8_out(B, cout, ohs, ows) if fmt in ("both", "f16") else (None, None)
    b32, y32 = _out((B, cout, ohs, ows)) if fmt in ("both", "f32") else (None, None)
    _lib.call("nlspn_gconv16", xs[0].device, layer, xs[0], split or cin, xs[1] if split else None,
              cin - split if split else 0, wpk, bpk, y16, y32, None, None, None, None, None, None, B, Hi, Wi, cout, ohs, ows,
              act, 1.0, 0, _lib.STREAM)
    torch.cuda.synchronize()
    assert all(_guard_ok(bf) for bf in (b16, b32) if bf is not None), "a store past the last stored element"
    if y16 is not None:
        _check_c8_pad(y16, cout)
        y16 = from_c8(y16, cout)
    return y16, y32, _act64(pre, act), bound


PLAIN_CH = {GC16_S2: (16, 128), GC16_T2: (64, 64), GC16_T2_C16: (64, 16)}
KIND = {GC16_S2: "s2", GC16_T2: "t2", GC16_T2_C16: "t2"}


def _run_plain(layer, gh, gw, record, act=ACT_RELU, B=2, cin=None, cout=None, parity=0, crop=None, split=None, fmt="both",
               tag=""):
    mode = GEO[layer][0]
    ci, co = PLAIN_CH[layer]
    cin, cout = cin or ci, cout or co
    Hi, Wi = (gh, gw) if mode == T2 else (2 * gh - parity, 2 * gw - parity)
    y16, y32, ref, bound = _plain(layer, B, cin, cout, Hi, Wi, act, seed=100 * layer + gh + gw, crop=crop, split=split, fmt=fmt)
    kind = KIND[layer]
    e = E_TANH if act == ACT_TANH else 0.0
    name = f"{kind}/id{layer}/{B}x{cin}>{cout}/{gh}x{gw}p{parity}{tag}"
    if y32 is not None:
        _check(name + "/f32", y32, ref, bound, C[kind], e, record=record)
    if y16 is not None:
        _check(name + "/f16", y16, ref, bound, C[kind], e, half=True)
    if y16 is not None and y32 is not None:  # the f16 copy is the f32 value rounded once, exactly
        assert torch.equal(y16.cpu(), y32.cpu().half()), "y16 is not y32 rounded to nearest-even"


PLAIN = (GC16_S2, GC16_T2, GC16_T2_C16)


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("layer", PLAIN)
def test_uneven_last_band_and_empty_tiles(layer, which, record_metric):
    """a. Stride 2: both input parities."""
    gh, gw = grids_a(layer)[which]
    for parity in ((0, 1) if GEO[layer][0] == S2 else (0,)):
        _run_plain(layer, gh, gw, record_metric, parity=parity)


@pytest.mark.parametrize("which", range(5))
@pytest.mark.parametrize("layer", PLAIN)
def test_band_and_tile_edges(layer, which, record_metric):
    gh, gw = grids_b(layer)[which]
    _run_plain(layer, gh, gw, record_metric, parity=(gh + gw) % 2)


@pytest.mark.parametrize("layer", PLAIN)
def test_channel_edges(layer, record_metric):
    """c. cin 20 (a partial 8-block: pad channels; three of a chunk's four blocks), cin 40 (a
    partial second chunk: blocks past the tensor's last read 0 through the descriptor's range),
    cout not a multiple of the co tile or of 8 (pad channels of the c8 output zero, nothing
    stored beyond), and the two-source input c0 = 32, c1 = 24."""
    wide = GEO[layer][4] == 64
    _run_plain(layer, 7, 21, record_metric, cin=20, parity=1, tag="/cin20")
    _run_plain(layer, 7, 21, record_metric, cin=40, tag="/cin40")
    _run_plain(layer, 7, 21, record_metric, cout=76 if wide else 12, tag="/cout")
    _run_plain(layer, 7, 21, record_metric, cin=56, split=32, parity=1, tag="/split32")


@pytest.mark.parametrize("off", [0, 1, 7])
@pytest.mark.parametrize("layer", [GC16_T2, GC16_T2_C16])
def test_transposed_crops(layer, off, record_metric):
    gh, gw = 6, 41
    _run_plain(layer, gh, gw, record_metric, act=ACT_NONE, crop=(2 * gh - off, 2 * gw - off), tag=f"/crop{off}")


@pytest.mark.parametrize("fmt", ["f16", "f32"])
@pytest.mark.parametrize("layer", PLAIN)
def test_one_output_format_alone(layer, fmt, record_metric):
    gh, gw = grids_a(layer)[0]
    _run_plain(layer, gh, gw, record_metric, fmt=fmt, tag="/" + fmt)


def test_tanh_epilogue(record_metric):
    """encode_aff's last layer: Tanh, both outputs (the initial h and its f16 copy)."""
    gh, gw = grids_a(GC16_S2)[0]
    _run_plain(GC16_S2, gh, gw, record_metric, act=ACT_TANH, cin=64, tag="/tanh")


@pytest.mark.parametrize("layer", PLAIN)
def test_nan_reaches_exactly_the_reference_outputs(layer):
    """h. The zero padding is an out-of-range buffer offset and a band's window overlaps its
    neighbour's: a NaN at two corners and one at the input column two bands share.  The NaN set
    equals the float64 reference's exactly in both outputs; every other element is in bound."""
    mode, (cin, cout) = GEO[layer][0], PLAIN_CH[layer]
    gh, gw = grids_a(layer)[0]
    _, bw, _ = _bands(layer, gw)
    Hi, Wi = (gh, gw) if mode == T2 else (2 * gh, 2 * gw)
    seam = bw if mode == T2 else 2 * bw - 1
    nan_at = [(0, 0, 0, 0), (1, cin - 1, Hi - 1, Wi - 1), (1, 3, Hi // 2, seam)]
    y16, y32, ref, bound = _plain(layer, 2, cin, cout, Hi, Wi, ACT_RELU, seed=8, nan_at=nan_at)
    nan_ref = torch.isnan(ref)
    assert 3 <= int(nan_ref[:, 0].sum()) <= 27
    for y, half in ((y32, False), (y16, True)):
        got = y.double().cpu()
        assert torch.equal(torch.isnan(got), nan_ref), (int(torch.isnan(got).sum()), int(nan_ref.sum()))
        fin = ~nan_ref
        _check(f"{KIND[layer]}/id{layer}/nan", torch.where(fin, got, 0.0), torch.where(fin, ref, 0.0),
               torch.where(fin, bound, 1.0), C[KIND[layer]], half=half)


# ------------------------------------------------------------------ the VALU kernel
@pytest.mark.parametrize("cin,Hi,Wi,in_div,crop", [(1, 27, 45, 10.0, None), (1, 28, 46, 10.0, (13, 22)),
                                                   (9, 27, 46, 1.0, None), (9, 28, 45, 10.0, (14, 20))])
def test_small_valu_kernel(cin, Hi, Wi, in_div, crop, record_metric):
    """NLSPN_GC16_S2_SMALL (cin 1 / 9 -> 16): f32 NCHW in (not rounded: the kernel's operands and
    sums are f32), odd and even sizes, in_div, a crop; the c8 store is the only f16 rounding."""
    B, cout = 2, 16
    g = torch.Generator().manual_seed(60 + cin + Hi)
    x = torch.rand((B, cin, Hi, Wi), generator=g) * in_div
    w = torch.randn((cout, cin, 3, 3), generator=g) / math.sqrt(4.0 * cin)
    b = torch.randn(cout, generator=g) * 0.3
    ohs, ows = crop or ((Hi - 1) // 2 + 1, (Wi - 1) // 2 + 1)
    ref = torch.relu(_conv64(S2, x.double() / in_div, w, b))[:, :, :ohs, :ows]
    bound = _conv64(S2, x.double() / in_div, w, b, True)[:, :, :ohs, :ows]
    buf, y = _c8_out(B, cout, ohs, ows)
    xd, wd, bd = x.to(DEV), w.to(DEV).contiguous(), b.to(DEV)
    _lib.call("nlspn_gconv16", xd.device, GC16_S2_SMALL, xd, cin, None, 0, wd, bd, y, None, None, None, None, None, None, None,
              B, Hi, Wi, cout, ohs, ows, ACT_RELU, in_div, 0, _lib.STREAM)
    torch.cuda.synchronize()
    assert _guard_ok(buf)
    assert C["small"] <= (9 * cin + 2 + (in_div != 1.0)) * U
    _check(f"small/cin{cin}/{Hi}x{Wi}", from_c8(y, cout), ref, bound, C["small"], half=True, record=record_metric)
    # the same arithmetic as the f32 family's VALU kernel: its output rounded once, bit for bit
    y32 = torch.empty((B, cout, ohs, ows), device=DEV)
    _lib.call("nlspn_gconv", xd.device, 6, xd, cin, None, 0, wd, bd, y32, None, None, None, None, None, B, Hi, Wi, cout, ohs,
              ows, ACT_RELU, in_div, 0, _lib.STREAM)
    assert torch.equal(from_c8(y, cout), y32.half())


# ------------------------------------------------------------------ ConvGRU
@functools.lru_cache(maxsize=None)
def _gru_ref(hc, B, H, W):
    """The ConvGRU cell (nlspnmodel.py:398-403) in float64 under the contract: h carried in f32,
    the convolutions read h, x, r*h and the weights as halves; GRU2 alone on the reference's
    rounded z (f32), r*h (f16) and qx (f32)."""
    g = torch.Generator().manual_seed(3 + hc + 7 * B + H * W)
    s = 1.0 / math.sqrt(6.0 * hc)
    wz, wr, wq = (_h(torch.randn((hc, 2 * hc, 3, 3), generator=g) * s) for _ in range(3))
    bias_z, bias_r, bias_q = (torch.randn(hc, generator=g) * 0.3 for _ in range(3))
    h = torch.tanh(torch.randn((B, hc, H, W), generator=g))          # f32 state
    x = _h(torch.relu(torch.randn((B, hc, H, W), generator=g)))       # a c8 activation
    hx, h64 = torch.cat([_h(h), x], 1), h.double()
    R = dict(hc=hc, wz=wz, wr=wr, wq=wq, bias_z=bias_z, bias_r=bias_r, bias_q=bias_q, h=h, x=x)
    R["z"] = torch.sigmoid(_conv64(S1, hx, wz, bias_z))
    R["r"] = torch.sigmoid(_conv64(S1, hx, wr, bias_r))
    R["rh"] = R["r"] * h64                                            # formed with the f32 h
    R["qx"] = _conv64(S1, x, wq[:, hc:], bias_q)
    R["bd_z"], R["bd_r"] = _conv64(S1, hx, wz, bias_z, True), _conv64(S1, hx, wr, bias_r, True)
    R["bd_qx"] = _conv64(S1, x, wq[:, hc:], bias_q, True)
    z32, rh16, qx32 = R["z"].float(), R["rh"].half(), R["qx"].float()
    R["z32"], R["rh16"], R["qx32"] = z32, rh16, qx32
    R["q2"] = torch.tanh(_conv64(S1, rh16.float(), wq[:, :hc], None) + qx32.double())
    R["bd_q2"] = _conv64(S1, rh16.float(), wq[:, :hc], None, True) + qx32.double().abs()
    R["hn2"] = (1 - z32.double()) * h64 + z32.double() * R["q2"]
    # the cell end to end: r*h rounded to f16 where the contract rounds it, nothing else
    q = torch.tanh(_conv64(S1, R["rh"].half().float(), wq[:, :hc], None) + R["qx"])
    R["hn"] = (1 - R["z"]) * h64 + R["z"] * q
    return R


def _gru1(R, B, H, W):
    hc = R["hc"]
    w1 = torch.cat([R["wz"], R["wr"], R["wq"]], 0).to(DEV)
    b1 = torch.cat([R["bias_z"], R["bias_r"], R["bias_q"]], 0).to(DEV)
    wpk, bpk = pack_conv16(w1, b1, GC16_GRU1)
    h = R["h"].to(DEV)
    h16, x16 = to_c8(h), to_c8(R["x"].to(DEV))
    bz, z = _out((B, hc, H, W))
    bq, qx = _out((B, hc, H, W))
    br, rh = _c8_out(B, hc, H, W)
    _lib.call("nlspn_gconv16", h.device, GC16_GRU1, h16, hc, x16, hc, wpk, bpk, None, None, h, z, rh, qx, None, None,
              B, H, W, 3 * hc, 0, 0, ACT_NONE, 1.0, hc, _lib.STREAM)
    torch.cuda.synchronize()
    assert _guard_ok(bz) and _guard_ok(bq) and _guard_ok(br)
    return z, rh, qx


def _gru2(R, z, rh16, qx, B, H, W):
    hc = R["hc"]
    wpk, bpk = pack_conv16(R["wq"][:, :hc].contiguous().to(DEV), R["bias_q"].to(DEV), GC16_GRU2)
    h = R["h"].to(DEV)
    b32, hn = _out((B, hc, H, W))
    b16, hn16 = _c8_out(B, hc, H, W)
    _lib.call("nlspn_gconv16", h.device, GC16_GRU2, rh16, hc, None, 0, wpk, bpk, None, None, h, z, None, qx, hn, hn16,
              B, H, W, hc, 0, 0, ACT_NONE, 1.0, hc, _lib.STREAM)
    torch.cuda.synchronize()
    assert _guard_ok(b32) and _guard_ok(b16)
    return hn, hn16


def gru_grids():
    """(B, H, W): the uneven last band with an extra row, the empty last tile, and one-band grids
    whose pixel-tile count is odd and even (a qx workgroup takes two pixel tiles, the last one
    alone when odd); then 9x2, 1x1 and a single row."""
    ex, em = grids_a(GC16_GRU1)
    bm = _bwmax(S1, GEO[GC16_GRU1][3])
    return [(2, *ex), (2, *em), (1, 17, bm), (1, 3, bm), (2, 9, 2), (2, 1, 1), (2, 1, 2 * bm + 3)]


def test_gru1_cases_cover_odd_and_even_tile_counts():
    par = set()
    for B, H, W in gru_grids():
        nbands, bw, bwl = _bands(GC16_GRU1, W)
        par.add((B * nbands * -(-H * bw // _npx_for(GC16_GRU1, bwl))) % 2)
    assert par == {0, 1}


def _gru_case(i):
    B, H, W = gru_grids()[i]
    return B, H, W


@pytest.mark.parametrize("case,hc", [(i, 128) for i in range(7)] + [(0, 256)])
def test_gru1_per_element(case, hc, record_metric):
    """GRU1's z, r*h (c8) and qx per element.  The qx tiles run K over x only."""
    B, H, W = _gru_case(case)
    R = _gru_ref(hc, B, H, W)
    z, rh, qx = _gru1(R, B, H, W)
    c = C["gru1"]
    name = f"gru1/hc{hc}/{B}x{H}x{W}"
    _check(name + "/qx", qx, R["qx"], R["bd_qx"], c, record=record_metric)
    _check(name + "/z", z, R["z"], R["bd_z"], c, E_SIG, record=record_metric)
    # r*h: |h| times r's bound, the f32 product's own rounding, then the f16 store
    habs = R["h"].double().abs()
    _check(name + "/rh", from_c8(rh, hc), R["rh"], habs * R["bd_r"], c, habs * E_SIG, 2 * U * R["rh"].abs(), half=True,
           record=record_metric)


@pytest.mark.parametrize("case,hc", [(i, 128) for i in range(7)] + [(0, 256)])
def test_gru2_per_element(case, hc, record_metric):
    """GRU2 fed the reference's rounded z, r*h and qx: h' in f32 and its f16 copy."""
    B, H, W = _gru_case(case)
    R = _gru_ref(hc, B, H, W)
    hn, hn16 = _gru2(R, R["z32"].to(DEV), to_c8(R["rh16"].to(DEV)), R["qx32"].to(DEV), B, H, W)
    c = C["gru2"]
    name = f"gru2/hc{hc}/{B}x{H}x{W}"
    # h' = (1 - z) h + z q: z times q's bound, and the blend's four roundings of values <= |h| + 1
    z = R["z32"].double()
    extra = 4 * U * (R["h"].double().abs() + 1)
    _check(name + "/hn", hn, R["hn2"], z * R["bd_q2"], c, z * E_TANH, extra, record=record_metric)
    _check(name + "/hn16", from_c8(hn16, hc), R["hn2"], z * R["bd_q2"], c, z * E_TANH, extra, half=True)
    assert torch.equal(from_c8(hn16, hc), hn.half()), "the f16 copy of h' is not h' rounded to nearest-even"


@pytest.mark.parametrize("case,hc", [(0, 128), (1, 128), (0, 256)])
def test_gru_cell_end_to_end(case, hc, record_metric):
    """The two-launch cell, GRU2 reading GRU1's own outputs, against float64: relative L2."""
    B, H, W = _gru_case(case)
    R = _gru_ref(hc, B, H, W)
    z, rh, qx = _gru1(R, B, H, W)
    hn, _ = _gru2(R, z, rh, qx, B, H, W)
    e = float((hn.double().cpu() - R["hn"]).norm() / R["hn"].norm())
    record_metric(f"gconv16_fwd/cell/hc{hc}/{B}x{H}x{W}", e)
    assert e <= BAR_CELL, e


def test_nan_in_the_gru():
    """A NaN in h (both copies, as a step writes them) and one in x at the band seam."""
    B, H, W = _gru_case(0)
    hc = 128
    R = dict(_gru_ref(hc, B, H, W))
    _, bw, _ = _bands(GC16_GRU1, W)
    h, x = R["h"].clone(), R["x"].clone()
    h[0, 5, 0, 0] = float("nan")
    x[1, 7, H // 2, bw] = float("nan")
    R["h"], R["x"] = h, x
    hx = torch.cat([_h(h), x], 1)
    z64 = torch.sigmoid(_conv64(S1, hx, R["wz"], R["bias_z"]))
    qx64 = _conv64(S1, x, R["wq"][:, hc:], R["bias_q"])
    z, rh, qx = _gru1(R, B, H, W)
    assert torch.equal(torch.isnan(z.cpu()), torch.isnan(z64)) and int(torch.isnan(z64)[:, 0].sum()) == 4 + 9
    assert torch.equal(torch.isnan(qx.cpu()), torch.isnan(qx64)) and int(torch.isnan(qx64)[:, 0].sum()) == 9
