"""GPU: the forward of the split-bf16 GRU-mode convolutions (csrc/nlspn_gconv_x3.h) per element
against float64, every preset of NLSPN_GCX3_CONFIGS and the VALU kernel, at the grids where the
tiling can go wrong.

Each case calls nlspn_gconv_x3 through _lib.call on weights packed by pack_conv_x3 /
pack_convt_x3 and c8x2 inputs (to_c8x2) of f32 operands.  Every operand tensor sits between NaN
guards (a read outside it poisons the output) and every output between sentinels.  Two float64
references on the CPU, with bound = the same convolution on absolute values (sum |w||x| + |b|):
    emu: the three split products of the very operands passed in, conv(w_hi, x_hi) +
         conv(w_hi, x_lo) + conv(w_lo, x_hi):     |got - emu| <= c_acc * bound [+ e_act]
    ref: the convolution of the unsplit f32 operands:
                                                   |got - ref| <= (2^-15 + c_acc) * bound [+ e_act]
c_acc = min(2e-6, (3 n + 2) 2^-24) for an n-term sum and e_act = 4e-7 where tanhf / expf run: the
f32 family's own conditions (tests/test_gpu_gconv_fwd.py).  2^-15 is the contract's bound on a
term (2^-17 per operand's residual, 2^-16 for the dropped lo lo).  A missing hi lo product costs
2^-9, a swapped hi / lo cell or a layout error O(1).  A split output (from_c8x2) obeys both bounds
plus 2^-17 |ref|, and where a launch writes f32 and split the split is split_bf16 of the f32
output bit for bit; the VALU preset's output is the f32 NLSPN_GC_S2_SMALL output split, bit for bit.

Measured on an MI355X (worst ratio to bound over every case of the kind, recorded per run as
gconv_x3_fwd/<kind>/<case>):
    kind     against emu (bar c_acc = 2e-6)             against ref (bar 2^-15 + c_acc = 3.25e-5)
    s2       1.8e-7  40 -> 128 from 16 + 24, 7x21         4.7e-6  16 -> 128, 1x41, odd input
    t2       1.8e-7  64 -> 24, 7x21                       6.1e-6  40 -> 64 from 16 + 24, 7x21
    t2_c16   1.6e-7  64 -> 16, 17x81                      4.5e-6  40 -> 16 from 16 + 24, 7x21
    gru1     2.6e-7  qx, hc 128, 17x39 (z 1.3e-8 beside   2.2e-6  qx, hc 128, 1x79 (z 2.1e-7,
             e_act, r*h 0 beside the store's 2^-17)                r*h 1.1e-7)
    gru2     6.6e-8  h', hc 256, 17x39                    9.3e-7  h', hc 128, 1x79
    small    4.2e-8  cin 9, 28x45 (unsplit f32 operands: both references are the same)
Against the emulation the kernels sit on the f32 family's own accumulation floor (2e-7 .. 4e-7);
against the unsplit operands they use a fifth of the contract's 2^-15 at most.

Grids are computed from each preset's own geometry (GEO mirrors NLSPN_GCX3_CONFIGS for the case
arithmetic only; what is launched is the library's own plan): the smallest grid whose narrower
last band spans an extra window row under the tile the widest band alone would allow, the
smallest grid with an empty last tile, one full band and one pixel more, 9x2, 1x1 and a single
row; stride 2 at both input parities.
"""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from nlspn_eccv20_amd import _lib
from nlspn_eccv20_amd.gru import (ACT_NONE, ACT_RELU, ACT_TANH, GC_S2_SMALL, GCX3_GRU1, GCX3_GRU2, GCX3_S2, GCX3_S2_SMALL,
                                  GCX3_T2, GCX3_T2_C16, from_c8x2, pack_conv_x3, pack_convt_x3, split_bf16, to_c8x2)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
SPLIT = 2.0 ** -17     # |a - hi - lo| <= 2^-17 |a|
TERM = 2.0 ** -15      # the contract's bound on a term
SENT = -7777.0
GUARD = 4096
E_ACT = 4e-7

S1, S2, T2 = 0, 1, 2
# id -> (mode, NPX, XR, XP, co tile)
GEO = {GCX3_S2: (S2, 64, 12, 40, 64), GCX3_GRU1: (S1, 64, 6, 40, 64), GCX3_GRU2: (S1, 64, 6, 40, 64),
       GCX3_T2: (T2, 64, 6, 40, 64), GCX3_T2_C16: (T2, 128, 6, 80, 16)}


def c_acc(n):
    return min(2e-6, (3 * n + 2) * U)


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
    ra, rb = f0 // w, min(gh - 1, (f0 + n - 1) // w)
    return (2 if mode == S2 else 1) * (rb - ra) + (2 if mode == T2 else 3)


@functools.lru_cache(maxsize=None)
def grid_extra_row(layer):
    """The smallest grid at which a tile sized for the widest band alone would span more than XR
    window rows in the narrower last band; None when no grid up to 400 columns has one."""
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


def grids(layer):
    mode, _, _, xp, _ = GEO[layer]
    bm = _bwmax(mode, xp)
    return [grid_extra_row(layer) or grid_uneven(layer), grid_empty_tile(layer), (5, bm + 1), (9, 2), (1, 1), (1, 2 * bm + 3)]


def test_computed_grids_have_their_property():
    for layer in GEO:
        mode = GEO[layer][0]
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
def _parts64(t):
    hi, lo = split_bf16(t)
    return hi.double(), lo.double()


def _conv64(mode, x, w, b=None):
    x, w, b = x.double(), w.double(), None if b is None else b.double()
    if mode == T2:
        return F.conv_transpose2d(x, w, b, stride=2, padding=1, output_padding=1)
    return F.conv2d(x, w, b, stride=2 if mode == S2 else 1, padding=1)


def _three(mode, x, w, b=None):
    """(emu, ref, bound) of one convolution of f32 operands: the three split products, the
    unsplit convolution, and the convolution of absolute values; float64."""
    xh, xl = _parts64(x)
    wh, wl = _parts64(w)
    emu = _conv64(mode, xh, wh, b) + _conv64(mode, xl, wh) + _conv64(mode, xh, wl)
    return emu, _conv64(mode, x, w, b), _conv64(mode, x.abs(), w.abs(), None if b is None else b.abs())


def _act64(y, act):
    return torch.relu(y) if act == ACT_RELU else torch.tanh(y) if act == ACT_TANH else y


def _guarded(t):
    """t on the device between NaN guards: a read outside it poisons the output."""
    t = t.contiguous()
    buf = torch.full((t.numel() + 2 * GUARD,), float("nan"), device=DEV, dtype=t.dtype)
    v = buf[GUARD:GUARD + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def _out(shape, dtype=torch.float32):
    n = math.prod(shape)
    buf = torch.full((n + 2 * GUARD,), SENT, device=DEV, dtype=dtype)
    return buf, buf[GUARD:GUARD + n].view(*shape)


def _guard_ok(buf):
    return bool((buf[:GUARD] == SENT).all()) and bool((buf[-GUARD:] == SENT).all())


def _split_out(B, cout, oh, ow):
    return _out((B, (cout + 7) // 8, 2, oh, ow, 8), torch.bfloat16)


def _check(name, got, emu, ref, bound, n, e_abs=0.0, extra=0.0, split=False, record=None):
    """Every element against both references; returns the worst ratios (emu, ref) to bound."""
    got = got.detach().double().cpu()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), f"{name}: a non-finite output (a read of a NaN guard?)"
    c = c_acc(n)
    store = SPLIT * ref.abs() if split else 0.0
    out = []
    for tag, want, cc in (("emu", emu, c), ("ref", ref, TERM + c)):
        err = (got - want).abs()
        ratio = float(((err - e_abs - extra - store).clamp(min=0) / (bound + 1e-300)).max())
        out.append(ratio)
        if record:
            record(f"gconv_x3_fwd/{name}/{tag}", ratio)
    for tag, want, cc in (("emu", emu, c), ("ref", ref, TERM + c)):
        err = (got - want).abs()
        ok = err <= cc * bound + e_abs + extra + store
        if not bool(ok.all()):
            idx = (~ok).nonzero()
            raise AssertionError(f"{name} against {tag}: {idx.shape[0]} of {ok.numel()} elements outside c = {cc:g} "
                                 f"(worst ratios {out}, largest error {float(err.max()):.3g}), first at {idx[:6].tolist()}")
    return out


def _check_pad(ys, cout):
    B, nb, _, H, W, _ = ys.shape
    flat = ys.permute(0, 2, 1, 5, 3, 4).reshape(B, 2, nb * 8, H, W)
    assert not bool(flat[:, :, cout:].any()), "pad channels of a c8x2 output must be zero"


def _same_split(ys, y32, cout):
    hi, lo = from_c8x2(ys, cout, parts=True)
    whi, wlo = split_bf16(y32)
    assert torch.equal(hi.view(torch.int16), whi.view(torch.int16)) and torch.equal(lo.view(torch.int16), wlo.view(torch.int16)), \
        "the split output is not split_bf16 of the f32 output"


# ------------------------------------------------------------------ plain layers (stride 2, transposed)
def _plain(layer, B, cin, cout, Hi, Wi, act, seed, crop=None, split=None, fmt="both"):
    mode = GEO[layer][0]
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((B, cin, Hi, Wi), generator=g)
    wshape = (cin, cout, 3, 3) if mode == T2 else (cout, cin, 3, 3)
    w = torch.randn(wshape, generator=g) / math.sqrt(4.0 * cin)
    b = torch.randn(cout, generator=g) * 0.3
    Ho, Wo = (2 * Hi, 2 * Wi) if mode == T2 else ((Hi - 1) // 2 + 1, (Wi - 1) // 2 + 1)
    ohs, ows = crop or (Ho, Wo)
    emu, ref, bound = (t[:, :, :ohs, :ows] for t in _three(mode, x, w, b))
    wpk, bpk = (pack_convt_x3 if mode == T2 else pack_conv_x3)(w.to(DEV), b.to(DEV), layer)
    wpk, bpk = _guarded(wpk), _guarded(bpk)
    xs = [_guarded(to_c8x2(x.to(DEV)))] if split is None else [_guarded(to_c8x2(x[:, :split].to(DEV))),
                                                              _guarded(to_c8x2(x[:, split:].to(DEV)))]
    bs, ys = _split_out(B, cout, ohs, ows) if fmt in ("both", "split") else (None, None)
    b32, y32 = _out((B, cout, ohs, ows)) if fmt in ("both", "f32") else (None, None)
    _lib.call("nlspn_gconv_x3", xs[0].device, layer, xs[0], split or cin, xs[1] if split else None,
              cin - split if split else 0, wpk, bpk, ys, y32, None, None, None, None, None, None, B, Hi, Wi, cout, ohs, ows,
              act, 1.0, 0, _lib.STREAM)
    torch.cuda.synchronize()
    assert all(_guard_ok(bf) for bf in (bs, b32) if bf is not None), "a store outside the output"
    if ys is not None:
        _check_pad(ys, cout)
    return ys, y32, _act64(emu, act), _act64(ref, act), bound


PLAIN_CH = {GCX3_S2: (16, 128), GCX3_T2: (64, 64), GCX3_T2_C16: (64, 16)}
KIND = {GCX3_S2: "s2", GCX3_T2: "t2", GCX3_T2_C16: "t2_c16"}
PLAIN = (GCX3_S2, GCX3_T2, GCX3_T2_C16)


def _run_plain(layer, gh, gw, record, act=ACT_RELU, B=2, cin=None, cout=None, parity=0, crop=None, split=None, fmt="both",
               tag=""):
    mode = GEO[layer][0]
    ci, co = PLAIN_CH[layer]
    cin, cout = cin or ci, cout or co
    Hi, Wi = (gh, gw) if mode == T2 else (2 * gh - parity, 2 * gw - parity)
    ys, y32, emu, ref, bound = _plain(layer, B, cin, cout, Hi, Wi, act, seed=100 * layer + gh + gw, crop=crop, split=split,
                                      fmt=fmt)
    n = cin * (4 if mode == T2 else 9)
    e = E_ACT if act == ACT_TANH else 0.0
    name = f"{KIND[layer]}/{B}x{cin}>{cout}/{gh}x{gw}p{parity}{tag}"
    if y32 is not None:
        _check(name + "/f32", y32, emu, ref, bound, n, e, record=record)
    if ys is not None:
        _check(name + "/split", from_c8x2(ys, cout), emu, ref, bound, n, e, split=True, record=record)
    if ys is not None and y32 is not None:
        _same_split(ys, y32, cout)


@pytest.mark.parametrize("which", range(6))
@pytest.mark.parametrize("layer", PLAIN)
def test_band_and_tile_edges(layer, which, record_metric):
    """The computed grids; stride 2 at both input parities."""
    gh, gw = grids(layer)[which]
    for parity in ((0, 1) if GEO[layer][0] == S2 else (0,)):
        _run_plain(layer, gh, gw, record_metric, parity=parity)


@pytest.mark.parametrize("layer", PLAIN)
def test_channel_edges(layer, record_metric):
    """cin 40 = 16 + 24 and 56 = 32 + 24 from two sources (a partial last chunk: the cell blocks
    past a source's last read 0 through the descriptor's range; a partial 8-block: pad channels),
    cin 40 from one source, and cout 24 in a 64-channel tile (12 in the 16-channel one): pad
    channels of the split output zero, nothing stored beyond."""
    _run_plain(layer, 7, 21, record_metric, cin=40, split=16, parity=1, tag="/16+24")
    _run_plain(layer, 7, 21, record_metric, cin=56, split=32, tag="/32+24")
    _run_plain(layer, 7, 21, record_metric, cin=40, tag="/cin40")
    _run_plain(layer, 7, 21, record_metric, cout=24 if GEO[layer][4] == 64 else 12, parity=1, tag="/cout")


@pytest.mark.parametrize("off", [1, 7])
@pytest.mark.parametrize("layer", [GCX3_T2, GCX3_T2_C16])
def test_transposed_crops(layer, off, record_metric):
    gh, gw = 6, 41
    _run_plain(layer, gh, gw, record_metric, act=ACT_NONE, crop=(2 * gh - off, 2 * gw - off), tag=f"/crop{off}")


@pytest.mark.parametrize("fmt", ["split", "f32"])
@pytest.mark.parametrize("layer", PLAIN)
def test_one_output_format_alone(layer, fmt, record_metric):
    gh, gw = grids(layer)[0]
    _run_plain(layer, gh, gw, record_metric, fmt=fmt, tag="/" + fmt)


def test_tanh_epilogue(record_metric):
    """encode_aff's last layer: Tanh, both outputs (the initial h and its split copy)."""
    gh, gw = grids(GCX3_S2)[0]
    _run_plain(GCX3_S2, gh, gw, record_metric, act=ACT_TANH, cin=64, tag="/tanh")


# ------------------------------------------------------------------ the VALU kernel
@pytest.mark.parametrize("cin,Hi,Wi,in_div,crop", [(1, 27, 45, 10.0, None), (9, 28, 45, 10.0, (14, 20)), (9, 27, 46, 1.0, None)])
def test_small_valu_kernel(cin, Hi, Wi, in_div, crop, record_metric):
    """NLSPN_GCX3_S2_SMALL (cin 1 / 9 -> 16): f32 NCHW in, the f32 kernel's arithmetic; the output
    is the f32 NLSPN_GC_S2_SMALL output split, bit for bit."""
    B, cout = 2, 16
    g = torch.Generator().manual_seed(60 + cin + Hi)
    x = torch.rand((B, cin, Hi, Wi), generator=g) * in_div
    w = torch.randn((cout, cin, 3, 3), generator=g) / math.sqrt(4.0 * cin)
    b = torch.randn(cout, generator=g) * 0.3
    ohs, ows = crop or ((Hi - 1) // 2 + 1, (Wi - 1) // 2 + 1)
    ref = torch.relu(_conv64(S2, x.double() / in_div, w, b))[:, :, :ohs, :ows]
    bound = _conv64(S2, x.double() / in_div, w.abs(), b.abs())[:, :, :ohs, :ows]
    buf, ys = _split_out(B, cout, ohs, ows)
    xd, wd, bd = _guarded(x.to(DEV)), _guarded(w.to(DEV)), _guarded(b.to(DEV))
    _lib.call("nlspn_gconv_x3", xd.device, GCX3_S2_SMALL, xd, cin, None, 0, wd, bd, ys, None, None, None, None, None, None, None,
              B, Hi, Wi, cout, ohs, ows, ACT_RELU, in_div, 0, _lib.STREAM)
    torch.cuda.synchronize()
    assert _guard_ok(buf)
    # unsplit operands: emu = ref; the f32 VALU sum's cap (9 cin + 2 (+ 1 for the division)) 2^-24 < 2e-6
    _check(f"small/cin{cin}/{Hi}x{Wi}", from_c8x2(ys, cout), ref, ref, bound, 9 * cin + (in_div != 1.0), split=True,
           record=record_metric)
    y32 = torch.empty((B, cout, ohs, ows), device=DEV)
    _lib.call("nlspn_gconv", xd.device, GC_S2_SMALL, xd, cin, None, 0, wd, bd, y32, None, None, None, None, None, B, Hi, Wi,
              cout, ohs, ows, ACT_RELU, in_div, 0, _lib.STREAM)
    _same_split(ys, y32, cout)


# ------------------------------------------------------------------ ConvGRU
@functools.lru_cache(maxsize=None)
def _gru_ref(hc, B, H, W):
    """The ConvGRU cell (nlspnmodel.py:398-403) in float64, emulated (split operands) and
    unsplit; GRU2 alone on the reference's z (f32), r*h (f32, split when passed in) and qx (f32)."""
    g = torch.Generator().manual_seed(3 + hc + 7 * B + H * W)
    s = 1.0 / math.sqrt(6.0 * hc)
    wz, wr, wq = (torch.randn((hc, 2 * hc, 3, 3), generator=g) * s for _ in range(3))
    bias_z, bias_r, bias_q = (torch.randn(hc, generator=g) * 0.3 for _ in range(3))
    h = torch.tanh(torch.randn((B, hc, H, W), generator=g))
    x = torch.relu(torch.randn((B, hc, H, W), generator=g))
    hx, h64 = torch.cat([h, x], 1), h.double()
    R = dict(hc=hc, wz=wz, wr=wr, wq=wq, bias_z=bias_z, bias_r=bias_r, bias_q=bias_q, h=h, x=x)
    for k, (inp, w, b) in {"z": (hx, wz, bias_z), "r": (hx, wr, bias_r), "qx": (x, wq[:, hc:], bias_q)}.items():
        R["e_" + k], R["r_" + k], R["bd_" + k] = _three(S1, inp, w, b)
    R["z32"], R["qx32"] = torch.sigmoid(R["r_z"]).float(), R["r_qx"].float()
    R["rh32"] = (torch.sigmoid(R["r_r"]) * h64).float()
    e, r, bd = _three(S1, R["rh32"], wq[:, :hc])
    z = R["z32"].double()
    R["bd_q2"] = bd + R["qx32"].double().abs()
    R["e_hn"] = (1 - z) * h64 + z * torch.tanh(e + R["qx32"].double())
    R["r_hn"] = (1 - z) * h64 + z * torch.tanh(r + R["qx32"].double())
    return R


def _gru1(R, B, H, W):
    hc = R["hc"]
    w1 = torch.cat([R["wz"], R["wr"], R["wq"]], 0).to(DEV)
    b1 = torch.cat([R["bias_z"], R["bias_r"], R["bias_q"]], 0).to(DEV)
    wpk, bpk = (_guarded(t) for t in pack_conv_x3(w1, b1, GCX3_GRU1))
    h = _guarded(R["h"].to(DEV))
    hs, xs = _guarded(to_c8x2(h)), _guarded(to_c8x2(R["x"].to(DEV)))
    bz, z = _out((B, hc, H, W))
    bq, qx = _out((B, hc, H, W))
    br, rh = _split_out(B, hc, H, W)
    _lib.call("nlspn_gconv_x3", h.device, GCX3_GRU1, hs, hc, xs, hc, wpk, bpk, None, None, h, z, rh, qx, None, None,
              B, H, W, 3 * hc, 0, 0, ACT_NONE, 1.0, hc, _lib.STREAM)
    torch.cuda.synchronize()
    assert _guard_ok(bz) and _guard_ok(bq) and _guard_ok(br)
    return z, rh, qx


def _gru2(R, z, rhs, qx, B, H, W):
    hc = R["hc"]
    wpk, bpk = (_guarded(t) for t in pack_conv_x3(R["wq"][:, :hc].contiguous().to(DEV), R["bias_q"].to(DEV), GCX3_GRU2))
    h = _guarded(R["h"].to(DEV))
    b32, hn = _out((B, hc, H, W))
    bs, hns = _split_out(B, hc, H, W)
    _lib.call("nlspn_gconv_x3", h.device, GCX3_GRU2, rhs, hc, None, 0, wpk, bpk, None, None, h, z, None, qx, hn, hns,
              B, H, W, hc, 0, 0, ACT_NONE, 1.0, hc, _lib.STREAM)
    torch.cuda.synchronize()
    assert _guard_ok(b32) and _guard_ok(bs)
    return hn, hns


def gru_grids():
    """(B, H, W, hc): the uneven last band with an extra row, the empty last tile, one full band
    plus one pixel, 9x2, 1x1, a single row; hc 128 and 256 on 17x39 (two bands, 20 | 19)."""
    ex, em = grid_extra_row(GCX3_GRU1), grid_empty_tile(GCX3_GRU1)
    bm = _bwmax(S1, GEO[GCX3_GRU1][3])
    return [(2, *ex, 128), (2, *em, 128), (1, 5, bm + 1, 128), (2, 9, 2, 128), (2, 1, 1, 128), (1, 1, 2 * bm + 3, 128),
            (1, 17, 39, 128), (1, 17, 39, 256)]


def test_gru1_cases_cover_odd_and_even_tile_counts():
    par = set()
    for B, H, W, _ in gru_grids():
        nbands, bw, bwl = _bands(GCX3_GRU1, W)
        par.add((B * nbands * -(-H * bw // _npx_for(GCX3_GRU1, bwl))) % 2)
    assert par == {0, 1}


@pytest.mark.parametrize("case", range(8))
def test_gru1_per_element(case, record_metric):
    """GRU1's z, r*h (c8x2) and qx per element.  The qx tiles run K over x only."""
    B, H, W, hc = gru_grids()[case]
    R = _gru_ref(hc, B, H, W)
    z, rh, qx = _gru1(R, B, H, W)
    name = f"gru1/hc{hc}/{B}x{H}x{W}"
    _check(name + "/qx", qx, R["e_qx"], R["r_qx"], R["bd_qx"], 9 * hc, record=record_metric)
    _check(name + "/z", z, torch.sigmoid(R["e_z"]), torch.sigmoid(R["r_z"]), R["bd_z"], 18 * hc, E_ACT, record=record_metric)
    # r*h: |h| times r's bound, the f32 product's own rounding, then the split store
    h64 = R["h"].double()
    habs = h64.abs()
    _check(name + "/rh", from_c8x2(rh, hc), torch.sigmoid(R["e_r"]) * h64, torch.sigmoid(R["r_r"]) * h64, habs * R["bd_r"],
           18 * hc, habs * E_ACT, 2 * U * habs, split=True, record=record_metric)


@pytest.mark.parametrize("case", range(8))
def test_gru2_per_element(case, record_metric):
    """GRU2 fed the reference's z, r*h and qx: h' in f32 and its split copy."""
    B, H, W, hc = gru_grids()[case]
    R = _gru_ref(hc, B, H, W)
    hn, hns = _gru2(R, _guarded(R["z32"].to(DEV)), _guarded(to_c8x2(R["rh32"].to(DEV))), _guarded(R["qx32"].to(DEV)), B, H, W)
    name = f"gru2/hc{hc}/{B}x{H}x{W}"
    # h' = (1 - z) h + z q: z times q's bound, and the blend's four roundings of values <= |h| + 1
    z = R["z32"].double()
    extra = 4 * U * (R["h"].double().abs() + 1)
    _check(name + "/hn", hn, R["e_hn"], R["r_hn"], z * R["bd_q2"], 9 * hc, z * E_ACT, extra, record=record_metric)
    _check(name + "/hns", from_c8x2(hns, hc), R["e_hn"], R["r_hn"], z * R["bd_q2"], 9 * hc, z * E_ACT, extra, split=True)
    _same_split(hns, hn, hc)
