"""GPU: the forward of the GRU-mode convolutions (csrc/nlspn_gconv.h) per element against
float64, every instantiated preset by its own id, at the grids where the tiling can go wrong.

Each case calls the C ABI (nlspn_gconv, nlspn_gconv_gru_train, nlspn_gconv_affnorm) through
_lib.call on weights packed by pack_conv / pack_convt, and compares every output element with
torch's float64 convolution of the same f32 values on the CPU (F.conv2d / F.conv_transpose2d
with output_padding 1, crop, bias, activation, the ConvGRU formulas of nlspnmodel.py:398-403):
    |got - ref64| <= c * (sum |w||x| + |b|)  [+ e_act]
the bound computed by the same float64 convolution on absolute values.  ReLU and tanh are
1-Lipschitz and sigmoid' <= 1/4, so the pre-activation bound carries over; outputs that pass
through tanhf / expf get the absolute term e_act for the device function itself.

Bars.  Both sides form exact f32 products; any f32 summation order of n = cin x taps of them
plus the bias satisfies c <= (n + 2) * 2^-24, the cap (a transposed conv's element has 1, 2 or
4 taps by its output phase; GRU2 adds qx: n + 3; the VALU kernel's in_div is one more rounding
per term: n + 3).  Each element is asserted at min(bar, its own cap), so no assert exceeds
the cap.  The bar of a kind is 4x the worst ratio measured on an MI355X over every case of the
kind (recorded by record_metric as gconv_fwd/*), rounded up to one digit — the convention of
tests/test_gpu_gconv_bwd.py:
    kind    measured (worst case)                bar     smallest cap used
    s2      3.9e-7  id 0, 16 -> 256, 14x23       2e-6    (144 + 2) 2^-24 = 8.7e-6   presets 0, 1, 20, 23
    t2      3.2e-7  id 4, 32 -> 64, 17x39        2e-6    (16 + 2) 2^-24 = 1.07e-6   presets 4, 5, 21, 22, 25 (raw taps)
    gru1    3.5e-7  qx, hc 256, 17x39            2e-6    (1152 + 2) 2^-24 = 6.9e-5  presets 2, 16, 18
            (z 4.0e-8, r 2.6e-8, r*h 2.8e-8 beside e_act: sigmoid' <= 1/4)
    gru2    2.0e-7  q, hc 256, 17x39 (h' 1.5e-7) 8e-7    (1152 + 3) 2^-24 = 6.9e-5  presets 3, 17, 24
    small   1.5e-7  cin 1, 27x45                 7e-7    (9 + 3) 2^-24 = 7.2e-7     the VALU kernel
(tests/test_gpu_heads.py asserts 2e-6 at 1152 terms: the same order.)
e_act (cap 16 * 2^-24 = 9.5e-7: above it the device function is suspect), measured on the same
data with the activation on against off (tanh: a layer with act none, then tanh, against
float64 tanh of the stored f32 pre-activation; sigmoid: GRU1 with convz = convr = convq's x
half, whose pre-activation is then qx's, bit for bit):
    tanhf                8.1e-8 -> 4e-7        1 / (1 + expf(-u))   8.1e-8 -> 4e-7
The two-launch cell end to end: relative L2 5.2e-7 at worst (hc 256, 17x39), bar 1e-5.
Whole model, largest |native - module| per output (B = 1, T = 3): 1.9e-6 at 50x70 (two ulps of
a depth near 10; both paths were always right there) -> bar 8e-6; 1.9e-6 at 136x312.

Before the planner sized a tile for the narrowest band it cuts (gc_tile, nlspn_gconv_plan.h)
17 cases failed on the same device, each at exactly the pixels the window arithmetic
predicts: presets 0 / 20 at 14x23 (row 13, columns 12..15), 23 at 10x21, 1 at 17x37, 5 / 22 at
27x160 (output row 51, columns 216..219), GRU1 (2) at 17x39 (pixel (16, 20) of qx, z, r), GRU2
(17) and the cell at 17x39, the tanh and NaN cases at 14x23, and the whole model at 136x312
(0.036 against 1.9e-6).  They pass after; presets 3, 4, 16, 21 and 24 were never wrong.
"""
import functools
import math
import types

import pytest
import torch
import torch.nn.functional as F

from _gconv_bwd_cases import gc_tiling
from nlspn_eccv20_amd import NLSPNModel, _lib
from nlspn_eccv20_amd.gru import ACT_NONE, ACT_RELU, ACT_TANH, GC_S2_SMALL, pack_conv, pack_convt

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
SENT = -7777.0   # outputs are allocated with a guard tail of this value
GUARD = 4096

S1, S2, T2 = 0, 1, 2
# id -> (mode, NPX, XR, XP): a mirror of NLSPN_GC_CONFIGS for the batch / tile-count arithmetic
# of the cases only (what is launched is the library's own plan)
GEO = {0: (S2, 64, 12, 40), 1: (S2, 64, 10, 72), 2: (S1, 64, 6, 40), 3: (S1, 64, 8, 40), 4: (T2, 64, 6, 40),
       5: (T2, 256, 6, 80), 16: (S1, 64, 8, 40), 17: (S1, 64, 6, 40), 18: (S1, 128, 8, 40), 20: (S2, 64, 12, 40),
       21: (T2, 64, 6, 40), 22: (T2, 256, 6, 80), 23: (S2, 32, 8, 40), 24: (S1, 32, 6, 40), 25: (T2, 256, 6, 80)}
CO_TILE = {0: 64, 1: 16, 2: 64, 3: 64, 4: 64, 5: 16, 16: 64, 17: 64, 18: 64, 20: 64, 21: 64, 22: 16, 23: 64, 24: 64, 25: 16}

# asserted c per kind and e_act (module docstring); each case asserts its bar against its own cap
C = {"s2": 2e-6, "t2": 2e-6, "gru1": 2e-6, "gru2": 8e-7, "small": 7e-7}
E_TANH = 4e-7
E_SIG = 4e-7
E_CAP = 16 * U
BAR_CELL = 1e-5      # the two-launch cell end to end: tests/test_gpu_gconv_bwd.py's forward bar, relative L2
BAR_MODEL = 8e-6     # whole model, largest absolute difference native against modules


def cap(n):
    return (n + 2) * U


def _c(kind, n):
    """The asserted c of an element whose sum has n terms (a number, or a tensor per element):
    the kind's bar, never above the element's own cap."""
    return torch.clamp(torch.as_tensor(cap(n), dtype=torch.float64), max=C[kind])


def _tiles(layer, gh, gw):
    """(nbands, tiles per band) of gc_tile for the grid (the mirror of tests/_gconv_bwd_cases.py)."""
    t = gc_tiling(*GEO[layer], gh, gw)
    return t["nbands"], t["tpb"]


def _batch_for_wide_tiles(layer, gh, gw, cout):
    """The smallest batch at which nlspn_gconv keeps NLSPN_GC_S2 / NLSPN_GC_GRU2 on their own
    64-pixel presets (0 / 3): at least two workgroups per CU."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    nbands, tpb = _tiles(layer, gh, gw)
    per_image = -(-cout // CO_TILE[layer]) * nbands * tpb
    B = -(-2 * cus // per_image)
    assert B * per_image >= 2 * cus
    return B


def _conv64(mode, x, w, b, absval=False):
    x, w, b = x.double(), w.double(), None if b is None else b.double()
    if absval:
        x, w, b = x.abs(), w.abs(), None if b is None else b.abs()
    if mode == T2:
        return F.conv_transpose2d(x, w, b, stride=2, padding=1, output_padding=1)
    return F.conv2d(x, w, b, stride=2 if mode == S2 else 1, padding=1)


def _act64(y, act):
    return torch.relu(y) if act == ACT_RELU else torch.tanh(y) if act == ACT_TANH else y


def _out(*shape):
    n = math.prod(shape)
    buf = torch.full((n + GUARD,), SENT, device=DEV, dtype=torch.float32)
    return buf, buf[:n].view(*shape)


def _guard_ok(buf):
    return bool((buf[-GUARD:] == SENT).all())


def _check(name, got, ref, bound, c, e_abs=0.0, extra=0.0, record=None):
    """Every element: |got - ref| <= c * bound + e_abs + extra (numbers or tensors per element).
    Returns the worst (err - e_abs - extra) / bound, recorded as the measured c."""
    got = got.detach().double().cpu()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    err = (got - ref).abs()
    ratio = float(((err - e_abs - extra).clamp(min=0) / (bound + 1e-300)).nan_to_num(nan=float("inf")).max())
    if record:
        record(f"gconv_fwd/{name}", ratio)
    ok = err <= c * bound + e_abs + extra
    if not bool(ok.all()):
        idx = (~ok).nonzero()
        raise AssertionError(f"{name}: {idx.shape[0]} of {ok.numel()} elements outside c = {float(torch.as_tensor(c).max()):g} "
                             f"(worst ratio {ratio:.3g}), "
                             f"first at {idx[:6].tolist()}")
    return ratio


# ------------------------------------------------------------------ plain layers (stride 2, transposed)
def _plain(layer, B, cin, cout, Hi, Wi, act, seed, crop=None, split=None, nan_at=()):
    """One launch of a stride-2 / transposed preset and its float64 reference, pre-activation
    bound and term count.  crop: the stored (ohs, ows); split: c0 of a two-source input."""
    mode = GEO[layer][0]
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((B, cin, Hi, Wi), generator=g)
    for idx in nan_at:
        x[idx] = float("nan")
    wshape = (cin, cout, 3, 3) if mode == T2 else (cout, cin, 3, 3)
    w = torch.randn(wshape, generator=g) / math.sqrt(4.0 * cin)
    b = torch.randn(cout, generator=g) * 0.3
    Ho, Wo = (2 * Hi, 2 * Wi) if mode == T2 else ((Hi - 1) // 2 + 1, (Wi - 1) // 2 + 1)
    ohs, ows = crop or (Ho, Wo)
    pre = _conv64(mode, x, w, b)[:, :, :ohs, :ows]
    bound = _conv64(mode, x, w, b, True)[:, :, :ohs, :ows]
    wpk, bpk = (pack_convt if mode == T2 else pack_conv)(w.to(DEV), b.to(DEV), layer)
    xs = [x.to(DEV)] if split is None else [x[:, :split].contiguous().to(DEV), x[:, split:].contiguous().to(DEV)]
    buf, y = _out(B, cout, ohs, ows)
    _lib.call("nlspn_gconv", xs[0].device, layer, xs[0], xs[0].shape[1], xs[1] if split else None,
              xs[1].shape[1] if split else 0, wpk, bpk, y, None, None, None, None, None, B, Hi, Wi, cout, ohs, ows, act, 1.0,
              0, _lib.STREAM)
    torch.cuda.synchronize()
    assert _guard_ok(buf), "a store past the last stored element (beyond cout or past the crop)"
    n = 9 * cin   # the terms of an output element; transposed: 1, 2 or 4 taps by output phase (oy & 1, ox & 1)
    if mode == T2:
        n = cin * (1 + torch.arange(ohs)[:, None] % 2) * (1 + torch.arange(ows)[None, :] % 2)
    return y, _act64(pre, act), bound, n


PLAIN_CH = {0: (16, 256), 20: (16, 64), 23: (16, 64), 1: (32, 16), 4: (32, 64), 21: (32, 64), 5: (16, 8), 22: (16, 8)}
KIND = {0: "s2", 1: "s2", 20: "s2", 23: "s2", 4: "t2", 5: "t2", 21: "t2", 22: "t2", 25: "t2"}


def _run_plain(layer, gh, gw, record, act=ACT_RELU, B=2, cin=None, cout=None, parity=0, crop=None, split=None, tag=""):
    mode = GEO[layer][0]
    ci, co = PLAIN_CH[layer]
    cin, cout = cin or ci, cout or co
    Hi, Wi = (gh, gw) if mode == T2 else (2 * gh - parity, 2 * gw - parity)
    y, ref, bound, n = _plain(layer, B, cin, cout, Hi, Wi, act, seed=100 * layer + gh + gw, crop=crop, split=split)
    kind = KIND[layer]
    e = E_TANH if act == ACT_TANH else 0.0
    return _check(f"{kind}/id{layer}/{B}x{cin}>{cout}/{gh}x{gw}p{parity}{tag}", y, ref, bound, _c(kind, n), e, record=record)


# a. every preset at the smallest grid whose narrower last band used to overrun the window, and
# at the smallest grid with an empty tile in the last band
GRIDS_A = [(0, 14, 23), (0, 4, 33), (20, 14, 23), (20, 4, 33), (23, 10, 21), (23, 2, 33), (1, 17, 37), (1, 3, 43),
           (4, 17, 39), (4, 3, 43), (21, 17, 39), (21, 3, 43), (5, 27, 160), (5, 4, 129), (22, 27, 160), (22, 4, 129)]


@pytest.mark.parametrize("layer,gh,gw", GRIDS_A)
def test_uneven_last_band_and_empty_tiles(layer, gh, gw, record_metric):
    """a. Stride 2: both input parities.  Preset 0 at the batch that keeps it on 64-pixel tiles."""
    B = _batch_for_wide_tiles(0, gh, gw, PLAIN_CH[0][1]) if layer == 0 else 2
    for parity in ((0, 1) if GEO[layer][0] == S2 else (0,)):
        _run_plain(layer, gh, gw, record_metric, B=B, parity=parity)


# b. one full band and one pixel more; npx shrunk by a narrow band; one row
GRIDS_B = [(20, 5, 19), (20, 5, 20), (1, 5, 35), (1, 5, 36), (4, 5, 39), (4, 5, 40), (5, 5, 79), (5, 5, 80)] + \
          [(layer, gh, gw) for layer in (20, 1, 4, 5) for gh, gw in ((9, 2), (1, 1), (1, 80))]


@pytest.mark.parametrize("layer,gh,gw", GRIDS_B)
def test_band_and_tile_edges(layer, gh, gw, record_metric):
    _run_plain(layer, gh, gw, record_metric, parity=(gh + gw) % 2)


# c. channel edges
@pytest.mark.parametrize("layer", [20, 1, 4, 5])
def test_channel_edges(layer, record_metric):
    """c. cin 20 (padded chunks, the last chunk's channel bound), cout not a multiple of the co
    tile (72 on 64, 8 on 16: nothing stored beyond cout), and the accepted two-source input
    c0 = 16, c1 = 16 = the conv of the concatenation."""
    wide = CO_TILE[layer] == 64
    _run_plain(layer, 7, 21, record_metric, cin=20, parity=1, tag="/cin20")
    _run_plain(layer, 7, 21, record_metric, cout=72 if wide else 8, tag="/cout")
    _run_plain(layer, 7, 21, record_metric, cin=32, split=16, parity=1, tag="/split16")


# d. transposed crops: _clip_as stores ohs x ows of the 2 Hi x 2 Wi output, up to seven off
@pytest.mark.parametrize("layer", [4, 5, 21, 22])
@pytest.mark.parametrize("off", [0, 1, 7])
def test_transposed_crops(layer, off, record_metric):
    gh, gw = 6, 41
    _run_plain(layer, gh, gw, record_metric, act=ACT_NONE, crop=(2 * gh - off, 2 * gw - off), tag=f"/crop{off}")


def test_tanh_epilogue_and_its_device_error(record_metric):
    """e_act of tanhf: the same launch with the activation off, then on; the on output against
    float64 tanh of the stored f32 pre-activation.  Then the tanh layer against float64."""
    worst = 0.0
    for layer, gh, gw in ((20, 14, 23), (1, 17, 37), (4, 17, 39)):
        mode, (cin, cout) = GEO[layer][0], PLAIN_CH[layer]
        Hi, Wi = (gh, gw) if mode == T2 else (2 * gh, 2 * gw)
        u, _, _, _ = _plain(layer, 2, cin, cout, Hi, Wi, ACT_NONE, seed=7)
        t, ref, bound, n = _plain(layer, 2, cin, cout, Hi, Wi, ACT_TANH, seed=7)
        worst = max(worst, float((t.double().cpu() - torch.tanh(u.double().cpu())).abs().max()))
        assert float(u.abs().max()) > 2.0   # the pre-activations reach tanh's curved range
        _check(f"{KIND[layer]}/id{layer}/tanh/{gh}x{gw}", t, ref, bound, _c(KIND[layer], n), E_TANH)
    record_metric("gconv_fwd/e_act/tanhf", worst)
    assert worst <= E_TANH <= E_CAP, worst


# ------------------------------------------------------------------ ConvGRU
@functools.lru_cache(maxsize=None)
def _gru_ref(hc, B, H, W, gru2_only=False):
    """The ConvGRU cell (nlspnmodel.py:398-403) in float64 on f32 values, the bound of every
    conv beside it (bd_*), and GRU2 alone on the f32-rounded z, r*h and qx of that reference."""
    g = torch.Generator().manual_seed(3 + hc + 7 * B + H * W)
    s = 1.0 / math.sqrt(6.0 * hc)
    wz, wr, wq = (torch.randn((hc, 2 * hc, 3, 3), generator=g) * s for _ in range(3))
    bias_z, bias_r, bias_q = (torch.randn(hc, generator=g) * 0.3 for _ in range(3))
    h = torch.tanh(torch.randn((B, hc, H, W), generator=g))
    x = torch.relu(torch.randn((B, hc, H, W), generator=g))
    hx, h64 = torch.cat([h, x], 1), h.double()
    R = dict(hc=hc, wz=wz, wr=wr, wq=wq, bias_z=bias_z, bias_r=bias_r, bias_q=bias_q, h=h, x=x)
    R["z"] = torch.sigmoid(_conv64(S1, hx, wz, bias_z))
    R["r"] = torch.sigmoid(_conv64(S1, hx, wr, bias_r))
    R["rh"] = R["r"] * h64
    R["qx"] = _conv64(S1, x, wq[:, hc:], bias_q)
    if not gru2_only:  # (GRU1's bounds and the cell end to end)
        R["bd_z"], R["bd_r"] = _conv64(S1, hx, wz, bias_z, True), _conv64(S1, hx, wr, bias_r, True)
        R["bd_qx"] = _conv64(S1, x, wq[:, hc:], bias_q, True)
        R["q"] = torch.tanh(_conv64(S1, R["rh"], wq[:, :hc], None) + R["qx"])
        R["hn"] = (1 - R["z"]) * h64 + R["z"] * R["q"]
    z32, rh32, qx32 = R["z"].float(), R["rh"].float(), R["qx"].float()
    R["z32"], R["rh32"], R["qx32"] = z32, rh32, qx32
    R["q2"] = torch.tanh(_conv64(S1, rh32, wq[:, :hc], None) + qx32.double())
    R["bd_q2"] = _conv64(S1, rh32, wq[:, :hc], None, True) + qx32.double().abs()
    R["hn2"] = (1 - z32.double()) * h64 + z32.double() * R["q2"]
    return R


def _gru1(layer, R, B, H, W, train=False, wz=None, wr=None, bias_z=None, bias_r=None):
    """GRU1 by preset id (nlspn_gconv) or through nlspn_gconv_gru_train (preset 2, also r)."""
    hc = R["hc"]
    w1 = torch.cat([R["wz"] if wz is None else wz, R["wr"] if wr is None else wr, R["wq"]], 0).to(DEV)
    b1 = torch.cat([R["bias_z"] if bias_z is None else bias_z, R["bias_r"] if bias_r is None else bias_r, R["bias_q"]], 0)
    wpk, bpk = pack_conv(w1, b1.to(DEV), layer)
    h, x = R["h"].to(DEV), R["x"].to(DEV)
    bufs = [_out(B, hc, H, W) for _ in range(4)]
    z, rh, qx, r = (o[1] for o in bufs)
    if train:
        _lib.call("nlspn_gconv_gru_train", h.device, 1, h, x, hc, wpk, bpk, h, z, rh, qx, None, r, None, B, H, W, hc,
                  _lib.STREAM)
    else:
        _lib.call("nlspn_gconv", h.device, layer, h, hc, x, hc, wpk, bpk, None, h, z, rh, qx, None, B, H, W, 3 * hc, 0, 0,
                  ACT_NONE, 1.0, hc, _lib.STREAM)
    torch.cuda.synchronize()
    assert all(_guard_ok(b) for b, _ in bufs)
    return z, rh, qx, (r if train else None)


def _gru2(layer, R, z, rh, qx, B, H, W, train=False):
    """GRU2 by preset id (nlspn_gconv) or through nlspn_gconv_gru_train (NLSPN_GC_GRU2, also q)."""
    hc = R["hc"]
    wpk, bpk = pack_conv(R["wq"][:, :hc].contiguous().to(DEV), R["bias_q"].to(DEV), layer)
    h = R["h"].to(DEV)
    bufs = [_out(B, hc, H, W) for _ in range(2)]
    hn, q = (o[1] for o in bufs)
    if train:
        _lib.call("nlspn_gconv_gru_train", h.device, 2, rh, None, 0, wpk, bpk, h, z, None, qx, hn, None, q, B, H, W, hc,
                  _lib.STREAM)
    else:
        _lib.call("nlspn_gconv", h.device, layer, rh, hc, None, 0, wpk, bpk, None, h, z, None, qx, hn, B, H, W, hc, 0, 0,
                  ACT_NONE, 1.0, hc, _lib.STREAM)
    torch.cuda.synchronize()
    assert all(_guard_ok(b) for b, _ in bufs)
    return hn, (q if train else None)


# (B, H, W): an uneven last band (17x39: 20 | 19), an empty last tile (3x43), and one-band grids
# whose pixel-tile count B * nbands * tpb is odd for the 64-pixel (17x38: 11) and the 128-pixel
# (3x38: 1) GRU1 presets — a qx workgroup takes two pixel tiles, the last one alone when odd
GRU_GRIDS = [(2, 17, 39), (2, 3, 43), (1, 17, 38), (1, 3, 38)]


def test_gru1_cases_cover_odd_and_even_tile_counts():
    for layer in (2, 16, 18):
        par = {(B * math.prod(_tiles(layer, H, W))) % 2 for B, H, W in GRU_GRIDS}
        assert par == {0, 1}, (layer, par)


@pytest.mark.parametrize("B,H,W", GRU_GRIDS)
@pytest.mark.parametrize("hc", [128, 256])
@pytest.mark.parametrize("layer", [2, 16, 18, "train"])
def test_gru1_per_element(layer, hc, B, H, W, record_metric):
    """e. GRU1's z, r*h and qx (through nlspn_gconv_gru_train also r) per element.  The qx tiles
    run K over x only."""
    R = _gru_ref(hc, B, H, W)
    train = layer == "train"
    z, rh, qx, r = _gru1(2 if train else layer, R, B, H, W, train=train)
    c = C["gru1"]
    assert c <= cap(9 * hc) and E_SIG <= E_CAP
    name = f"gru1/id{layer}/hc{hc}/{B}x{H}x{W}"
    _check(name + "/qx", qx, R["qx"], R["bd_qx"], c, record=record_metric)
    _check(name + "/z", z, R["z"], R["bd_z"], c, E_SIG, record=record_metric)
    # r*h: |h| times r's bound, and the product's own rounding
    habs = R["h"].double().abs()
    _check(name + "/rh", rh, R["rh"], habs * R["bd_r"], c, habs * E_SIG, 2 * U * R["rh"].abs(), record=record_metric)
    if train:
        _check(name + "/r", r, R["r"], R["bd_r"], c, E_SIG, record=record_metric)


@pytest.mark.parametrize("B,H,W", [(2, 23, 39), (2, 5, 51)])
def test_gru1_128_pixel_tiles(B, H, W, record_metric):
    """a. Preset 18 (128-pixel tiles) at its own smallest grid with an uneven last band that
    used to overrun (23x39) and with an empty last tile (5x51)."""
    test_gru1_per_element(18, 128, B, H, W, record_metric)


def _check_gru2(name, R, hn, q, record):
    c = C["gru2"]
    assert c <= (9 * R["hc"] + 3) * U and E_TANH <= E_CAP   # 9 hc products and qx
    if q is not None:
        _check(name + "/q", q, R["q2"], R["bd_q2"], c, E_TANH, record=record)
    # h' = (1 - z) h + z q: z times q's bound, and the blend's four roundings of values <= |h| + 1
    z = R["z32"].double()
    _check(name + "/hn", hn, R["hn2"], z * R["bd_q2"], c, z * E_TANH, 4 * U * (R["h"].double().abs() + 1), record=record)


@pytest.mark.parametrize("B,H,W", GRU_GRIDS)
@pytest.mark.parametrize("hc", [128, 256])
@pytest.mark.parametrize("layer", [3, 17, 24, "train"])
def test_gru2_per_element(layer, hc, B, H, W, record_metric):
    """e. GRU2 fed the f32 z, r*h and qx of the float64 reference: h' (through
    nlspn_gconv_gru_train also q) has a per-element bound of its own."""
    R = _gru_ref(hc, B, H, W)
    train = layer == "train"
    hn, q = _gru2(3 if train else layer, R, R["z32"].to(DEV), R["rh32"].to(DEV), R["qx32"].to(DEV), B, H, W, train=train)
    _check_gru2(f"gru2/id{layer}/hc{hc}/{B}x{H}x{W}", R, hn, q, record_metric)


def test_gru2_32_pixel_tiles_one_row(record_metric):
    """a. Preset 24 (32-pixel tiles) at 1x65: two bands of one row, the last band's second tile
    partly empty."""
    test_gru2_per_element(24, 128, 2, 1, 65, record_metric)


@pytest.mark.parametrize("H,W", [(17, 39), (3, 43)])
def test_gru2_on_its_own_wide_tiles(H, W, record_metric):
    """a. NLSPN_GC_GRU2 stays on preset 3 (64-pixel tiles) only with two workgroups per CU:
    the batch that reaches it (ids 16 / 17 cover the same tilings unconditionally)."""
    B = _batch_for_wide_tiles(3, H, W, 128)
    R = _gru_ref(128, B, H, W, gru2_only=True)
    hn, _ = _gru2(3, R, R["z32"].to(DEV), R["rh32"].to(DEV), R["qx32"].to(DEV), B, H, W)
    _check_gru2(f"gru2/id3wide/hc128/{B}x{H}x{W}", R, hn, None, record_metric)


@pytest.mark.parametrize("H,W", [(9, 2), (1, 1), (1, 80)])
def test_gru_band_and_tile_edges(H, W, record_metric):
    """b. The stride-1 presets where a narrow band shrinks npx (9x2, 1x1) and on one row (1x80);
    one full band and one pixel more are GRU_GRIDS' 17x38 and 17x39."""
    test_gru1_per_element(2, 128, 2, H, W, record_metric)
    test_gru2_per_element(3, 128, 2, H, W, record_metric)


@pytest.mark.parametrize("B,H,W", GRU_GRIDS[:2])
@pytest.mark.parametrize("hc", [128, 256])
def test_gru_cell_end_to_end(hc, B, H, W, record_metric):
    """e. The two-launch cell, GRU2 reading GRU1's own outputs, against float64: relative L2
    within the forward bar of tests/test_gpu_gconv_bwd.py's cell test."""
    R = _gru_ref(hc, B, H, W)
    z, rh, qx, _ = _gru1(2, R, B, H, W)
    hn, _ = _gru2(3, R, z, rh, qx, B, H, W)
    e = float((hn.double().cpu() - R["hn"]).norm() / R["hn"].norm())
    record_metric(f"gconv_fwd/cell/hc{hc}/{B}x{H}x{W}", e)
    assert e <= BAR_CELL, e


def test_sigmoid_device_error(record_metric):
    """e_act of 1 / (1 + expf(-u)): GRU1 with convz = convr = [0 | convq's x half] and convq's
    bias, so z's and r's pre-activation is qx's (the h half adds exact zeros, the x chunks run
    in the same order): z and r against float64 sigmoid of the stored f32 qx."""
    B, H, W, hc = 2, 17, 39, 128
    R = _gru_ref(hc, B, H, W)
    wzx = torch.cat([torch.zeros_like(R["wq"][:, :hc]), R["wq"][:, hc:]], 1)
    z, rh, qx, r = _gru1(2, R, B, H, W, train=True, wz=wzx, wr=wzx, bias_z=R["bias_q"], bias_r=R["bias_q"])
    want = torch.sigmoid(qx.double().cpu())
    worst = max(float((z.double().cpu() - want).abs().max()), float((r.double().cpu() - want).abs().max()))
    record_metric("gconv_fwd/e_act/sigmoid", worst)
    assert float(qx.abs().max()) > 2.0
    assert worst <= E_SIG <= E_CAP, worst


# ------------------------------------------------------------------ f. the fused affinity normalisation
@pytest.mark.parametrize("gh,gw", [(27, 160), (4, 129)])
@pytest.mark.parametrize("kind", ["AS", "ASS", "TC", "TGASS"])
def test_affnorm_bitequal_and_raw_taps(kind, gh, gw, record_metric):
    """f. nlspn_gconv_affnorm (id 25) is bit-equal to id 5 followed by affinity_normalization,
    crop included, and the raw taps are inside the per-element bound."""
    from nlspn_eccv20_amd.propagation import affinity_normalization
    B, cin, K = 2, 16, 8
    ohs, ows = 2 * gh - 3, 2 * gw - 1
    raw, ref, bound, n = _plain(5, B, cin, K, gh, gw, ACT_NONE, seed=25, crop=(ohs, ows))
    _check(f"t2/id25raw/{gh}x{gw}", raw, ref, bound, _c("t2", n), record=record_metric)
    # (the same generator sequence as _plain: the same input and weights)
    g = torch.Generator().manual_seed(25)
    x = torch.randn((B, cin, gh, gw), generator=g)
    w = torch.randn((cin, K, 3, 3), generator=g) / math.sqrt(4.0 * cin)
    b = torch.randn(K, generator=g) * 0.3
    wpk, bpk = pack_convt(w.to(DEV), b.to(DEV), 25)
    assert torch.equal(wpk, pack_convt(w.to(DEV), b.to(DEV), 5)[0])
    gamma = torch.tensor([0.37], device=DEV)
    buf, fused = _out(B, K + 1, ohs, ows)
    xd = x.to(DEV)
    _lib.call("nlspn_gconv_affnorm", xd.device, xd, cin, wpk, bpk, fused, gamma, _lib.AFF_KINDS[kind], B, gh, gw, K, ohs,
              ows, ACT_NONE, _lib.STREAM)
    torch.cuda.synchronize()
    assert _guard_ok(buf)
    want = affinity_normalization(raw.contiguous(), gamma, kind)
    assert want.shape == fused.shape and torch.equal(fused, want), float((fused - want).abs().max())


# ------------------------------------------------------------------ g. the VALU kernel
@pytest.mark.parametrize("cin,Hi,Wi,in_div,crop", [(1, 27, 45, 10.0, None), (1, 28, 46, 10.0, (13, 22)),
                                                   (9, 27, 46, 1.0, None), (9, 28, 45, 10.0, (14, 20))])
def test_small_valu_kernel(cin, Hi, Wi, in_div, crop, record_metric):
    """g. NLSPN_GC_S2_SMALL (cin 1 / 9 -> 16): odd and even input sizes, in_div, a crop; the
    reference divides in float64 (the f32 division is one more rounding per term)."""
    B, cout = 2, 16
    g = torch.Generator().manual_seed(60 + cin + Hi)
    x = torch.rand((B, cin, Hi, Wi), generator=g) * in_div
    w = torch.randn((cout, cin, 3, 3), generator=g) / math.sqrt(4.0 * cin)
    b = torch.randn(cout, generator=g) * 0.3
    ohs, ows = crop or ((Hi - 1) // 2 + 1, (Wi - 1) // 2 + 1)
    ref = torch.relu(_conv64(S2, x.double() / in_div, w, b))[:, :, :ohs, :ows]
    bound = _conv64(S2, x.double() / in_div, w, b, True)[:, :, :ohs, :ows]
    buf, y = _out(B, cout, ohs, ows)
    xd, wd, bd = x.to(DEV), w.to(DEV).contiguous(), b.to(DEV)
    _lib.call("nlspn_gconv", xd.device, GC_S2_SMALL, xd, cin, None, 0, wd, bd, y, None, None, None, None, None, B, Hi, Wi,
              cout, ohs, ows, ACT_RELU, in_div, 0, _lib.STREAM)
    torch.cuda.synchronize()
    assert _guard_ok(buf)
    assert C["small"] <= (9 * cin + 2 + (in_div != 1.0)) * U
    _check(f"small/cin{cin}/{Hi}x{Wi}", y, ref, bound, C["small"], record=record_metric)


# ------------------------------------------------------------------ h. padding and NaN
@pytest.mark.parametrize("layer,gh,gw,seam", [(20, 14, 23, 2 * 12 - 1), (1, 5, 43, 2 * 22 - 1), (4, 3, 43, 22), (5, 4, 129, 65)])
def test_nan_reaches_exactly_the_reference_outputs(layer, gh, gw, seam):
    """h. The zero padding is an out-of-range buffer offset, and a band's window overlaps its
    neighbour's: one NaN at a border cell and one at the input column two bands share.  The set
    of NaN outputs equals the float64 reference's exactly (ReLU keeps NaN), every other element
    is within the bound."""
    mode, (cin, cout) = GEO[layer][0], PLAIN_CH[layer]
    Hi, Wi = (gh, gw) if mode == T2 else (2 * gh, 2 * gw)
    nan_at = [(0, 0, 0, 0), (1, cin - 1, Hi - 1, Wi - 1), (1, 3, Hi // 2, seam)]
    y, ref, bound, n = _plain(layer, 2, cin, cout, Hi, Wi, ACT_RELU, seed=8, nan_at=nan_at)
    got = y.double().cpu()
    nan_ref = torch.isnan(ref)
    assert 3 <= int(nan_ref[:, 0].sum()) <= 27
    assert torch.equal(torch.isnan(got), nan_ref), (int(torch.isnan(got).sum()), int(nan_ref.sum()))
    fin = ~nan_ref
    _check(f"{KIND[layer]}/id{layer}/nan", torch.where(fin, got, 0.0), torch.where(fin, ref, 0.0),
           torch.where(fin, bound, 1.0), _c(KIND[layer], n))


def test_nan_in_the_gru(record_metric):
    """h. The same through GRU1: a NaN in h and one in x at the band seam of 17x39."""
    B, H, W, hc = 2, 17, 39, 128
    R = dict(_gru_ref(hc, B, H, W))
    h, x = R["h"].clone(), R["x"].clone()
    h[0, 5, 0, 0] = float("nan")
    x[1, 7, 9, 20] = float("nan")
    R["h"], R["x"] = h, x
    hx = torch.cat([h, x], 1)
    z64 = torch.sigmoid(_conv64(S1, hx, R["wz"], R["bias_z"]))
    qx64 = _conv64(S1, x, R["wq"][:, hc:], R["bias_q"])
    z, rh, qx, _ = _gru1(2, R, B, H, W)
    assert torch.equal(torch.isnan(z.cpu()), torch.isnan(z64)) and int(torch.isnan(z64)[:, 0].sum()) == 4 + 9
    assert torch.equal(torch.isnan(qx.cpu()), torch.isnan(qx64)) and int(torch.isnan(qx64)[:, 0].sum()) == 9


# ------------------------------------------------------------------ i. the whole model
T = 3


def _model(H, W, seed=5, hc=128):
    args = types.SimpleNamespace(prop_kernel=3, affinity="TGASS", affinity_gamma=0.5, prop_time=T,
                                 preserve_input=True, always_clip=False, conf_prop=True, offset=True,
                                 network="resnet34", from_scratch=True, zero_init_aff=False, use_GRU=True,
                                 use_S2D=False, GRU_hidden_dim=hc, GRU_input_dim=hc, lr=1e-3, max_depth=10.0,
                                 patch_height=H, patch_width=W, model_name="NLSPN")
    torch.manual_seed(seed)
    m = NLSPNModel(args).to(DEV).eval()
    with torch.no_grad():  # weights and biases of a trained scale
        for mod in (m.encode_dep, m.encode_aff, m.GRU, m.decode_aff):
            for p in mod.parameters():
                p.add_(0.02 * torch.randn_like(p))
    return m


def _model_diff(H, W):
    """Largest |native - module| per output of propagate_heads (B = 1, T = 3, GRU mode)."""
    m = _model(H, W)
    g = torch.Generator(device=DEV).manual_seed(9)
    pred_init = torch.rand((1, 1, H, W), device=DEV, generator=g) * 10
    dep = pred_init * (torch.rand((1, 1, H, W), device=DEV, generator=g) < 0.02)
    off_aff = torch.randn((1, 24, H, W), device=DEV, generator=g)
    conf = torch.rand((1, 1, H, W), device=DEV, generator=g)
    outs = {}
    for native in (True, False):
        m.native_gru = native
        with torch.no_grad():
            o = m.propagate_heads(pred_init, off_aff, conf, dep)
        outs[native] = [p.clone() for p in o["pred_inter"]] + [o["pred"].clone()]
    assert len(outs[True]) == T + 1
    return [float((a.double() - b.double()).abs().max()) for a, b in zip(outs[True], outs[False])]


def test_whole_model_at_a_size_the_planner_got_wrong(record_metric):
    """i. 136x312 (1/4 scale 34x78, 1/8 scale 17x39: uneven bands in the last encoder conv and
    the ConvGRU): native against native_gru = False, the largest absolute difference per output
    (not an RMSE: one wrong 1/8-scale pixel vanishes in a mean) within 4x the largest difference
    at 50x70, where both paths were right."""
    small = _model_diff(50, 70)
    big = _model_diff(136, 312)
    for i, (a, b) in enumerate(zip(small, big)):
        record_metric(f"gconv_fwd/model/50x70/out{i}", a)
        record_metric(f"gconv_fwd/model/136x312/out{i}", b)
    assert max(big) <= BAR_MODEL, (big, small)
