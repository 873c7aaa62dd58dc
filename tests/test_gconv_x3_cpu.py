"""CPU: the split-bf16 GRU-mode convolutions (csrc/nlspn_gconv_x3.h) off the device: split_bf16
and the c8x2 layout helpers, the weight packers, every refusal of nlspn_gconv_x3 before a device
call, the unit's resource remarks (no scratch), the model's gru_precision switch, and the
emulation the GPU tests are held against.

The emulation (emu_*) is the contract in float64 torch: every convolution the matrix cores run
is conv(w_hi, x_hi) + conv(w_hi, x_lo) + conv(w_lo, x_hi) with (hi, lo) = split_bf16 of the f32
weights (once) and of each activation where it is produced; the VALU first layers and the last
decoder layer are plain convolutions of unsplit operands; epilogues in float64.  ``carry`` is
what a layer end does to the activation it hands on: the kernels hold f32 there
(``carry32``), the yardstick run keeps float64 (``carry64``).  The two runs agree to 2.5e-6
relative L2 per chain (a quarter of the GPU tests' 1e-5 bar): a one-ulp difference in where a
split lands cannot by itself use up that bar.  Measured here: encode_dep 1.6e-6, encode_aff
1.2e-6, gru 2.2e-6, decode_aff 6.5e-7 (the two runs split different values, so what is left of
an activation after its split, up to 2^-17 of it, differs between them).
"""
import ctypes
import os
import subprocess
import sys
import types

import pytest
import torch
import torch.nn.functional as F

from nlspn_eccv20_amd import NLSPNModel, _lib
from nlspn_eccv20_amd import gru as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nlspn_eccv20_amd", "csrc")
P = ctypes.c_void_p(64)  # never dereferenced: validation fails first


# ------------------------------------------------------------------ split_bf16 and the layout
def test_split_bf16_parts_and_bound():
    g = torch.Generator().manual_seed(1)
    a = torch.randn(1_000_000, generator=g)
    hi, lo = G.split_bf16(a)
    assert hi.dtype == lo.dtype == torch.bfloat16
    assert torch.equal(hi, a.to(torch.bfloat16))                       # RNE bf16 of a
    assert torch.equal(lo, (a - hi.float()).to(torch.bfloat16))        # RNE bf16 of the f32 difference
    # RNE by hand on the bit pattern: add 0x7fff + the kept lsb, drop 16 bits
    bits = a.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    rne = ((bits + 0x7FFF + ((bits >> 16) & 1)) >> 16) & 0xFFFF
    assert torch.equal(hi.view(torch.int16).to(torch.int64) & 0xFFFF, rne)
    err = (a.double() - hi.double() - lo.double()).abs() / a.double().abs()
    assert float(err.max()) <= 2.0 ** -17
    assert float(err.max()) > 2.0 ** -18                               # the bound is 2^-17, not 2^-18
    assert float(((a.double() - hi.double()).abs() / a.double().abs()).max()) <= 2.0 ** -8


@pytest.mark.parametrize("C", [1, 8, 9, 20, 128])
def test_c8x2_round_trip(C):
    g = torch.Generator().manual_seed(C)
    x = torch.randn((2, C, 5, 7), generator=g) * 3
    y = G.to_c8x2(x)
    nb = (C + 7) // 8
    assert y.shape == (2, nb, 2, 5, 7, 8) and y.dtype == torch.bfloat16 and y.is_contiguous()
    hi, lo = G.split_bf16(x)
    ghi, glo = G.from_c8x2(y, C, parts=True)
    assert torch.equal(ghi, hi) and torch.equal(glo, lo)
    assert torch.equal(G.from_c8x2(y, C), hi.float() + lo.float())
    # block k's hi plane holds channels 8k .. 8k + 7 of hi, its lo plane those of lo; pad channels are zero
    assert torch.equal(y[1, nb - 1, 0, 3, 4, 0], hi[1, 8 * (nb - 1), 3, 4])
    assert torch.equal(y[1, nb - 1, 1, 3, 4, 0], lo[1, 8 * (nb - 1), 3, 4])
    flat = y.permute(0, 2, 1, 5, 3, 4).reshape(2, 2, nb * 8, 5, 7)
    assert not bool(flat[:, :, C:].any())


# ------------------------------------------------------------------ the packers
@pytest.mark.parametrize("cout,cin,layer", [(256, 16, G.GCX3_S2), (128, 256, G.GCX3_S2), (72, 20, G.GCX3_S2),
                                            (384, 256, G.GCX3_GRU1), (128, 128, G.GCX3_GRU2), (64, 40, G.GCX3_GRU2)])
def test_pack_conv_x3_round_trip(cout, cin, layer):
    g = torch.Generator().manual_seed(cout + cin)
    w = torch.randn((cout, cin, 3, 3), generator=g)
    b = torch.randn(cout, generator=g)
    wpk, bpk = G.pack_conv_x3(w, b, layer)
    co, cc, tr = G._layout_of(G._X3, layer)
    assert (co, cc, tr) == (64, 16, False)
    ct, cp = -(-cout // co), -(-cin // cc) * cc
    assert wpk.dtype == torch.bfloat16 and wpk.numel() == ct * 2 * cp * 9 * co
    assert bpk.dtype == torch.float32 and bpk.numel() == ct * co and torch.equal(bpk[:cout], b) and not bool(bpk[cout:].any())
    hi, lo = G.split_bf16(w)
    got = G.unpack_conv_x3(wpk, cout, cin, layer)
    assert got.dtype == torch.float32 and torch.equal(got, hi.float() + lo.float())
    # the layout itself: [co_tile][cell block = 2 (ci / 8) + part][tap][co][8]
    v = wpk.reshape(ct, 2 * cp // 8, 9, co, 8)
    o, i = min(cout - 1, 70), min(cin - 1, 19)
    assert torch.equal(v[o // co, 2 * (i // 8), 5, o % co, i % 8], hi[o, i, 1, 2])
    assert torch.equal(v[o // co, 2 * (i // 8) + 1, 5, o % co, i % 8], lo[o, i, 1, 2])
    assert int((wpk != 0).sum()) == int((hi != 0).sum()) + int((lo != 0).sum())  # pad channels are zero


@pytest.mark.parametrize("cin,cout,layer,co", [(128, 256, G.GCX3_T2, 64), (256, 16, G.GCX3_T2_C16, 16),
                                               (40, 72, G.GCX3_T2, 64), (20, 8, G.GCX3_T2_C16, 16)])
def test_pack_convt_x3_round_trip(cin, cout, layer, co):
    g = torch.Generator().manual_seed(cout + cin)
    w = torch.randn((cin, cout, 3, 3), generator=g)
    wpk, bpk = G.pack_convt_x3(w, None, layer)
    assert G._layout_of(G._X3, layer) == (co, 16, True)
    ct, cp = -(-cout // co), -(-cin // 16) * 16
    assert wpk.dtype == torch.bfloat16 and wpk.numel() == ct * co * 2 * cp * 9
    assert not bool(bpk.any())
    hi, lo = G.split_bf16(w)
    assert torch.equal(G.unpack_convt_x3(wpk, cin, cout, layer), hi.float() + lo.float())
    assert int((wpk != 0).sum()) == int((hi != 0).sum()) + int((lo != 0).sum())
    # [phase][co_tile][cell block][ntap][co][8], the phases (2 py + px) and their taps in the kernel's order
    for o, i, ky, kx in ((5, 11, 1, 2), (5, 11, 1, 1), (cout - 1, cin - 1, 2, 0), (cout - 1, cin - 1, 2, 2)):
        py, px = int(ky != 1), int(kx != 1)
        phase, ntap, t = 2 * py + px, (2 if py else 1) * (2 if px else 1), (ky // 2) * (2 if px else 1) + kx // 2
        base = sum((1, 2, 2, 4)[:phase]) * ct * 2 * cp * co
        for part, src in ((0, hi), (1, lo)):
            at = base + ((((o // co) * (2 * cp // 8) + 2 * (i // 8) + part) * ntap + t) * co + o % co) * 8 + i % 8
            assert float(wpk[at]) == float(src[i, o, ky, kx])


# ------------------------------------------------------------------ refusals before any device call
def _gconv_x3(**over):
    a = dict(layer=G.GCX3_S2, x0=P, c0=16, x1=None, c1=0, wpk=P, bias=P, ys=P, y32=None, h=None, zb=None, rhs=None,
             qxb=None, hout32=None, houts=None, B=1, Hi=16, Wi=16, cout=256, ohs=8, ows=8, act=1, in_div=1.0, hc=0,
             stream=None)
    a.update(over)
    lib = _lib.get()
    rc = lib.nlspn_gconv_x3(*a.values())
    return rc, lib.nlspn_last_error().decode()


GRU1 = dict(layer=G.GCX3_GRU1, c0=128, x1=P, c1=128, ys=None, h=P, zb=P, rhs=P, qxb=P, cout=384, hc=128, act=0)
GRU2 = dict(layer=G.GCX3_GRU2, c0=128, ys=None, h=P, zb=P, qxb=P, hout32=P, houts=P, cout=128, hc=128, act=0)


@pytest.mark.parametrize("over,code,msg", [
    (dict(x0=None), _lib.EINVAL, "null"),
    (dict(wpk=None), _lib.EINVAL, "null"),
    (dict(bias=None), _lib.EINVAL, "null"),
    (dict(c1=16), _lib.EINVAL, "bad shape"),                              # c1 > 0 without x1
    (dict(layer=G.GC_S2), _lib.EINVAL, "not a split-bf16 preset"),        # an f32 preset
    (dict(layer=G.GC16_S2), _lib.EINVAL, "not a split-bf16 preset"),      # an f16 preset
    (dict(layer=99), _lib.EINVAL, "not a split-bf16 preset"),
    (dict(ys=None), _lib.EINVAL, "both outputs null"),
    (dict(layer=G.GCX3_T2, ys=None), _lib.EINVAL, "both outputs null"),
    (dict(layer=G.GCX3_S2_SMALL, c0=1, cout=16, y32=P), _lib.EINVAL, "not supported"),   # the VALU kernel: c8x2 only
    (dict(layer=G.GCX3_S2_SMALL, c0=32, cout=16), _lib.EINVAL, "VALU kernel's range"),
    (dict(GRU1, ys=P), _lib.EINVAL, "not supported"),                     # a GRU launch has no ys / y32
    (dict(GRU2, y32=P), _lib.EINVAL, "not supported"),
    (dict(GRU1, rhs=None), _lib.EINVAL, "GRU launch needs"),
    (dict(GRU1, h=None), _lib.EINVAL, "GRU launch needs"),
    (dict(GRU2, houts=None), _lib.EINVAL, "GRU launch needs"),            # both h' outputs are required
    (dict(GRU2, hout32=None), _lib.EINVAL, "GRU launch needs"),
    (dict(GRU1, hc=96, c0=96, cout=288), _lib.EINVAL, "GRU launch needs"),  # hc no multiple of the co tile
    (dict(c0=8, x1=P, c1=16), _lib.EINVAL, "straddle"),                   # c0 no multiple of the 16-channel chunk
    (dict(c0=40, x1=P, c1=24), _lib.EINVAL, "straddle"),
    (dict(in_div=10.0), _lib.EINVAL, "in_div"),
    (dict(ohs=9), _lib.EINVAL, "stored size"),
    (dict(act=3), _lib.EINVAL, "activation"),
])
def test_gconv_x3_validates_before_any_device_call(over, code, msg):
    rc, text = _gconv_x3(**over)
    assert rc == code and msg in text and text.startswith("gconv_x3"), (rc, text)


def test_a_good_split_passes_the_chunk_rule_and_the_layout_query():
    rc, text = _gconv_x3(c0=16, x1=P, c1=24, ohs=9)   # c0 = 16 is a whole chunk: the next refusal is another one
    assert rc == _lib.EINVAL and "stored size" in text and "straddle" not in text, (rc, text)
    lib = _lib.get()
    assert G._layout_of(G._X3, G.GCX3_S2_SMALL) == (0, 1, False)
    assert lib.nlspn_gconv_x3_pack_layout(G.GC16_S2, None, None, None) == _lib.EINVAL
    assert "not a split-bf16 preset" in lib.nlspn_last_error().decode()
    # the other families' queries do not know the split presets: the packs cannot be mixed up
    assert lib.nlspn_gconv_pack_layout(G.GCX3_S2, None, None, None) == _lib.EINVAL
    assert lib.nlspn_gconv16_pack_layout(G.GCX3_S2, None, None, None) == _lib.EINVAL
    assert lib.nlspn_abi_version() == 3


def test_x3_unit_compiles_without_scratch(tmp_path):
    """The compiler's kernel-resource-usage remarks of the unit (the code object's metadata values)."""
    sys.path.insert(0, CSRC)
    import resource_usage as RU
    path = os.path.join(RU.BUILD_DIR, "nlspn_kern_gconv_x3.ru.txt")
    if os.path.exists(path):
        rows = RU.parse(open(path).read())
    else:
        out = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
                              "-ffp-contract=off", "-Rpass-analysis=kernel-resource-usage", "-c", "-o",
                              str(tmp_path / "gx3.o"), os.path.join(CSRC, "nlspn_kern_gconv_x3.hip")],
                             capture_output=True, text=True, cwd=CSRC)
        assert out.returncode == 0, out.stderr[-2000:]
        rows = RU.parse(out.stderr)
    # the five MFMA presets and the VALU kernel
    assert len(rows) == 6 and all("gconvx3_kernel" in n or "gsmallx3_kernel" in n for n in rows), sorted(rows)
    assert sum("gsmallx3_kernel" in n for n in rows) == 1
    bad = {n: (r.get("ScratchSize"), r.get("VGPRs Spill")) for n, r in rows.items()
           if r.get("ScratchSize", 0) != 0 or r.get("VGPRs Spill", 0) != 0}
    assert not bad, bad


# ------------------------------------------------------------------ the switch
def make_model(H=32, W=32, T=3, hc=128, device="cpu", seed=5):
    """The seeded hc-128 GRU-mode model of the GPU tests (weights and biases of a trained scale)."""
    args = types.SimpleNamespace(prop_kernel=3, affinity="TGASS", affinity_gamma=0.5, prop_time=T,
                                 preserve_input=True, always_clip=False, conf_prop=True, offset=True,
                                 network="resnet34", from_scratch=True, zero_init_aff=False, use_GRU=True,
                                 use_S2D=False, GRU_hidden_dim=hc, GRU_input_dim=hc, lr=1e-3, max_depth=10.0,
                                 patch_height=H, patch_width=W, model_name="NLSPN")
    torch.manual_seed(seed)
    m = NLSPNModel(args).to(device).eval()
    with torch.no_grad():
        for mod in (m.encode_dep, m.encode_aff, m.GRU, m.decode_aff):
            for p in mod.parameters():
                p.add_(0.02 * torch.randn_like(p))
    return m


def test_gru_precision_accepts_bf16x3_and_refuses_the_rest():
    m = make_model()
    assert m.gru_precision == "fp32"
    m.gru_precision = "bf16x3"
    assert m.gru_precision == "bf16x3"
    for bad in ("bf16", "half", 16, None, "FP16", "BF16X3", "bf16x2"):
        with pytest.raises(ValueError, match="gru_precision"):
            m.gru_precision = bad
    assert m.gru_precision == "bf16x3"       # a refused value changes nothing
    assert "gru_precision" not in m.state_dict() and "_gru_precision" not in m.state_dict()
    # on the CPU the HIP path never runs, so neither does its split variant: the mode is ignored
    assert not m._gru_x3(torch.zeros(1, 1, 8, 8)) and not m._gru_fp16(torch.zeros(1, 1, 8, 8))
    x, aff = torch.rand(1, 1, 32, 32), torch.rand(1, 9, 32, 32)
    with torch.no_grad():
        a = m._gru_update(None, aff, x, 2)
        m.gru_precision = "fp32"
        b = m._gru_update(None, aff, x, 2)
    assert isinstance(a, torch.Tensor) and torch.equal(a, b)   # the modules' plain state, not the (h, split) pair
    assert m._gru_convs.stats["fwd_x3"] == 0 and m._gru_convs.stats["fwd"] == 0 and m._gru_convs.stats["fwd16"] == 0


# ------------------------------------------------------------------ the emulation yardstick
def carry32(t):
    """What a kernel's epilogue holds: the f32 value."""
    return t.float().double()


def carry64(t):
    return t


def _split64(t):
    """split_bf16 of the value a layer end carries (f32: the contract's split; float64: the yardstick's)."""
    hi = t.to(torch.bfloat16).to(t.dtype)
    lo = (t - hi).to(torch.bfloat16).to(t.dtype)
    return hi.double(), lo.double()


def conv3(fn, x, w, **kw):
    """The three split products of a convolution, in float64: x the carried activation, w f32 weights."""
    xh, xl = _split64(x)
    wh, wl = _split64(w.detach().cpu().float())
    return fn(xh, wh, None, **kw) + fn(xl, wh, None, **kw) + fn(xh, wl, None, **kw)


def _b(conv):
    return conv.bias.detach().cpu().double()[None, :, None, None]


def _conv_of(s):
    return s[0] if isinstance(s, torch.nn.Sequential) else s


def emu_encoder(seqs, x, last, carry):
    """A stride-2 encoder chain: the VALU first layer on unsplit f32 operands, the others split.
    x: the f32 input (after in_div).  Returns the carried output of the last layer."""
    for i, s in enumerate(seqs):
        c = _conv_of(s)
        if i == 0:
            y = F.conv2d(x.double(), c.weight.detach().cpu().double(), None, stride=2, padding=1)
        else:
            y = conv3(F.conv2d, x, c.weight, stride=2, padding=1)
        y = y + _b(c)
        x = carry(torch.relu(y) if i < len(seqs) - 1 else last(y))
    return x


def emu_gru(g, h, x, carry):
    """One ConvGRU step: h the carried f32 state, x the carried input; z and qx carried, r*h formed
    from the carried r and h and carried, then split."""
    hc = g.convz.out_channels
    hx = torch.cat([h, x], 1)
    z = carry(torch.sigmoid(conv3(F.conv2d, hx, g.convz.weight, padding=1) + _b(g.convz)))
    rh = carry(torch.sigmoid(conv3(F.conv2d, hx, g.convr.weight, padding=1) + _b(g.convr)) * h)
    qx = carry(conv3(F.conv2d, x, g.convq.weight[:, hc:], padding=1) + _b(g.convq))
    q = torch.tanh(conv3(F.conv2d, rh, g.convq.weight[:, :hc], padding=1) + qx)
    return carry((1 - z) * h + z * q)


def emu_decoder(seqs, x, crop, carry):
    """decode_aff: split transposed layers, the last one a plain convolution of unsplit operands
    on the carried output of the layer before it; cropped."""
    kw = dict(stride=2, padding=1, output_padding=1)
    for i, s in enumerate(seqs):
        c = _conv_of(s)
        if i == len(seqs) - 1:
            x = F.conv_transpose2d(x, c.weight.detach().cpu().double(), None, **kw) + _b(c)
        else:
            x = carry(torch.relu(conv3(F.conv_transpose2d, x, c.weight, **kw) + _b(c)))
    return carry(x[:, :, :crop[0], :crop[1]])


def emu_chains(m, new_pred, aff, carry, H, W):
    """Every chain of one GRU update on CPU copies of m's weights, each from the emulation's own
    inputs: encode_dep, encode_aff, one ConvGRU step and decode_aff."""
    x = (new_pred.cpu().float() / torch.tensor(m.args.max_depth, dtype=torch.float32))  # the division in f32, as the loads
    dep = emu_encoder(list(m.encode_dep), x, torch.relu, carry)
    h = emu_encoder(list(m.encode_aff)[:3], aff.cpu().float(), torch.tanh, carry)
    hn = emu_gru(m.GRU, h, dep, carry)
    raw = emu_decoder(list(m.decode_aff), hn, (H, W), carry)
    return {"encode_dep": dep, "encode_aff": h, "gru": hn, "decode_aff": raw}


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def test_emulation_does_not_depend_on_where_a_split_lands():
    H, W = 50, 70
    m = make_model(H, W)
    g = torch.Generator().manual_seed(3)
    new_pred = torch.rand((1, 1, H, W), generator=g) * 10
    aff = torch.rand((1, 9, H, W), generator=g) - 0.3
    with torch.no_grad():
        a, b = emu_chains(m, new_pred, aff, carry64, H, W), emu_chains(m, new_pred, aff, carry32, H, W)
    got = {k: rel_l2(b[k], a[k]) for k in a}
    print("emulation, f32-carried against float64-carried:", got)
    assert all(float(v.abs().max()) > 0 for v in a.values())
    assert all(v <= 2.5e-6 for v in got.values()), got
    # and the split terms matter: without w_lo x_hi the chains move by far more than the bar
    x = torch.randn((1, 16, 9, 9), generator=g)
    w = torch.randn((8, 16, 3, 3), generator=g)
    full = F.conv2d(x.double(), w.double(), None, padding=1)
    assert rel_l2(conv3(F.conv2d, x, w, padding=1), full) <= 2.0 ** -15
    xh, _ = _split64(x)
    wh, _ = _split64(w)
    assert rel_l2(F.conv2d(xh, wh, None, padding=1), full) > 2.0 ** -11
