"""CPU: the f16-operand GRU-mode convolutions (csrc/nlspn_gconv16.h) off the device: the c8
layout helpers, the weight packers (layout and a single round-to-nearest-even), every refusal
of nlspn_gconv16 before a device call, the unit's resource remarks (no scratch) and the
model's gru_precision switch."""
import ctypes
import os
import subprocess
import sys
import types

import pytest
import torch

from nlspn_eccv20_amd import NLSPNModel, _lib
from nlspn_eccv20_amd import gru as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nlspn_eccv20_amd", "csrc")
P = ctypes.c_void_p(64)  # never dereferenced: validation fails first


@pytest.mark.parametrize("C", [1, 8, 9, 20, 128])
def test_c8_round_trip(C):
    g = torch.Generator().manual_seed(C)
    x = torch.randn((2, C, 5, 7), generator=g) * 3
    y = G.to_c8(x)
    nb = (C + 7) // 8
    assert y.shape == (2, nb, 5, 7, 8) and y.dtype == torch.float16 and y.is_contiguous()
    assert torch.equal(G.from_c8(y, C), x.half())
    # the cell of pixel (3, 4), block k holds channels 8k .. 8k + 7; pad channels are zero
    flat = y.permute(0, 1, 4, 2, 3).reshape(2, nb * 8, 5, 7)
    assert torch.equal(flat[:, :C], x.half()) and not bool(flat[:, C:].any())
    assert torch.equal(y[1, nb - 1, 3, 4, 0], x.half()[1, 8 * (nb - 1), 3, 4])


@pytest.mark.parametrize("cout,cin,layer", [(256, 16, G.GC16_S2), (128, 256, G.GC16_S2), (72, 20, G.GC16_S2),
                                            (384, 256, G.GC16_GRU1), (128, 128, G.GC16_GRU2), (64, 40, G.GC16_GRU2)])
def test_pack_conv16_inverts_to_the_rounded_weight(cout, cin, layer):
    g = torch.Generator().manual_seed(cout + cin)
    w = torch.randn((cout, cin, 3, 3), generator=g)
    b = torch.randn(cout, generator=g)
    wpk, bpk = G.pack_conv16(w, b, layer)
    co, cc, tr = G._layout16(layer)
    assert (co, cc, tr) == (64, 32, False)
    ct, cp = -(-cout // co), -(-cin // cc) * cc
    assert wpk.dtype == torch.float16 and wpk.numel() == ct * cp * 9 * co
    assert bpk.dtype == torch.float32 and bpk.numel() == ct * co and torch.equal(bpk[:cout], b) and not bool(bpk[cout:].any())
    assert torch.equal(G.unpack_conv16(wpk, cout, cin, layer), w.half())  # bit for bit: one RNE rounding
    # the layout itself: [co_tile][ci / 8][tap][co][8]
    v = wpk.reshape(ct, cp // 8, 9, co, 8)
    o, i = min(cout - 1, 70), min(cin - 1, 19)
    assert torch.equal(v[o // co, i // 8, 5, o % co, i % 8], w.half()[o, i, 1, 2])
    assert int((wpk != 0).sum()) == int((w.half() != 0).sum())  # padding is zero


@pytest.mark.parametrize("cin,cout,layer,co", [(128, 256, G.GC16_T2, 64), (256, 16, G.GC16_T2_C16, 16),
                                               (40, 72, G.GC16_T2, 64), (20, 8, G.GC16_T2_C16, 16)])
def test_pack_convt16_inverts_to_the_rounded_weight(cin, cout, layer, co):
    g = torch.Generator().manual_seed(cout + cin)
    w = torch.randn((cin, cout, 3, 3), generator=g)
    wpk, bpk = G.pack_convt16(w, None, layer)
    assert G._layout16(layer) == (co, 32, True)
    assert wpk.dtype == torch.float16 and wpk.numel() == -(-cout // co) * co * -(-cin // 32) * 32 * 9
    assert not bool(bpk.any())
    assert torch.equal(G.unpack_convt16(wpk, cin, cout, layer), w.half())
    assert int((wpk != 0).sum()) == int((w.half() != 0).sum())
    # the layout itself: [phase][co_tile][ci / 8][ntap][co][8], the phases (2 py + px) and their taps
    # in the kernel's order (py = 0 reads ky = 1, py = 1 reads ky = 0, 2; likewise kx); one interior
    # element and one of the last (partial, where the counts leave one) tile, by an index computed here
    ct, cp = -(-cout // co), -(-cin // 32) * 32
    for o, i, ky, kx in ((5, 11, 1, 2), (5, 11, 1, 1), (cout - 1, cin - 1, 2, 0), (cout - 1, cin - 1, 2, 2)):
        py, px = int(ky != 1), int(kx != 1)
        phase, ntap, t = 2 * py + px, (2 if py else 1) * (2 if px else 1), (ky // 2) * (2 if px else 1) + kx // 2
        base = sum((1, 2, 2, 4)[:phase]) * ct * cp * co
        at = base + ((((o // co) * (cp // 8) + i // 8) * ntap + t) * co + o % co) * 8 + i % 8
        assert float(wpk[at]) == float(w.half()[i, o, ky, kx])


def test_pack_rounds_to_nearest_even_once():
    # 1 + 2^-11 is a tie between 1 and 1 + 2^-10 (even: 1); 1 + 3 * 2^-11 a tie that rounds up to 1 + 2^-9
    w = torch.zeros((64, 32, 3, 3))
    w[0, 0, 0, 0], w[1, 0, 0, 0], w[2, 0, 0, 0] = 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 70000.0
    got = G.unpack_conv16(G.pack_conv16(w, None, G.GC16_S2)[0], 64, 32, G.GC16_S2)
    assert float(got[0, 0, 0, 0]) == 1.0 and float(got[1, 0, 0, 0]) == 1 + 2.0 ** -9
    assert torch.isinf(got[2, 0, 0, 0])  # a plain conversion: overflow gives inf, no clamping


def _gconv16(**over):
    a = dict(layer=G.GC16_S2, x0=P, c0=16, x1=None, c1=0, wpk=P, bias=P, y16=P, y32=None, h=None, zb=None, rh16=None,
             qxb=None, hout32=None, hout16=None, B=1, Hi=16, Wi=16, cout=256, ohs=8, ows=8, act=1, in_div=1.0, hc=0,
             stream=None)
    a.update(over)
    lib = _lib.get()
    rc = lib.nlspn_gconv16(*a.values())
    return rc, lib.nlspn_last_error().decode()


GRU1 = dict(layer=G.GC16_GRU1, c0=128, x1=P, c1=128, y16=None, h=P, zb=P, rh16=P, qxb=P, cout=384, hc=128, act=0)
GRU2 = dict(layer=G.GC16_GRU2, c0=128, y16=None, h=P, zb=P, qxb=P, hout32=P, hout16=P, cout=128, hc=128, act=0)


@pytest.mark.parametrize("over,code,msg", [
    (dict(x0=None), _lib.EINVAL, "null"),
    (dict(wpk=None), _lib.EINVAL, "null"),
    (dict(bias=None), _lib.EINVAL, "null"),
    (dict(c1=16), _lib.EINVAL, "bad shape"),                              # c1 > 0 without x1
    (dict(layer=G.GC_S2), _lib.EINVAL, "not an f16 preset"),              # an f32 preset
    (dict(layer=G.GC_DG_S1), _lib.EINVAL, "not an f16 preset"),
    (dict(layer=99), _lib.EINVAL, "not an f16 preset"),
    (dict(y16=None), _lib.EINVAL, "both outputs null"),
    (dict(layer=G.GC16_T2, y16=None), _lib.EINVAL, "both outputs null"),
    (dict(layer=G.GC16_S2_SMALL, c0=1, cout=16, y32=P), _lib.EINVAL, "not supported"),   # the VALU kernel: c8 only
    (dict(layer=G.GC16_S2_SMALL, c0=1, cout=16, y16=None, y32=P), _lib.EINVAL, "not supported"),
    (dict(layer=G.GC16_S2_SMALL, c0=32, cout=16), _lib.EINVAL, "VALU kernel's range"),
    (dict(GRU1, y16=P), _lib.EINVAL, "not supported"),                    # a GRU launch has no y16 / y32
    (dict(GRU2, y32=P), _lib.EINVAL, "not supported"),
    (dict(GRU1, rh16=None), _lib.EINVAL, "GRU launch needs"),
    (dict(GRU1, h=None), _lib.EINVAL, "GRU launch needs"),
    (dict(GRU2, hout16=None), _lib.EINVAL, "GRU launch needs"),           # both h' outputs are required
    (dict(GRU2, hout32=None), _lib.EINVAL, "GRU launch needs"),
    (dict(GRU1, hc=96, c0=96, cout=288), _lib.EINVAL, "GRU launch needs"),
    (dict(c0=16, x1=P, c1=16), _lib.EINVAL, "straddle"),                  # c0 no multiple of the 32-channel chunk
    (dict(c0=40, x1=P, c1=24), _lib.EINVAL, "straddle"),
    (dict(in_div=10.0), _lib.EINVAL, "in_div"),
    (dict(ohs=9), _lib.EINVAL, "stored size"),
    (dict(act=3), _lib.EINVAL, "activation"),
])
def test_gconv16_validates_before_any_device_call(over, code, msg):
    rc, text = _gconv16(**over)
    assert rc == code and msg in text, (rc, text)


def test_a_good_split_passes_the_chunk_rule():
    # c0 = 32 passes the straddle rule: the next refusal is another one
    rc, text = _gconv16(c0=32, x1=P, c1=16, ohs=9)
    assert rc == _lib.EINVAL and "stored size" in text and "straddle" not in text, (rc, text)


def test_pack_layout_query():
    lib = _lib.get()
    assert G._layout16(G.GC16_S2_SMALL) == (0, 1, False)
    assert lib.nlspn_gconv16_pack_layout(G.GC_S2, None, None, None) == _lib.EINVAL
    assert "not an f16 preset" in lib.nlspn_last_error().decode()
    # the f32 query does not know the f16 presets either: the two families' packs cannot be mixed up
    assert lib.nlspn_gconv_pack_layout(G.GC16_S2, None, None, None) == _lib.EINVAL


def test_f16_unit_compiles_without_scratch(tmp_path):
    sys.path.insert(0, CSRC)
    import resource_usage as RU
    path = os.path.join(RU.BUILD_DIR, "nlspn_kern_gconv16.ru.txt")
    if os.path.exists(path):
        rows = RU.parse(open(path).read())
    else:
        out = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
                              "-ffp-contract=off", "-Rpass-analysis=kernel-resource-usage", "-c", "-o",
                              str(tmp_path / "g16.o"), os.path.join(CSRC, "nlspn_kern_gconv16.hip")],
                             capture_output=True, text=True, cwd=CSRC)
        assert out.returncode == 0, out.stderr[-2000:]
        rows = RU.parse(out.stderr)
    # the five MFMA presets and the VALU kernel
    assert len(rows) == 6 and all("gconv16_kernel" in n or "gsmall16_kernel" in n for n in rows), sorted(rows)
    assert sum("gsmall16_kernel" in n for n in rows) == 1
    bad = {n: (r.get("ScratchSize"), r.get("VGPRs Spill")) for n, r in rows.items()
           if r.get("ScratchSize", 0) != 0 or r.get("VGPRs Spill", 0) != 0}
    assert not bad, bad


def _model():
    args = types.SimpleNamespace(prop_kernel=3, affinity="TGASS", affinity_gamma=0.5, prop_time=3,
                                 preserve_input=True, always_clip=False, conf_prop=True, offset=True,
                                 network="resnet34", from_scratch=True, zero_init_aff=False, use_GRU=True,
                                 use_S2D=False, GRU_hidden_dim=128, GRU_input_dim=128, lr=1e-3, max_depth=10.0,
                                 patch_height=32, patch_width=32, model_name="NLSPN")
    return NLSPNModel(args)


def test_gru_precision_default_and_value_error():
    m = _model()
    assert m.gru_precision == "fp32"
    m.gru_precision = "fp16"
    assert m.gru_precision == "fp16"
    for bad in ("bf16", "half", 16, None, "FP16"):
        with pytest.raises(ValueError, match="gru_precision"):
            m.gru_precision = bad
    assert m.gru_precision == "fp16"       # a refused value changes nothing
    assert "gru_precision" not in m.state_dict() and "_gru_precision" not in m.state_dict()
    assert m._gru_convs.stats["fwd16"] == 0
    # on the CPU the HIP path never runs, so neither does its f16 variant
    assert not m._gru_fp16(torch.zeros(1, 1, 8, 8))
