"""GPU: the GRU-mode section on the f16 matrix cores (NLSPNModel.gru_precision = "fp16",
nlspn_eccv20_amd/gru.py, csrc/nlspn_gconv16.h): every chain against the torch modules'
arithmetic in float64 with .half() at exactly the contract's rounding points, the reference's
own GRU fixture, and the switch's behaviour.

Chains (relative L2 against float64 on the CPU; bar 4x the worst measured on an MI355X, rounded
up to one digit, on condition <= 1e-3; recorded per run as gru16/chain/*):
    chain        50x70 (B = 2)   136x312 (B = 1; 1/8 scale 17x39: uneven bands)   bar
    encode_dep   3.1e-5          4.1e-5                                            2e-4
    encode_aff   4.7e-5          6.0e-5                                            3e-4
    gru          2.0e-5          7.8e-6                                            8e-5
    decode_aff   1.0e-6          1.1e-6                                            5e-6
(What is left is device and reference rounding an activation to different f16 neighbours where
the f32 sum and the float64 one straddle a tie: 2^-11 on that element, carried through the layers
after it.  decode_aff's output passes no f16 rounding after its first layer.)
The contract's rounding points: weights to f16 once (not the VALU first layers', not the last
decoder layer's: those stay f32); every activation a later f16 convolution reads, once, where it
is produced; h carried in f32 with an f16 copy; r*h formed in f32, then rounded; z, qx f32.

The reference's fixture (tests/golden/gru_off_tgass_preserve.npz) has a ConvGRU of hidden width
8.  The HIP convolutions take widths that are multiples of 128 (GruConvs.supported), so on this
fixture _native_gru declines and, by the switch's own rule, "fp16" is ignored: the torch modules
run and fwd16 stays 0.  The test asserts exactly that, and the f32 figures beside it:
    output       RMSE fp16 = fp32    largest |difference| fp16 = fp32    bars (4x)
    pred         1.5e-7              1.9e-6                              6e-7, 8e-6
    pred_inter   1.5e-7              1.9e-6                              7e-7, 8e-6
    aff          4.8e-9              1.2e-7                              2e-8, 5e-7
How far the fp16 mode itself sits from f32 is therefore measured on a model the HIP path
accepts (hc = 128, T = 3), fp16 against fp32-native, per output (gru16/model/*; bars 4x):
    output       RMSE      largest |difference|    bars
    pred         8.8e-6    1.1e-4                  4e-5, 5e-4
    pred_inter   6.6e-6    1.1e-4                  3e-5, 5e-4
    aff          1.3e-6    1.2e-5                  6e-6, 5e-5
(depths up to 10, two GRU updates: the fp16 mode sits about 9e-6 RMSE from the f32 path, under
the 1e-4 bar by a factor of ten on this model; its largest single difference, 1.1e-4, is sixty
times the f32 path's own 1.9e-6.  The f32 path's distance from the modules is 2e-6 at most,
tests/test_gpu_gconv_fwd.py.)
"""
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from nlspn_eccv20_amd import NLSPNModel, SectionGraph
from nlspn_eccv20_amd.gru import GruConvs, from_c8

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = 3

BAR_CHAIN = {"encode_dep": 2e-4, "encode_aff": 3e-4, "gru": 8e-5, "decode_aff": 5e-6}
# the fixture: (RMSE, largest |difference|) per output, 4x measured
BAR_FIXTURE = {"pred": (6e-7, 8e-6), "pred_inter": (7e-7, 8e-6), "aff": (2e-8, 5e-7)}
# fp16 against fp32-native on the hc = 128 model: (RMSE, largest |difference|) of pred / pred_inter / aff
BAR_MODEL = {"pred": (4e-5, 5e-4), "pred_inter": (3e-5, 5e-4), "aff": (6e-6, 5e-5)}


def test_bars_meet_their_condition():
    assert all(b <= 1e-3 for b in BAR_CHAIN.values())


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


def _inputs(B, H, W, seed=9):
    g = torch.Generator(device=DEV).manual_seed(seed)
    pred_init = torch.rand((B, 1, H, W), device=DEV, generator=g) * 10
    dep = pred_init * (torch.rand((B, 1, H, W), device=DEV, generator=g) < 0.02)
    off_aff = torch.randn((B, 24, H, W), device=DEV, generator=g)
    conf = torch.rand((B, 1, H, W), device=DEV, generator=g)
    return pred_init, off_aff, conf, dep


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def _h64(t):
    """Rounded to f16 once, as float64."""
    return t.float().half().double()


def _wb(seq):
    c = seq[0] if isinstance(seq, torch.nn.Sequential) else seq
    return c.weight.detach().cpu(), c.bias.detach().cpu().double()


def _enc64(seqs, x, last):
    """A stride-2 encoder chain under the contract: the first (VALU) layer on f32 weights and the
    f32 input, the others on f16 weights and the f16-rounded activation of the layer before."""
    for i, s in enumerate(seqs):
        w, b = _wb(s)
        w = w.double() if i == 0 else _h64(w)
        x = F.conv2d(x if i == 0 else _h64(x), w, b, stride=2, padding=1)
        x = torch.relu(x) if i < len(seqs) - 1 else last(x)
    return x


@pytest.mark.parametrize("B,H,W", [(2, 50, 70), (1, 136, 312)])
def test_chains_against_float64_with_the_contracts_roundings(B, H, W, record_metric):
    m = _model(H, W)
    m.gru_precision = "fp16"
    gc = GruConvs()
    g = torch.Generator(device=DEV).manual_seed(3)
    new_pred = torch.rand((B, 1, H, W), device=DEV, generator=g) * 10
    aff = torch.rand((B, 9, H, W), device=DEV, generator=g) - 0.3
    hc = 128
    with torch.no_grad():
        P = gc.pack16(m)
        d16 = gc.encode_dep16(P, new_pred, m.args.max_depth)
        h32, h16 = gc.encode_aff16(P, aff)
        hn32, hn16 = gc.gru16(P, (h32, h16), d16)
        raw = gc.decode_aff16(P, (hn32, hn16), (H, W))   # no gamma: the raw taps
    torch.cuda.synchronize()
    assert gc.stats["fwd16"] == 3 + 3 + 2 + 2 and gc.stats["fwd"] == 1
    got = {}
    # encode_dep: the division in f32, as the kernel's loads
    x = (new_pred.cpu() / torch.tensor(m.args.max_depth, dtype=torch.float32)).double()
    ref = _enc64(list(m.encode_dep), x, torch.relu)
    got["encode_dep"] = _rel(from_c8(d16, hc), _h64(ref))
    # encode_aff: Tanh; the f32 state and its f16 copy
    ref = _enc64(list(m.encode_aff)[:3], aff.cpu().double(), torch.tanh)
    got["encode_aff"] = max(_rel(h32, ref), _rel(from_c8(h16, hc), _h64(ref)))
    assert torch.equal(from_c8(h16, hc), h32.half())
    # one ConvGRU step from the device's own state and input
    hh, xx = h32.cpu().double(), from_c8(d16, hc).cpu().double()
    hx = torch.cat([_h64(h32.cpu()), xx], 1)
    G = m.GRU
    cv = lambda t, c, sl=slice(None): F.conv2d(t, _h64(c.weight.detach().cpu()[:, sl]), None, padding=1)  # noqa: E731
    z = torch.sigmoid(cv(hx, G.convz) + G.convz.bias.detach().cpu().double()[None, :, None, None])
    r = torch.sigmoid(cv(hx, G.convr) + G.convr.bias.detach().cpu().double()[None, :, None, None])
    qx = cv(xx, G.convq, slice(hc, None)) + G.convq.bias.detach().cpu().double()[None, :, None, None]
    q = torch.tanh(cv(_h64(r * hh), G.convq, slice(0, hc)) + qx)
    ref = (1 - z) * hh + z * q
    got["gru"] = max(_rel(hn32, ref), _rel(from_c8(hn16, hc), _h64(ref)))
    assert torch.equal(from_c8(hn16, hc), hn32.half())
    # decode_aff from the device's own new state: two f16 layers, the last one f32
    x = from_c8(hn16, hc).cpu().double()
    seqs = list(m.decode_aff)
    for i, s in enumerate(seqs):
        w, b = _wb(s)
        last = i == len(seqs) - 1
        x = F.conv_transpose2d(x if last else _h64(x), w.double() if last else _h64(w), b, stride=2, padding=1,
                               output_padding=1)
        if not last:
            x = torch.relu(x)
        if i == 1:
            x = x.float().double()   # the last layer reads the f32 NCHW output
    ref = x[:, :, :H, :W]
    assert raw.shape == ref.shape
    got["decode_aff"] = _rel(raw, ref)
    for k, v in got.items():
        record_metric(f"gru16/chain/{k}/{B}x{H}x{W}", v)
    for k, v in got.items():
        assert v <= BAR_CHAIN[k], (k, got)


# ------------------------------------------------------------------ the reference's fixture
def _errs(o, z):
    inter = torch.stack(list(o["pred_inter"]), 0)
    out = {}
    for got, key in ((o["pred"], "pred"), (inter, "pred_inter"), (o["aff"], "aff")):
        g = got.detach().cpu().numpy().astype(np.float64)
        out[key] = (float(np.sqrt(np.mean((g - z[key]) ** 2))), float(np.abs(g - z[key]).max()))
    return out


def test_reference_fixture_under_the_fp16_switch(record_metric):
    """The fixture's hidden width (8) is none the HIP convolutions take, so the switch is ignored
    there (module docstring): the modules run, fwd16 == 0, the outputs equal the "fp32" ones."""
    from test_backward_golden import _gru_off_model
    m, z = _gru_off_model("gru_off_tgass_preserve", DEV)
    m.eval()
    t = lambda k: torch.from_numpy(np.ascontiguousarray(z[k].astype(np.float32))).to(DEV)  # noqa: E731
    res = {}
    for prec in ("fp32", "fp16"):
        m.gru_precision = prec
        m._gru_convs.reset_stats()
        with torch.no_grad():
            o = m.propagate_heads(t("pred_init"), t("off_aff"), t("conf"), t("dep"))
        torch.cuda.synchronize()
        res[prec] = (_errs(o, z), o, dict(m._gru_convs.stats))
    assert not GruConvs.supported(m)
    assert res["fp16"][2]["fwd16"] == 0 and res["fp16"][2]["fwd"] == 0
    for key, (rmse, mx) in res["fp16"][0].items():
        r32, m32 = res["fp32"][0][key]
        record_metric(f"gru16/fixture/{key}/rmse/fp16", rmse)
        record_metric(f"gru16/fixture/{key}/rmse/fp32", r32)
        record_metric(f"gru16/fixture/{key}/max/fp16", mx)
        record_metric(f"gru16/fixture/{key}/max/fp32", m32)
    for key, (rmse, mx) in res["fp16"][0].items():
        assert rmse <= BAR_FIXTURE[key][0] and mx <= BAR_FIXTURE[key][1], (key, rmse, mx)
    assert torch.equal(res["fp16"][1]["pred"], res["fp32"][1]["pred"])


def test_fp16_against_fp32_native_on_a_supported_model(record_metric):
    """What the f16 operands cost end to end where the mode does run (hc = 128, 50x70, T = 3)."""
    m = _model(50, 70)
    ins = _inputs(1, 50, 70)
    outs = {}
    for prec in ("fp32", "fp16"):
        m.gru_precision = prec
        with torch.no_grad():
            o = m.propagate_heads(*ins)
        outs[prec] = {"pred": o["pred"].clone(), "pred_inter": torch.stack(list(o["pred_inter"]), 0).clone(),
                      "aff": o["aff"].clone()}
    assert m._gru_convs.stats["fwd16"] > 0
    for k in ("pred", "pred_inter", "aff"):
        d = (outs["fp16"][k].double() - outs["fp32"][k].double())
        rmse, mx = float(d.pow(2).mean().sqrt()), float(d.abs().max())
        record_metric(f"gru16/model/{k}/rmse", rmse)
        record_metric(f"gru16/model/{k}/max", mx)
        assert torch.isfinite(outs["fp16"][k]).all()
        assert rmse <= BAR_MODEL[k][0] and mx <= BAR_MODEL[k][1], (k, rmse, mx)
        assert mx > 0.0   # the mode did change the arithmetic


# ------------------------------------------------------------------ the switch
def _section(m, ins):
    with torch.no_grad():
        o = m.propagate_heads(*ins)
    return [p.clone() for p in o["pred_inter"]] + [o["pred"].clone(), o["aff"].clone()]


def test_fp32_is_todays_path_bit_for_bit():
    ins = _inputs(1, 50, 70)
    untouched = _model(50, 70)
    want = _section(untouched, ins)
    m = _model(50, 70)
    m.gru_precision = "fp16"
    m.gru_precision = "fp32"
    m._gru_convs.reset_stats()
    got = _section(m, ins)
    assert m._gru_convs.stats["fwd16"] == 0 and m._gru_convs.stats["fwd"] > 0
    assert all(torch.equal(a, b) for a, b in zip(got, want))


def test_fp16_launch_counts_and_determinism():
    m = _model(50, 70)
    m.gru_precision = "fp16"
    ins = _inputs(1, 50, 70)
    m._gru_convs.reset_stats()
    a = _section(m, ins)
    s = m._gru_convs.stats
    # per update: encode_dep 3, ConvGRU 2, decode_aff 2 f16 launches and the f32 last layer; encode_aff 3 once
    assert s["fwd16"] == (T - 1) * 7 + 3 and s["fwd"] == T - 1 and s["gru_fwd"] == T - 1, s
    b = _section(m, ins)
    assert all(torch.equal(x, y) for x, y in zip(a, b))   # two runs are bit-equal
    assert all(t.dtype == torch.float32 for t in a)


def test_fp16_is_ignored_under_gradients_and_without_native_gru():
    ins = _inputs(1, 50, 70)
    m = _model(50, 70)
    m.native_gru_train = True
    with torch.enable_grad():
        m.gru_precision = "fp32"
        o = m.propagate_heads(*ins)
        want = [p.detach().clone() for p in o["pred_inter"]] + [o["pred"].detach().clone(), o["aff"].detach().clone()]
        m.gru_precision = "fp16"
        m._gru_convs.reset_stats()
        o = m.propagate_heads(*ins)
        got = [p.detach() for p in o["pred_inter"]] + [o["pred"].detach(), o["aff"].detach()]
    assert m._gru_convs.stats["fwd16"] == 0 and m._gru_convs.stats["fwd"] > 0
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    # native_gru = False: the modules run
    m.native_gru = False
    m._gru_convs.reset_stats()
    mod16 = _section(m, ins)
    assert m._gru_convs.stats["fwd16"] == 0 and m._gru_convs.stats["fwd"] == 0
    m.gru_precision = "fp32"
    # (two runs of the MIOpen modules are not bit-equal, so: within the project's 1e-4 bar, per element)
    for a, b in zip(mod16, _section(m, ins)):
        assert float((a - b).abs().max()) <= 1e-4


def test_section_graph_replays_the_fp16_section_bit_for_bit():
    m = _model(50, 70)
    m.gru_precision = "fp16"
    pred_init, off_aff, conf, dep = _inputs(1, 50, 70)
    eager = _section(m, (pred_init, off_aff, conf, dep))
    sg = SectionGraph(m, pred_init, off_aff, conf, dep)
    for _ in range(2):
        o = sg.replay(pred_init, off_aff, conf, dep)
        torch.cuda.synchronize()
        got = list(o["pred_inter"]) + [o["pred"], o["aff"]]
        assert all(torch.equal(a, b) for a, b in zip(got, eager))
