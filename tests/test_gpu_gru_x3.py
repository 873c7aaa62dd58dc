"""GPU: the GRU-mode section on the bf16 matrix cores with split operands
(NLSPNModel.gru_precision = "bf16x3", nlspn_eccv20_amd/gru.py, csrc/nlspn_gconv_x3.h) on the
hc-128 model, 50x70, B = 1, T = 3: every chain against the float64 emulation of the contract
(tests/test_gconv_x3_cpu.py: the three split products, split_bf16 at the contract's points,
activations carried in f32), the section against the "fp32" native section and against the
"fp16" mode's distance from it, and the switch's behaviour.

Chains, relative L2 against the emulation; bar 1e-5, the project's order-only bar for the native
path against the f32 modules (tests/test_gpu_gru.py); recorded as gru_x3/chain/*.
Section against the "fp32" native section (pred, pred_inter, aff): finite, different (> 0),
RMSE <= 1e-4 and largest difference <= 1e-3 (the fixture bars the f32 path is held to), and RMSE
at most 1/8 of the "fp16" mode's against the same section on the same inputs (expected about
1/64: operand error 2^-17 against 2^-11; the factor 8 leaves room for the f32 accumulation floor
both modes share); recorded as gru_x3/model/*.

Measured on an MI355X:
    chain        relative L2 against the emulation        (bar 1e-5)
    encode_dep   2.6e-6
    encode_aff   3.1e-6
    gru          1.3e-6
    decode_aff   1.6e-7
    output       RMSE bf16x3 (fp16)      largest |difference| bf16x3 (fp16)     RMSE ratio
    pred         2.4e-7 (8.8e-6)         3.8e-6 (1.1e-4)                         1/37
    pred_inter   1.8e-7 (6.6e-6)         3.8e-6 (1.1e-4)                         1/36
    aff          2.4e-8 (1.3e-6)         2.4e-7 (1.2e-5)                         1/55
"""
import numpy as np
import pytest
import torch

from nlspn_eccv20_amd import SectionGraph
from nlspn_eccv20_amd.gru import GruConvs, from_c8x2, split_bf16
from test_gconv_x3_cpu import carry32, emu_decoder, emu_encoder, emu_gru, make_model, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = 3
H, W = 50, 70
BAR_CHAIN = 1e-5
BAR_RMSE, BAR_MAX = 1e-4, 1e-3


def _model(hc=128):
    return make_model(H, W, T, hc, DEV)


def _inputs(B=1, seed=9):
    g = torch.Generator(device=DEV).manual_seed(seed)
    pred_init = torch.rand((B, 1, H, W), device=DEV, generator=g) * 10
    dep = pred_init * (torch.rand((B, 1, H, W), device=DEV, generator=g) < 0.02)
    off_aff = torch.randn((B, 24, H, W), device=DEV, generator=g)
    conf = torch.rand((B, 1, H, W), device=DEV, generator=g)
    return pred_init, off_aff, conf, dep


def _split_sum(t):
    hi, lo = split_bf16(t.float())
    return hi.double() + lo.double()


def test_chains_against_the_emulation(record_metric):
    m = _model()
    m.gru_precision = "bf16x3"
    gc = GruConvs()
    g = torch.Generator(device=DEV).manual_seed(3)
    new_pred = torch.rand((1, 1, H, W), device=DEV, generator=g) * 10
    aff = torch.rand((1, 9, H, W), device=DEV, generator=g) - 0.3
    hc = 128
    with torch.no_grad():
        P = gc.pack_x3(m)
        ds = gc.encode_dep_x3(P, new_pred, m.args.max_depth)
        h32, hs = gc.encode_aff_x3(P, aff)
        hn32, hns = gc.gru_x3(P, (h32, hs), ds)
        raw = gc.decode_aff_x3(P, (hn32, hns), (H, W))   # no gamma: the raw taps
    torch.cuda.synchronize()
    assert gc.stats["fwd_x3"] == 3 + 3 + 2 + 2 and gc.stats["fwd"] == 1 and gc.stats["fwd16"] == 0
    got = {}
    with torch.no_grad():
        x = new_pred.cpu() / torch.tensor(m.args.max_depth, dtype=torch.float32)   # the division in f32, as the loads
        ref = emu_encoder(list(m.encode_dep), x, torch.relu, carry32)
        got["encode_dep"] = rel_l2(from_c8x2(ds, hc), _split_sum(ref))
        ref = emu_encoder(list(m.encode_aff)[:3], aff.cpu(), torch.tanh, carry32)
        got["encode_aff"] = max(rel_l2(h32, ref), rel_l2(from_c8x2(hs, hc), _split_sum(ref)))
        # one ConvGRU step and decode_aff from the device's own state and input (their f32 values)
        ref = emu_gru(m.GRU, h32.cpu().double(), from_c8x2(ds, hc).cpu().double(), carry32)
        got["gru"] = max(rel_l2(hn32, ref), rel_l2(from_c8x2(hns, hc), _split_sum(ref)))
        ref = emu_decoder(list(m.decode_aff), hn32.cpu().double(), (H, W), carry32)
        assert raw.shape == ref.shape
        got["decode_aff"] = rel_l2(raw, ref)
    # the split copies are split_bf16 of the f32 states, bit for bit
    for s, f in ((hs, h32), (hns, hn32)):
        hi, lo = from_c8x2(s, hc, parts=True)
        whi, wlo = split_bf16(f)
        assert torch.equal(hi, whi) and torch.equal(lo, wlo)
    for k, v in got.items():
        record_metric(f"gru_x3/chain/{k}", v)
    assert all(v <= BAR_CHAIN for v in got.values()), got


def _outs(m, ins):
    with torch.no_grad():
        o = m.propagate_heads(*ins)
    return {"pred": o["pred"].clone(), "pred_inter": torch.stack(list(o["pred_inter"]), 0).clone(), "aff": o["aff"].clone()}


def test_section_against_fp32_native_and_fp16(record_metric):
    m = _model()
    ins = _inputs()
    outs = {}
    for prec in ("fp32", "fp16", "bf16x3"):
        m.gru_precision = prec
        outs[prec] = _outs(m, ins)
    assert m._gru_convs.stats["fwd_x3"] > 0 and m._gru_convs.stats["fwd16"] > 0
    fig = {}
    for prec in ("fp16", "bf16x3"):
        for k in ("pred", "pred_inter", "aff"):
            d = outs[prec][k].double() - outs["fp32"][k].double()
            fig[prec, k] = (float(d.pow(2).mean().sqrt()), float(d.abs().max()))
            record_metric(f"gru_x3/model/{k}/rmse/{prec}", fig[prec, k][0])
            record_metric(f"gru_x3/model/{k}/max/{prec}", fig[prec, k][1])
    for k in ("pred", "pred_inter", "aff"):
        rmse, mx = fig["bf16x3", k]
        assert torch.isfinite(outs["bf16x3"][k]).all()
        assert mx > 0.0, k                                   # the mode did change the arithmetic
        assert rmse <= BAR_RMSE and mx <= BAR_MAX, (k, rmse, mx)
        assert rmse <= fig["fp16", k][0] / 8, (k, rmse, fig["fp16", k][0])


# ------------------------------------------------------------------ the switch
def _section(m, ins):
    with torch.no_grad():
        o = m.propagate_heads(*ins)
    return [p.clone() for p in o["pred_inter"]] + [o["pred"].clone(), o["aff"].clone()]


def test_fp32_is_todays_path_bit_for_bit():
    ins = _inputs()
    want = _section(_model(), ins)
    m = _model()
    m.gru_precision = "bf16x3"
    m.gru_precision = "fp32"
    m._gru_convs.reset_stats()
    got = _section(m, ins)
    assert m._gru_convs.stats["fwd_x3"] == 0 and m._gru_convs.stats["fwd"] > 0
    assert all(torch.equal(a, b) for a, b in zip(got, want))


def test_x3_launch_counts_and_determinism():
    m = _model()
    m.gru_precision = "bf16x3"
    ins = _inputs()
    m._gru_convs.reset_stats()
    a = _section(m, ins)
    s = m._gru_convs.stats
    # per update: encode_dep 3, ConvGRU 2, decode_aff 2 split launches and the f32 last layer; encode_aff 3 once
    assert s["fwd_x3"] == (T - 1) * 7 + 3 and s["fwd"] == T - 1 and s["gru_fwd"] == T - 1 and s["fwd16"] == 0, s
    b = _section(m, ins)
    assert all(torch.equal(x, y) for x, y in zip(a, b))   # two runs are bit-equal
    assert all(t.dtype == torch.float32 for t in a)


def test_x3_is_ignored_under_gradients_and_without_native_gru():
    ins = _inputs()
    m = _model()
    m.native_gru_train = True
    with torch.enable_grad():
        m.gru_precision = "fp32"
        o = m.propagate_heads(*ins)
        want = [p.detach().clone() for p in o["pred_inter"]] + [o["pred"].detach().clone(), o["aff"].detach().clone()]
        m.gru_precision = "bf16x3"
        m._gru_convs.reset_stats()
        o = m.propagate_heads(*ins)
        got = [p.detach() for p in o["pred_inter"]] + [o["pred"].detach(), o["aff"].detach()]
    assert m._gru_convs.stats["fwd_x3"] == 0 and m._gru_convs.stats["fwd"] > 0
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    # native_gru = False: the modules run
    m.native_gru = False
    m._gru_convs.reset_stats()
    mod = _section(m, ins)
    assert m._gru_convs.stats["fwd_x3"] == 0 and m._gru_convs.stats["fwd"] == 0
    m.gru_precision = "fp32"
    # (two runs of the MIOpen modules are not bit-equal, so: within the project's 1e-4 bar, per element)
    for a, b in zip(mod, _section(m, ins)):
        assert float((a - b).abs().max()) <= 1e-4


def test_x3_is_ignored_on_the_hidden_8_fixture():
    """The reference's fixture has a ConvGRU of hidden width 8, which GruConvs.supported declines:
    the modules run, fwd_x3 == 0, fwd == 0, pred equals the "fp32" run's."""
    from test_backward_golden import _gru_off_model
    m, z = _gru_off_model("gru_off_tgass_preserve", DEV)
    m.eval()
    t = lambda k: torch.from_numpy(np.ascontiguousarray(z[k].astype(np.float32))).to(DEV)  # noqa: E731
    res = {}
    for prec in ("fp32", "bf16x3"):
        m.gru_precision = prec
        m._gru_convs.reset_stats()
        with torch.no_grad():
            o = m.propagate_heads(t("pred_init"), t("off_aff"), t("conf"), t("dep"))
        torch.cuda.synchronize()
        res[prec] = (o["pred"].clone(), dict(m._gru_convs.stats))
    assert not GruConvs.supported(m)
    assert res["bf16x3"][1]["fwd_x3"] == 0 and res["bf16x3"][1]["fwd"] == 0
    assert torch.equal(res["bf16x3"][0], res["fp32"][0])


def test_section_graph_replays_the_x3_section_bit_for_bit():
    m = _model()
    m.gru_precision = "bf16x3"
    pred_init, off_aff, conf, dep = _inputs()
    eager = _section(m, (pred_init, off_aff, conf, dep))
    sg = SectionGraph(m, pred_init, off_aff, conf, dep)
    for _ in range(2):
        o = sg.replay(pred_init, off_aff, conf, dep)
        torch.cuda.synchronize()
        got = list(o["pred_inter"]) + [o["pred"], o["aff"]]
        assert all(torch.equal(a, b) for a, b in zip(got, eager))
