"""CPU: the backward entry points of the GRU-mode convolutions (include/nlspn_prop.h:
nlspn_gconv_dgrad, nlspn_gconv_wgrad, nlspn_gconv_gru_train, nlspn_gconv_gru_gates_backward)
refuse bad arguments before touching a device, the adjoint weight packers invert, and the
new translation unit compiles without scratch."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

from nlspn_eccv20_amd import _lib
from nlspn_eccv20_amd import gru as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nlspn_eccv20_amd", "csrc")
P = ctypes.c_void_p(64)  # never dereferenced: validation fails first


def _err(rc):
    return rc, _lib.get().nlspn_last_error().decode()


def _dgrad(**over):
    a = dict(layer=G.GC_DG_S1, g=P, cg=128, wpk=P, ysave=None, add0=None, add1=None, dx0=P, dx1=P, split=128, B=1,
             Hg=8, Wg=8, cout=256, Ho=8, Wo=8, act=0, scale=1.0, stream=None)
    a.update(over)
    return _err(_lib.get().nlspn_gconv_dgrad(*a.values()))


def _wgrad(**over):
    lib = _lib.get()
    a = dict(stride=1, s=P, Cs=128, l0=P, c0=128, l1=P, c1=128, dw=P, db=P, bias_from_large=0, scale=1.0, ws=P,
             ws_bytes=lib.nlspn_gconv_wgrad_workspace_bytes(1, 128, 256, 1, 8, 8, 8, 8), B=1, Hs=8, Ws=8, Hl=8, Wl=8,
             stream=None)
    a.update(over)
    return _err(lib.nlspn_gconv_wgrad(*a.values()))


def _gru_train(**over):
    a = dict(stage=1, x0=P, x1=P, c1=128, wpk=P, bias=P, h=P, zb=P, rhb=P, qxb=P, hout=None, rb=P, qb=None, B=1, H=8,
             W=8, hc=128, stream=None)
    a.update(over)
    return _err(_lib.get().nlspn_gconv_gru_train(*a.values()))


def _gates(**over):
    a = dict(stage=1, dhn=P, z=P, r=None, q=P, h=P, drh=None, duq=P, duzr=P, dh=None, act=0, B=1, hc=128, H=8, W=8,
             stream=None)
    a.update(over)
    return _err(_lib.get().nlspn_gconv_gru_gates_backward(*a.values()))


@pytest.mark.parametrize("fn,over,code,msg", [
    (_dgrad, dict(g=None), _lib.EINVAL, "null"),
    (_dgrad, dict(dx0=None), _lib.EINVAL, "null"),
    (_dgrad, dict(layer=G.GC_GRU2), _lib.EINVAL, "not a data-gradient preset"),
    (_dgrad, dict(split=300), _lib.EINVAL, "cout mismatch"),
    (_dgrad, dict(dx1=None), _lib.EINVAL, "cout mismatch"),        # split < cout without a second output
    (_dgrad, dict(act=1), _lib.EINVAL, "needs the saved output"),
    (_dgrad, dict(Ho=9), _lib.EINVAL, "does not belong"),
    (_dgrad, dict(layer=G.GC_DG_T2, Ho=14, Wo=16), _lib.EINVAL, "does not belong"),  # a crop of two rows
    (_wgrad, dict(s=None), _lib.EINVAL, "null"),
    (_wgrad, dict(ws=None), _lib.EINVAL, "null"),
    (_wgrad, dict(l1=None), _lib.EINVAL, "bad channels"),
    (_wgrad, dict(c0=120, c1=136), _lib.EINVAL, "straddle"),       # a two-source chunk over both sources
    (_wgrad, dict(ws_bytes=1024), _lib.EINVAL, "workspace too small"),
    (_wgrad, dict(stride=3), _lib.EINVAL, "stride"),
    (_wgrad, dict(Hl=9), _lib.EINVAL, "does not belong"),
    (_wgrad, dict(bias_from_large=1), _lib.EINVAL, "one source"),
    (_gru_train, dict(rb=None), _lib.EINVAL, "null r buffer"),
    (_gru_train, dict(stage=2, qb=None), _lib.EINVAL, "null q buffer"),
    (_gru_train, dict(hc=96), _lib.EINVAL, "not a multiple of the tile"),
    (_gru_train, dict(zb=None), _lib.EINVAL, "GRU launch needs"),
    (_gru_train, dict(stage=3), _lib.EINVAL, "stage"),
    (_gates, dict(q=None), _lib.EINVAL, "null pointer"),
    (_gates, dict(stage=2), _lib.EINVAL, "null pointer"),          # stage 2 needs r, d(rh) and dh
    (_gates, dict(hc=0), _lib.EINVAL, "bad shape"),
])
def test_backward_entry_points_validate_first(fn, over, code, msg):
    rc, text = fn(**over)
    assert rc == code and msg in text, (rc, text)


def test_forward_entry_refuses_dgrad_presets():
    lib = _lib.get()
    rc = lib.nlspn_gconv(G.GC_DG_S1, P, 128, None, 0, P, P, P, None, None, None, None, None, 1, 8, 8, 128, 8, 8, 0, 1.0,
                         0, None)
    assert rc == _lib.EINVAL and "nlspn_gconv_dgrad" in lib.nlspn_last_error().decode()


def _gconv(**over):
    a = dict(layer=G.GC_S2, x0=P, c0=16, x1=P, c1=16, wpk=P, bias=P, y=P, h=None, zb=None, rhb=None, qxb=None, hout=None,
             B=1, Hi=8, Wi=8, cout=64, ohs=4, ows=4, act=0, in_div=1.0, hc=0, stream=None)
    a.update(over)
    return _err(_lib.get().nlspn_gconv(*a.values()))


@pytest.mark.parametrize("over", [
    dict(c0=20, c1=12),                                   # a chunk of 4 or 8 channels over both sources
    dict(c0=8, c1=8),
    dict(layer=G.GC_T2, c0=24, c1=8, ohs=16, ows=16),
    dict(layer=G.GC_GRU1, c0=120, c1=136, cout=384, hc=128, h=P, zb=P, rhb=P, qxb=P),
])
def test_forward_entry_refuses_a_split_that_straddles_a_chunk(over):
    """Two sources whose first is no multiple of the 16 packed channels: a chunk over x0's last
    channels would read zeros past them and x1's first channels would be skipped.  Refused
    before any launch (the pointers are placeholders), as nlspn_gconv_wgrad refuses it."""
    rc, text = _gconv(**over)
    assert rc == _lib.EINVAL and "straddle" in text and f"c0 = {over['c0']}" in text, (rc, text)


def test_forward_entry_validates_a_good_split_past_the_chunk_rule():
    # the same call with c0 = 16 passes the channel rule: the next refusal is another one
    rc, text = _gconv(c0=16, c1=16, ohs=9)
    assert rc == _lib.EINVAL and "stored size" in text and "straddle" not in text, (rc, text)
    rc, text = _gconv(c0=20, c1=0, x1=None, ohs=9)  # one source: any channel count
    assert rc == _lib.EINVAL and "stored size" in text, (rc, text)


def test_wgrad_workspace_is_a_pure_function_of_the_shape():
    lib = _lib.get()
    # GRU [convz; convr] at NYU B=8: 64 x 32 channel tiles -> 4 x 8 tiles, 512 / 32 = 16 K slices of
    # 256 x 256 x 9 floats, then the bias partials (one slice per 16384 elements of a plane set)
    n = lib.nlspn_gconv_wgrad_workspace_bytes(1, 256, 256, 8, 29, 38, 29, 38)
    assert n == 4 * (16 * 256 * 256 * 9 + 1 * 256)
    assert lib.nlspn_gconv_wgrad_workspace_bytes(3, 256, 256, 8, 29, 38, 29, 38) == 0
    # the narrow last decoder layer (small 16 channels, large 8): one-wave 16 x 16 tiles
    n = lib.nlspn_gconv_wgrad_workspace_bytes(2, 16, 8, 2, 28, 36, 50, 70)
    assert n == 4 * (56 * 16 * 16 * 9 + 1 * 16)


def test_adjoint_packers_invert_and_match_the_forward_packers():
    torch.manual_seed(0)
    for cout, cin in ((128, 256), (256, 16), (16, 9), (16, 1)):
        conv = torch.nn.Conv2d(cin, cout, 3, 2, 1)
        dg, adj = G.pack_adjoint(conv)
        assert dg == (G.GC_DG_T2_C16 if cin <= 16 else G.GC_DG_T2)
        # the dgrad weights of a stride-2 conv are pack_convt of the same tensor
        assert torch.equal(adj, G.pack_convt(conv.weight, None, G.GC_T2_C16 if cin <= 16 else G.GC_T2)[0])
        assert torch.equal(G.unpack_convt(adj, cout, cin, dg), conv.weight.detach())
    for cin, cout in ((128, 256), (256, 16), (16, 8)):
        convt = torch.nn.ConvTranspose2d(cin, cout, 3, 2, 1, 1)
        dg, adj = G.pack_adjoint(convt)
        assert dg == (G.GC_DG_S2_C16 if cin <= 16 else G.GC_DG_S2)
        assert torch.equal(G.unpack_conv(adj, cin, cout, dg), convt.weight.detach())
    w = torch.randn(256, 256, 3, 3)
    adj = G.pack_adjoint_s1(w)
    assert torch.equal(G.unpack_conv(adj, 256, 256, G.GC_DG_S1), w.transpose(0, 1).flip(2, 3))
    # the forward packers round-trip through the same inverses
    assert torch.equal(G.unpack_conv(G.pack_conv(w, None, G.GC_GRU2)[0], 256, 256, G.GC_GRU2), w)


def _convt_tap_slot(ky, kx):
    """(output phase 2 py + px, taps of the phase, the tap's index in it) in the kernel's order
    (csrc/nlspn_gconv.h gc_tap): py = 0 reads ky = 1, py = 1 reads ky = 0, 2; likewise kx."""
    py, px = int(ky != 1), int(kx != 1)
    return 2 * py + px, (2 if py else 1) * (2 if px else 1), (ky // 2) * (2 if px else 1) + kx // 2


@pytest.mark.parametrize("cout,cin,layer,co", [(72, 20, G.GC_S2, 64), (24, 40, G.GC_S2_C16, 16), (192, 40, G.GC_GRU2, 64)])
def test_pack_conv_puts_each_weight_at_its_place(cout, cin, layer, co):
    """[co_tile][cin_pad][9][co]: one interior element and one of the last partial tile, by an
    index computed here (a pack / unpack pair that are wrong together does not pass); padding zero."""
    w = torch.randn((cout, cin, 3, 3), generator=torch.Generator().manual_seed(cout + cin))
    wpk, bpk = G.pack_conv(w, None, layer)
    assert G._layout(layer) == (co, 16, False)
    ct, cp = -(-cout // co), -(-cin // 16) * 16
    assert wpk.dtype == torch.float32 and wpk.numel() == ct * cp * 9 * co and bpk.numel() == ct * co and not bool(bpk.any())
    for o, i, ky, kx in ((5, 3, 1, 2), (cout - 1, cin - 1, 2, 0)):
        assert float(wpk[(((o // co) * cp + i) * 9 + 3 * ky + kx) * co + o % co]) == float(w[o, i, ky, kx])
    assert cout % co != 0 or cin % 16 != 0  # (the second element lies in a partial tile)
    assert int((wpk != 0).sum()) == int((w != 0).sum())
    assert torch.equal(G.unpack_conv(wpk, cout, cin, layer), w)


@pytest.mark.parametrize("cin,cout,layer,co", [(40, 72, G.GC_T2, 64), (20, 8, G.GC_T2_C16, 16)])
def test_pack_convt_puts_each_weight_at_its_place(cin, cout, layer, co):
    """[phase][co_tile][cin_pad][ntap][co], the phases and their taps in the kernel's order."""
    assert G._T_TAPS == [[(1, 1)], [(1, 0), (1, 2)], [(0, 1), (2, 1)], [(0, 0), (0, 2), (2, 0), (2, 2)]]
    w = torch.randn((cin, cout, 3, 3), generator=torch.Generator().manual_seed(cout + cin))
    wpk, bpk = G.pack_convt(w, None, layer)
    assert G._layout(layer) == (co, 16, True)
    ct, cp = -(-cout // co), -(-cin // 16) * 16
    assert wpk.dtype == torch.float32 and wpk.numel() == ct * cp * 9 * co and not bool(bpk.any())
    for o, i, ky, kx in ((5, 3, 1, 2), (5, 3, 1, 1), (cout - 1, cin - 1, 2, 0), (cout - 1, cin - 1, 2, 2)):
        phase, ntap, t = _convt_tap_slot(ky, kx)
        base = sum(n for n in (1, 2, 2, 4)[:phase]) * ct * cp * co
        assert float(wpk[base + (((o // co) * cp + i) * ntap + t) * co + o % co]) == float(w[i, o, ky, kx])
    assert int((wpk != 0).sum()) == int((w != 0).sum())
    assert torch.equal(G.unpack_convt(wpk, cin, cout, layer), w)


NEW_KERNELS = ("gwgrad_kernel", "gwgrad_reduce_kernel", "gbias_partial_kernel", "ggates_kernel", "gconv_kernel")


def test_backward_unit_compiles_without_scratch(tmp_path):
    sys.path.insert(0, CSRC)
    import resource_usage as RU
    path = os.path.join(RU.BUILD_DIR, "nlspn_kern_gconv_bwd.ru.txt")
    if os.path.exists(path):
        rows = RU.parse(open(path).read())
    else:
        out = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
                              "-ffp-contract=off", "-Rpass-analysis=kernel-resource-usage", "-c", "-o",
                              str(tmp_path / "bwd.o"), os.path.join(CSRC, "nlspn_kern_gconv_bwd.hip")],
                             capture_output=True, text=True, cwd=CSRC)
        assert out.returncode == 0, out.stderr[-2000:]
        rows = RU.parse(out.stderr)
    # 5 data-gradient presets, 4 weight-gradient tilings, the reduce / bias / gates kernels
    assert len(rows) == 12 and all(any(k in n for k in NEW_KERNELS) for n in rows), sorted(rows)
    for k in NEW_KERNELS:
        assert any(k in n for n in rows), k
    bad = {n: (r.get("ScratchSize"), r.get("VGPRs Spill")) for n, r in rows.items()
           if r.get("ScratchSize", 0) != 0 or r.get("VGPRs Spill", 0) != 0}
    assert not bad, bad


# ------------------------------------------------------------------ the per-element cases (tests/_gconv_bwd_cases.py)
import _gconv_bwd_cases as bc  # noqa: E402

DG_IDS = [c["id"] for c in bc.DG_CASES]
GW_IDS = [c["id"] for c in bc.GW_CASES]
GATE_IDS = [c["id"] for c in bc.GATE_CASES]


@pytest.mark.parametrize("cid", ["dg32-2x128>64-6x41-off1.1", "dg33-2x32>16-6x41-off0.1", "dg34-2x64>128-6x41-off1.7",
                                 "dg35-2x8>16-6x41-off7.0", "dg36-2x128>128-5x38"])
def test_dgrad_reference_is_the_input_gradient_of_the_torch_module(cid):
    """The float64 reference of each preset kind against the module the model holds: a stride-2
    Conv2d (presets 32 / 33), a ConvTranspose2d whose output is cropped (34 / 35), a stride-1
    Conv2d (36), each with a bias (which the gradient must not see)."""
    c, o = bc.DG_BY_ID[cid], bc.dgrad_operands(cid)
    if c["mode"] == bc.S2:
        mod = torch.nn.ConvTranspose2d(c["cout"], c["cg"], 3, 2, 1, 1)
    else:
        mod = torch.nn.Conv2d(c["cout"], c["cg"], 3, 2 if c["mode"] == bc.T2 else 1, 1)
    mod = mod.double()
    with torch.no_grad():
        mod.weight.copy_(o["w"])
    x = torch.randn((c["B"], c["cout"], c["Ho"], c["Wo"]), dtype=torch.float64, requires_grad=True)
    y = mod(x)[..., :c["Hg"], :c["Wg"]]
    (y * o["g"].double()).sum().backward()
    ref = bc.dgrad_linear(c, o["g"].double(), o["w"].double())
    assert float(x.grad.abs().max()) > 0.1
    assert torch.allclose(ref, x.grad, rtol=1e-12, atol=1e-12 * float(x.grad.abs().max()))


@pytest.mark.parametrize("cid", DG_IDS)
def test_dgrad_bound_dominates_and_float32_is_within_a_quarter_of_the_bar(cid):
    """X >= |ref| everywhere, and R32: torch's float32 evaluation of the same operation on the
    CPU is within c / 4 of the float64 reference at every element (tanh: beside e)."""
    R = bc.dgrad_reference(cid)
    assert bool((R["X"] * (1 + 1e-12) >= R["ref"].abs()).all())
    assert bool(torch.isfinite(R["ref"]).all()) and float(R["c"].max()) <= bc.C_MFMA
    got = bc.dgrad_float32(cid).double()
    assert bool(((got - R["ref"]).abs() <= 0.25 * R["c"] * R["X"] + R["e"]).all()), bc.ratio(got, R["ref"], R["X"], R["e"])


@pytest.mark.parametrize("cid", ["dg32-2x128>64-7x21-off1.0-relu-add.sep", "dg34-2x64>128-7x21-off1.0-relu-add.sep",
                                 "dg36-2x128>128-7x21-relu-scale0.1-add.sep", "dg35-2x8>16-6x41-off1.7"])
def test_dgrad_bound_is_the_gradient_when_nothing_is_negative(cid):
    R = bc.dgrad_reference(cid, "nonneg")
    assert float(R["ref"].max()) > 1 and torch.allclose(R["ref"], R["X"], rtol=1e-14, atol=0)


@pytest.mark.parametrize("cid", ["dg34-2x64>128-6x41-off1.7", "dg35-2x8>16-6x41-off7.0", "dg34-2x64>128-6x41-off7.7"])
def test_cropped_gradient_reference_is_the_uncropped_one_with_zero_rows(cid):
    c, o = bc.DG_BY_ID[cid], bc.dgrad_operands(cid)
    full = dict(c, Hg=2 * c["Ho"], Wg=2 * c["Wo"])
    gz = torch.zeros((c["B"], c["cg"], full["Hg"], full["Wg"]), dtype=torch.float64)
    gz[..., :c["Hg"], :c["Wg"]] = o["g"]
    a, b = bc.dgrad_linear(c, o["g"].double(), o["w"].double()), bc.dgrad_linear(full, gz, o["w"].double())
    assert c["Hg"] < full["Hg"] or c["Wg"] < full["Wg"]
    assert torch.allclose(a, b, rtol=1e-12, atol=1e-13)


@pytest.mark.parametrize("cid", GW_IDS)
def test_wgrad_plan_mirror_bound_and_float32_condition(cid):
    """The mirror's workspace equals the library's query (no device), the case hits the edges
    its id claims, X >= |ref|, and R32 for dW and db."""
    c = bc.GW_BY_ID[cid]
    p = bc.gw_plan_of(c)
    need = _lib.get().nlspn_gconv_wgrad_workspace_bytes(c["stride"], c["Cs"], c["c0"] + c["c1"], c["B"], c["Hs"], c["Ws"],
                                                        c["Hl"], c["Wl"])
    assert need == 4 * p["floats"] > 0
    assert c["edges"] <= bc.gw_edges(p), (c["edges"] - bc.gw_edges(p), p)
    if c["stride"] == 2:  # the large size from {2 Hs, 2 Hs - 1, 2 Hs - 7} x {2 Ws, 2 Ws - 1, 2 Ws - 7}
        assert 2 * c["Hs"] - c["Hl"] in (0, 1, 7) and 2 * c["Ws"] - c["Wl"] in (0, 1, 7)
    assert c["c1"] == 0 or (c["c0"] % 16 == 0 and not c["bfl"])
    R = bc.wgrad_case_reference(cid)
    assert bool((R["Xw"] * (1 + 1e-12) >= R["dw"].abs()).all()) and bool((R["Xb"] * (1 + 1e-12) >= R["db"].abs()).all())
    dw32, db32 = bc.wgrad_float32(cid)
    assert bool(((dw32.double() - R["dw"]).abs() <= 0.25 * R["cw"] * R["Xw"]).all()), bc.ratio(dw32, R["dw"], R["Xw"])
    assert bool(((db32.double() - R["db"]).abs() <= 0.25 * R["cb"] * R["Xb"]).all()), bc.ratio(db32, R["db"], R["Xb"])


def test_wgrad_cases_cover_every_tiling_and_edge():
    by = {}
    for c in bc.GW_CASES:
        e = bc.gw_edges(bc.gw_plan_of(c))
        by.setdefault(next(x for x in e if x.startswith("tiling")), set()).update(e)
        assert c["Ws"] in (1, 3, 13, 18, 36, 48, 64, 65, 130)
    assert set(by) == {"tiling1222", "tiling2222", "tiling2241", "tiling2111"}
    for t, e in by.items():
        assert {"bands1", "bands2", "bands3", "units1", "last_slice_short", "padded_kstep"} <= e, (t, e)
    assert any(c["Hs"] == 1 for c in bc.GW_CASES) and {c["scale"] for c in bc.GW_CASES} == {1.0, 0.1}
    assert {(c["bfl"], bc.gw_plan_of(c)["nsb"] > 1) for c in bc.GW_CASES} == {(False, False), (False, True), (True, False), (True, True)}
    # three bands of 130: 44 | 44 | 42, the last one's k-steps padded to 44; two bands of 65: 33 | 32
    assert bc.gw_plan(1, 24, 40, 1, 2, 130, 2, 130)["widths"] == [44, 44, 42] and bc.gw_plan(1, 24, 40, 1, 2, 130, 2, 130)["k4"][-1] == 44
    assert bc.gw_plan(1, 40, 48, 2, 3, 65, 3, 65)["widths"] == [33, 32]


@pytest.mark.parametrize("cid", DG_IDS)
def test_dgrad_case_hits_its_claimed_edge(cid):
    c = bc.DG_BY_ID[cid]
    assert c["edges"] <= bc.dg_edges(c["preset"], c["gh"], c["gw"]), (c["edges"], bc.dg_edges(c["preset"], c["gh"], c["gw"]))
    if c["mode"] == bc.T2:
        assert (c["Hg"], c["Wg"]) == (c["gh"], c["gw"]) and 2 * c["Hg"] - c["Ho"] in (0, 1) and 2 * c["Wg"] - c["Wo"] in (0, 1)
    elif c["mode"] == bc.S2:
        assert (c["Ho"], c["Wo"]) == (c["gh"], c["gw"]) and 0 <= 2 * c["Ho"] - c["Hg"] <= 7 and 0 <= 2 * c["Wo"] - c["Wg"] <= 7
    assert c["cg"] * c["Hg"] * c["Wg"] <= 256 * 17 * 39 * 4 and c["cout"] <= 256


def test_dgrad_grids_are_the_forward_tests_and_the_s1_empty_tile_grid_is_the_smallest():
    assert {(c["preset"], c["gh"], c["gw"]) for c in bc.DG_A} >= {
        (32, 17, 39), (32, 3, 43), (33, 27, 160), (33, 4, 129), (34, 14, 23), (34, 4, 33), (35, 17, 37), (35, 3, 43), (36, 17, 39)}
    empty = [(gh * gw, gh, gw) for gh in range(1, 24) for gw in range(1, 130) if bc.gc_tiling(*bc.DG_GEO[36], gh, gw)["empty_last"]]
    assert min(empty)[1:] == (3, 43) and (36, 3, 43) in {(c["preset"], c["gh"], c["gw"]) for c in bc.DG_A}
    # the mirror's geometry is the library's: the output-channel tile of every data-gradient preset
    for preset, co in bc.DG_CO_TILE.items():
        assert G._layout(preset)[0] == co and G._layout(preset)[2] == (bc.DG_GEO[preset][0] == bc.T2)


def test_planted_values_survive_the_seeding():
    for c in bc.DG_CASES:
        o = bc.dgrad_operands(c["id"])
        if c["act"] == bc.ACT_RELU:
            y = o["ysave"].view(-1)
            assert y[:6].tolist() == list(bc.RELU_PLANTS) and bool(torch.signbit(y[1])) and not bool(torch.signbit(y[0]))
            assert int((y == 0).sum()) > 6 and int((y < 0).sum()) == 2 and float(y[2]) == 2.0 ** -126
        elif c["act"] == bc.ACT_TANH:
            y = o["ysave"].view(-1)
            assert y[:6].double().tolist() == list(bc.TANH_PLANTS) and float(y.abs().max()) == 1.0 and c["scale"] == 0.1
        else:
            assert o["ysave"] is None
        assert (o["add"] is None) == (c["add"] == "none")
    o = bc.gate_operands("gates-stage1-3x128x5x7")
    assert o["z"][-1].view(-1)[:2].tolist() == [0.0, 1.0] and o["r"][-1].view(-1)[:3].tolist() == [0.0, 1.0, 0.5]
    assert o["q"][-1].view(-1)[:2].tolist() == [1.0, -1.0] and torch.equal(o["q"][-1].view(-1)[5:9], o["h"][-1].view(-1)[5:9])
    assert (3 * 128 * 5 * 7) % 256 != 0
    for cid in ("gates-stage0-relu", "gates-stage0-tanh"):
        y = bc.gate_operands(cid)["z"].view(-1)
        assert y[:6].double().tolist() == list(bc.RELU_PLANTS if cid.endswith("relu") else bc.TANH_PLANTS)
    assert bc.SEEDS == {} or all(k in bc.DG_BY_ID or k in bc.GW_BY_ID or k in bc.GATE_BY_ID for k in bc.SEEDS)


@pytest.mark.parametrize("cid", GATE_IDS)
def test_gate_bound_dominates_and_float32_is_within_a_quarter_of_the_bar(cid):
    want, f32 = bc.gate_formulas(cid, torch.float64), bc.gate_formulas(cid, torch.float32)
    for k, (ref, X) in want.items():
        assert bool((X * (1 + 1e-12) >= ref.abs()).all())
        got = f32[k][0].double()
        assert bool(((got - ref).abs() <= 0.25 * bc.C_GATES * X).all()), (k, bc.ratio(got, ref, X) / bc.U)
