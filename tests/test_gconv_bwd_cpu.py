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
