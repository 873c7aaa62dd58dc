"""CPU: the entry points of the split-bf16 weight gradient (include/nlspn_prop.h:
nlspn_gconv_wgrad_bf16x3, nlspn_gconv_wgrad_bf16x3_workspace_bytes) refuse bad arguments before
touching a device, the Python layers expose and validate the mode, and the new translation unit
compiles without scratch."""
import ctypes
import os
import subprocess
import sys
import types

import pytest

from nlspn_eccv20_amd import NLSPNModel, _lib
from nlspn_eccv20_amd.gru import GruConvs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nlspn_eccv20_amd", "csrc")
P = ctypes.c_void_p(64)  # never dereferenced: validation fails first


def _wgrad(**over):
    lib = _lib.get()
    a = dict(stride=1, s=P, Cs=128, l0=P, c0=128, l1=P, c1=128, dw=P, db=P, bias_from_large=0, scale=1.0, ws=P,
             ws_bytes=lib.nlspn_gconv_wgrad_bf16x3_workspace_bytes(1, 128, 256, 1, 8, 8, 8, 8), B=1, Hs=8, Ws=8, Hl=8, Wl=8,
             stream=None)
    a.update(over)
    rc = lib.nlspn_gconv_wgrad_bf16x3(*a.values())
    return rc, lib.nlspn_last_error().decode()


@pytest.mark.parametrize("over,msg", [
    (dict(s=None), "null"),
    (dict(l0=None), "null"),
    (dict(dw=None), "null"),
    (dict(ws=None), "null"),
    (dict(l1=None), "bad channels"),
    (dict(c0=0), "bad channels"),
    (dict(c0=120, c1=136), "straddle"),
    (dict(ws_bytes=1024), "workspace too small"),
    (dict(stride=3), "stride"),
    (dict(stride=0), "stride"),
    (dict(Hl=9), "does not belong"),                  # stride 1: the sizes are equal
    (dict(stride=2, Hl=17, Wl=16), "does not belong"),  # stride 2: at most twice the small size
    (dict(B=0), "bad shape"),
    (dict(bias_from_large=1), "one source"),
    # both channel counts <= 16: forwarded to the f32 entry, whose checks are the same
    (dict(Cs=16, c0=9, c1=0, l1=None, ws_bytes=16), "workspace too small"),
])
def test_entry_point_validates_first(over, msg):
    rc, text = _wgrad(**over)
    assert rc == _lib.EINVAL and msg in text, (rc, text)


def test_signatures_and_header_list_the_entry_points():
    for name in ("nlspn_gconv_wgrad_bf16x3", "nlspn_gconv_wgrad_bf16x3_workspace_bytes"):
        assert name in _lib.SIGNATURES and name in _lib.header_symbols() and name in _lib.AB_OPTIONAL
        assert hasattr(_lib.get(), name)
    assert _lib.SIGNATURES["nlspn_gconv_wgrad_bf16x3"] == _lib.SIGNATURES["nlspn_gconv_wgrad"]
    assert _lib.SIGNATURES["nlspn_gconv_wgrad_bf16x3_workspace_bytes"] == _lib.SIGNATURES["nlspn_gconv_wgrad_workspace_bytes"]
    assert _lib.get().nlspn_abi_version() == 3


def test_the_f32_workspace_query_is_unchanged():
    lib = _lib.get()
    assert lib.nlspn_gconv_wgrad_workspace_bytes(1, 256, 256, 8, 29, 38, 29, 38) == 4 * (16 * 256 * 256 * 9 + 1 * 256)
    # the new mode plans fewer, larger slices (128 x 16 tiles: 2 x 16 = 32 tiles, 256 / 32 = 8 slices)
    assert lib.nlspn_gconv_wgrad_bf16x3_workspace_bytes(1, 256, 256, 8, 29, 38, 29, 38) == 4 * (8 * 256 * 256 * 9 + 1 * 256)


def _model():
    args = types.SimpleNamespace(prop_kernel=3, affinity="TGASS", affinity_gamma=0.5, prop_time=3,
                                 preserve_input=True, always_clip=False, conf_prop=True, offset=True,
                                 network="resnet34", from_scratch=True, zero_init_aff=False, use_GRU=True,
                                 use_S2D=False, GRU_hidden_dim=128, GRU_input_dim=128, lr=1e-3, max_depth=10.0,
                                 patch_height=48, patch_width=64, model_name="NLSPN")
    return NLSPNModel(args)


def test_model_property_validates_and_forwards():
    m = _model()
    assert m.gru_wgrad_precision == "fp32" and m._gru_convs.wgrad_precision == "fp32"
    assert m.native_gru_train is False
    for bad in ("bf16", "fp16", None):
        with pytest.raises(ValueError, match="gru_wgrad_precision"):
            m.gru_wgrad_precision = bad
        assert m.gru_wgrad_precision == "fp32"
    m.gru_wgrad_precision = "bf16x3"
    assert m.gru_wgrad_precision == "bf16x3" and m._gru_convs.wgrad_precision == "bf16x3"
    assert m.gru_precision == "fp32"   # the inference setting is another one
    m.gru_wgrad_precision = "fp32"
    assert m._gru_convs.wgrad_precision == "fp32"


def test_gruconvs_counts_the_mode_apart():
    gc = GruConvs()
    assert gc.wgrad_precision == "fp32" and gc.stats["wgrad_x3"] == 0 and gc.stats["wgrad"] == 0
    gc.stats["wgrad_x3"] += 4
    gc.reset_stats()
    assert gc.stats["wgrad_x3"] == 0


def test_new_unit_compiles_without_scratch(tmp_path):
    sys.path.insert(0, CSRC)
    import resource_usage as RU
    path = os.path.join(RU.BUILD_DIR, "nlspn_kern_gwgrad16.ru.txt")
    if os.path.exists(path):
        rows = RU.parse(open(path).read())
    else:
        out = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
                              "-ffp-contract=off", "-Rpass-analysis=kernel-resource-usage", "-c", "-o",
                              str(tmp_path / "gw16.o"), os.path.join(CSRC, "nlspn_kern_gwgrad16.hip")],
                             capture_output=True, text=True, cwd=CSRC)
        assert out.returncode == 0, out.stderr[-2000:]
        rows = RU.parse(out.stderr)
    assert len(rows) == 2 and all("gwgrad16_kernel" in n for n in rows), sorted(rows)   # stride 1, stride 2
    bad = {n: (r.get("ScratchSize"), r.get("VGPRs Spill")) for n, r in rows.items()
           if r.get("ScratchSize", 0) != 0 or r.get("VGPRs Spill", 0) != 0}
    assert not bad, bad
