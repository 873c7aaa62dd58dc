"""CPU: the entry points of the streaming weight gradient of the narrow layers
(include/nlspn_prop.h: nlspn_gconv_wgrad_narrow, its workspace query and its coverage query) are
declared everywhere, agree with gwn_covers, refuse bad arguments before touching a device and
forward the declined shapes' workspace; the Python layers expose and validate the switch; the new
translation unit compiles without scratch; every case of tests/_gwnarrow_cases.py hits the edges
it claims and meets the bar's condition (a float32 evaluation within a quarter of c)."""
import ctypes
import os
import subprocess
import sys
import types

import pytest

import _gconv_bwd_cases as bc
import _gwnarrow_cases as nc
from nlspn_eccv20_amd import NLSPNModel, _lib
from nlspn_eccv20_amd.gru import GruConvs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nlspn_eccv20_amd", "csrc")
P = ctypes.c_void_p(64)  # never dereferenced: validation fails first
NAMES = ("nlspn_gconv_wgrad_narrow", "nlspn_gconv_wgrad_narrow_workspace_bytes", "nlspn_gconv_wgrad_narrow_covers")


def test_signatures_and_header_list_the_entry_points():
    for name in NAMES:
        assert name in _lib.SIGNATURES and name in _lib.header_symbols() and name in _lib.AB_OPTIONAL
        assert hasattr(_lib.get(), name)
    assert _lib.SIGNATURES["nlspn_gconv_wgrad_narrow"] == _lib.SIGNATURES["nlspn_gconv_wgrad"]
    assert _lib.SIGNATURES["nlspn_gconv_wgrad_narrow_workspace_bytes"] == _lib.SIGNATURES["nlspn_gconv_wgrad_workspace_bytes"]
    assert _lib.get().nlspn_abi_version() == 3


def test_covers_is_gwn_covers_over_a_grid():
    lib = _lib.get()
    n = 0
    for stride in (0, 1, 2, 3):
        for Cs in (0, 1, 3, 8, 15, 16, 17, 40):
            for c0 in (0, 1, 5, 8, 9, 16, 17, 32):
                for c1 in (0, 1, 16):
                    want = stride == 2 and 1 <= Cs <= 16 and 1 <= c0 <= 16 and c1 == 0
                    assert nc.gwn_covers(stride, Cs, c0, c1) == want
                    assert lib.nlspn_gconv_wgrad_narrow_covers(stride, Cs, c0, c1) == int(want), (stride, Cs, c0, c1)
                    n += want
    assert n == 5 * 5


@pytest.mark.parametrize("shape", [(2, 40, 16, 2, 13, 18, 26, 36), (2, 16, 17, 2, 13, 18, 25, 35), (1, 16, 16, 2, 7, 9, 7, 9),
                                   (1, 256, 256, 8, 29, 38, 29, 38)])
def test_a_declined_shapes_workspace_is_the_f32_entrys(shape):
    lib = _lib.get()
    assert not nc.gwn_covers(shape[0], shape[1], shape[2], 0)
    assert lib.nlspn_gconv_wgrad_narrow_workspace_bytes(*shape) == lib.nlspn_gconv_wgrad_workspace_bytes(*shape) > 0


def test_workspace_of_a_covered_shape_and_of_a_bad_one():
    lib = _lib.get()
    # NYU 228 x 304, B = 8: 8 x 29 groups x 3 bands = 696 units, two per slice: 348 slabs of nb 256 + 16 floats
    assert lib.nlspn_gconv_wgrad_narrow_workspace_bytes(2, 16, 1, 8, 114, 152, 228, 304) == 4 * 348 * (1 * 256 + 16)
    assert lib.nlspn_gconv_wgrad_narrow_workspace_bytes(2, 16, 8, 8, 114, 152, 228, 304) == 4 * 348 * (5 * 256 + 16)
    assert lib.nlspn_gconv_wgrad_narrow_workspace_bytes(2, 16, 9, 8, 114, 152, 229, 304) == 0   # larger than twice the small size
    assert lib.nlspn_gconv_wgrad_narrow_workspace_bytes(3, 16, 9, 8, 114, 152, 228, 304) == 0


def _wgrad(**over):
    lib = _lib.get()
    a = dict(stride=2, s=P, Cs=16, l0=P, c0=8, l1=None, c1=0, dw=P, db=P, bias_from_large=1, scale=1.0, ws=P,
             ws_bytes=lib.nlspn_gconv_wgrad_narrow_workspace_bytes(2, 16, 8, 2, 8, 8, 16, 15), B=2, Hs=8, Ws=8, Hl=16, Wl=15,
             stream=None)
    a.update(over)
    rc = lib.nlspn_gconv_wgrad_narrow(*a.values())
    return rc, lib.nlspn_last_error().decode()


@pytest.mark.parametrize("over,msg", [
    (dict(s=None), "null"),
    (dict(l0=None), "null"),
    (dict(dw=None), "null"),
    (dict(ws=None), "null"),
    (dict(c0=0), "bad channels"),
    (dict(c1=8), "bad channels"),                      # a second source without its tensor
    (dict(c1=8, l1=P), "straddle"),
    (dict(c0=16, c1=16, l1=P), "one source"),          # the bias gradient from two sources
    (dict(stride=3), "stride"),
    (dict(Hl=17), "does not belong"),
    (dict(Wl=17), "does not belong"),
    (dict(B=0), "bad shape"),
    (dict(Hs=0), "bad shape"),
    (dict(ws_bytes=1024), "workspace too small"),      # the narrow plan's own size
    (dict(Cs=40, ws_bytes=1024), "workspace too small"),  # a declined shape: the f32 entry's refusal
])
def test_entry_point_validates_first(over, msg):
    rc, text = _wgrad(**over)
    assert rc == _lib.EINVAL and msg in text, (rc, text)


def _model():
    args = types.SimpleNamespace(prop_kernel=3, affinity="TGASS", affinity_gamma=0.5, prop_time=3,
                                 preserve_input=True, always_clip=False, conf_prop=True, offset=True,
                                 network="resnet34", from_scratch=True, zero_init_aff=False, use_GRU=True,
                                 use_S2D=False, GRU_hidden_dim=128, GRU_input_dim=128, lr=1e-3, max_depth=10.0,
                                 patch_height=48, patch_width=64, model_name="NLSPN")
    return NLSPNModel(args)


def test_model_property_validates_and_forwards():
    m = _model()
    assert m.gru_wgrad_narrow is False and m._gru_convs.wgrad_narrow is False and m.native_gru_train is False
    for bad in (1, 0, "yes", None):
        with pytest.raises(ValueError, match="gru_wgrad_narrow"):
            m.gru_wgrad_narrow = bad
        assert m.gru_wgrad_narrow is False
    m.gru_wgrad_narrow = True
    assert m.gru_wgrad_narrow is True and m._gru_convs.wgrad_narrow is True
    assert m.gru_wgrad_precision == "fp32"   # the two switches are apart
    m.gru_wgrad_narrow = False
    assert m._gru_convs.wgrad_narrow is False


def test_gruconvs_counts_the_entry_apart():
    gc = GruConvs()
    assert gc.wgrad_narrow is False and gc.stats["wgrad_narrow"] == 0 and gc.stats["wgrad"] == 0
    gc.stats["wgrad_narrow"] += 2
    gc.reset_stats()
    assert gc.stats["wgrad_narrow"] == 0


def test_new_unit_compiles_without_scratch(tmp_path):
    sys.path.insert(0, CSRC)
    import resource_usage as RU
    path = os.path.join(RU.BUILD_DIR, "nlspn_kern_gwnarrow.ru.txt")
    if os.path.exists(path):
        rows = RU.parse(open(path).read())
    else:
        out = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
                              "-ffp-contract=off", "-Rpass-analysis=kernel-resource-usage", "-c", "-o",
                              str(tmp_path / "gwn.o"), os.path.join(CSRC, "nlspn_kern_gwnarrow.hip")],
                             capture_output=True, text=True, cwd=CSRC)
        assert out.returncode == 0, out.stderr[-2000:]
        rows = RU.parse(out.stderr)
    # the kernels of 1 .. 9 N blocks and the reduce
    assert len(rows) == 10 and sum("gwnarrow_kernel" in n for n in rows) == 9 and sum("gwnarrow_reduce_kernel" in n for n in rows) == 1, sorted(rows)
    bad = {n: (r.get("ScratchSize"), r.get("VGPRs Spill")) for n, r in rows.items()
           if r.get("ScratchSize", 0) != 0 or r.get("VGPRs Spill", 0) != 0}
    assert not bad, bad


# ------------------------------------------------------------------ the cases
def test_the_table_covers_what_it_must():
    got = set().union(*(nc.gwn_edges(c, nc.plan_of(c)) for c in nc.CASES))
    for e in ("units1", "full_band", "band_plus_one", "bands3", "hs1", "hsR", "hsR+1", "hs_not_multiple", "images>1",
              "slice_crosses_images", "last_slice_short", "odd_wl", "misaligned", "scaled", "nsl>1", "db_small", "db_large",
              "crop0x0", "crop1x1", "crop7x7", "crop0x1", "crop1x0", "crop0x7"):
        assert e in got, e
    chans = {(c["Cs"], c["c0"], c["bfl"]) for c in nc.CASES}
    assert {(16, 1, False), (16, 9, False), (16, 8, True), (8, 16, True), (16, 16, False), (3, 5, False)} <= chans
    # db from either side, each with and without a crop, and from more than one slice
    for bfl in (False, True):
        crops = {(2 * c["Hs"] - c["Hl"], 2 * c["Ws"] - c["Wl"]) == (0, 0) for c in nc.CASES if c["bfl"] == bfl}
        assert crops == {True, False}, bfl
        assert any(nc.plan_of(c)["nsl"] > 1 for c in nc.CASES if c["bfl"] == bfl)


@pytest.mark.parametrize("cid", [c["id"] for c in nc.CASES])
def test_case_hits_its_edges_and_is_covered(cid):
    c = nc.BY_ID[cid]
    p = nc.plan_of(c)
    assert nc.gwn_covers(2, c["Cs"], c["c0"], c["c1"]) and c["Hl"] <= 2 * c["Hs"] and c["Wl"] <= 2 * c["Ws"]
    assert c["B"] * c["Hs"] * c["Ws"] <= 10 ** 5
    assert c["edges"] <= nc.gwn_edges(c, p), (c["edges"] - nc.gwn_edges(c, p), p)
    assert _lib.get().nlspn_gconv_wgrad_narrow_workspace_bytes(*nc.shape_of(c)) == 4 * p["floats"]
    assert p["lds_bytes"] <= 160 * 1024 and sum(p["widths"]) == c["Ws"] and max(p["widths"]) <= nc.BW


@pytest.mark.parametrize("cid", [c["id"] for c in nc.CASES])
def test_float32_evaluation_is_within_a_quarter_of_the_bar(cid):
    R = nc.reference(cid)
    dw32, db32 = nc.float32(cid)
    rw = bc.ratio(dw32, R["dw"], R["Xw"]) / float(R["cw"].min())
    rb = bc.ratio(db32, R["db"], R["Xb"]) / R["cb"]
    assert rw <= 0.25 and rb <= 0.25, (cid, rw, rb)


def test_the_perturbed_reference_is_outside_the_bar():
    """The reference without the last slice's units (tests/test_gpu_gwnarrow_elem.py shows with it
    that the check can fail) is farther from the true one than the bar allows."""
    cid = "n16-9-5x65-band-plus-one-crop1"
    a, b = nc.reference(cid), nc.reference(cid, "skip_last_slice")
    assert bool(((a["dw"] - b["dw"]).abs() > a["cw"] * a["Xw"]).any())
