"""Cases, seeded operands, float64 references and bars of the per-element tests of the GRU-mode
convolutions' backward (csrc/nlspn_gconv_bwd.h, the NLSPN_GC_DG_* presets of csrc/nlspn_gconv.h),
shared by tests/test_gconv_bwd_cpu.py (CPU: the references against torch's modules, the bars
against a float32 evaluation, every case id's claimed edge) and tests/test_gpu_gconv_bwd_elem.py
(GPU: every element of every output through the C ABI).  tests/test_gpu_gwgrad16.py takes
wgrad_reference from here, tests/test_gpu_gconv_fwd.py gc_tiling.

References.  torch on the CPU in float64 on the exact f32 values the device gets, built from
the FORWARD operation (torch.autograd.grad of F.conv2d / F.conv_transpose2d), never from the
packing helpers: pack_adjoint, pack_adjoint_s1, pack_conv and pack_convt are under test too.

Bars.  |got - ref64| <= c * X + e for every element, none excluded; X is the same linear
operation on absolute values (the sum of the absolute values of the monomials).
    dgrad   X = |scale| |act'(ysave)| sum |w||g| + |add|,  c = min(2e-6, (n + 4) 2^-24), n the
            element's own term count (9 cg; transposed adjoints cg x 1, 2 or 4 by output phase);
            tanh adds e = 3 * 2^-24 |scale| sum |w||g| (the roundings of 1 - y y at |y| <= 1)
    wgrad   X = |scale| sum |s||l|,  c = min(2e-6, (n + nsl + 2) 2^-24), n the in-range terms of
            the element, nsl the slice count of the plan;  db likewise with sum |g| and nsb
    gates   c = 8 * 2^-24 (at most six roundings per output)
2e-6 is the project's per-element bar for f32 MFMA accumulation (kinds s2 / t2 / gru1 of
tests/test_gpu_gconv_fwd.py, the second term of C_CAP in tests/test_gpu_gwgrad16.py).  No bar is
derived from the kernels under test.  Condition (tests/test_gconv_bwd_cpu.py): the same operation
evaluated in float32 by torch on the CPU is within a quarter of c of the float64 reference in
every case, so a correct float32 implementation has a 4x margin.

Guarded operands (GPU): every device operand is a view into a NaN buffer with GUARD NaNs on
both sides (a read outside the operand turns an output into NaN), every output is pre-filled
with NaN between two runs of SENT that must be intact afterwards.

Mirrors of the planning arithmetic (gc_tiling of gc_tile, gw_plan of csrc/nlspn_gwgrad_plan.h's
gw_plan) only state which edge a case hits (the `edges` of a case); tests/test_gconv_bwd_cpu.py
checks every claim and ties gw_plan to the library's workspace query,
tests/test_gwgrad16_plan_cpu.py compares it field by field with the launcher's function.
"""
import functools
import math
import zlib

import torch
import torch.nn.functional as F

U = 2.0 ** -24
SENT = -7777.0
GUARD = 4096
C_MFMA = 2e-6
C_GATES = 8 * U
ACT_NONE, ACT_RELU, ACT_TANH = 0, 1, 2
S1, S2, T2 = 0, 1, 2

# data-gradient preset -> (mode, NPX, XR, XP) and its output-channel tile: a mirror of
# NLSPN_GC_DG_CONFIGS (csrc/nlspn_gconv_plan.h) for the edge claims only
DG_GEO = {32: (T2, 64, 6, 40), 33: (T2, 256, 6, 80), 34: (S2, 64, 12, 40), 35: (S2, 64, 10, 72), 36: (S1, 64, 8, 40)}
DG_CO_TILE = {32: 64, 33: 16, 34: 64, 35: 16, 36: 64}
# (cg, cout) per preset, the sides GruConvs.pack_adjoint gives them (hidden width 64 / 128)
DG_CH = {32: (128, 64), 33: (32, 16), 34: (64, 128), 35: (8, 16), 36: (128, 128)}


def gc_bwmax(mode, xp):
    return xp - 2 if mode == S1 else (xp - 3) // 2 + 1 if mode == S2 else xp - 1


def gc_tiling(mode, npx, xr, xp, gh, gw):
    """gc_tile (csrc/nlspn_gconv_plan.h) for a gh x gw grid: nbands, bw, the last band's width
    bwl, the pixels per tile npx and the tiles per band tpb (of the widest band)."""
    bwmax = gc_bwmax(mode, xp)
    nbands = -(-gw // bwmax)
    bw = -(-gw // nbands)
    bwl = gw - (nbands - 1) * bw

    def rows(n):
        dr = (n + bwl - 2) // bwl
        return dr + 3 if mode == S1 else 2 * dr + 3 if mode == S2 else dr + 2
    full = npx
    while npx > 1 and rows(npx) > xr:
        npx -= 1
    tpb = -(-gh * bw // npx)
    return dict(nbands=nbands, bw=bw, bwl=bwl, npx=npx, npx_full=full, tpb=tpb, bwmax=bwmax,
                empty_last=(tpb - 1) * npx >= gh * bwl)


def dg_edges(preset, gh, gw):
    """The edges a tiled grid hits under a data-gradient preset."""
    t = gc_tiling(*DG_GEO[preset], gh, gw)
    e = set()
    if t["nbands"] > 1 and t["bwl"] < t["bw"]:
        e.add("uneven_last_band")
    if t["empty_last"]:
        e.add("empty_tile")
    if gw == t["bwmax"]:
        e.add("full_band")
    if gw == t["bwmax"] + 1:
        e.add("band_plus_one")
    if t["npx"] < t["npx_full"]:
        e.add("npx_shrunk")
    if t["tpb"] > 1:
        e.add("tiles>1")
    return e


# ---------------------------------------------------------------------------- weight gradient plan
GW_TARGET, GW_BW, GW_MAX_BIAS = 512, 64, 64


def gw_plan(stride, Cs, Cl, B, Hs, Ws, Hl, Wl):
    """gw_plan (csrc/nlspn_gwgrad_plan.h): the tiling by channel counts, bands, units, slices
    and workspace floats of one nlspn_gconv_wgrad call."""
    tiling, mt, nt = ("1222", 64, 32) if stride == 1 else ("2222", 64, 32) if Cl > 16 else \
        ("2241", 128, 16) if Cs > 16 else ("2111", 16, 16)
    mtiles, ntiles = -(-Cs // mt), -(-Cl // nt)
    nbands = -(-Ws // GW_BW)
    bw = -(-Ws // nbands)
    units = B * Hs * nbands
    tiles = mtiles * ntiles
    target = -(-GW_TARGET // tiles)
    nsl = max(1, min(units, target))
    ups = -(-units // nsl)
    nsl = -(-units // ups)
    slab = mtiles * mt * ntiles * nt * 9
    nsb = max(1, min(GW_MAX_BIAS, (B * Hl * Wl + 16383) // 16384))
    widths = [min(bw, Ws - b * bw) for b in range(nbands)]
    return dict(tiling=tiling, mtiles=mtiles, ntiles=ntiles, nbands=nbands, bw=bw, widths=widths,
                k4=[(w + 3) & ~3 for w in widths], units=units, target=target, ups=ups, nsl=nsl, nsb=nsb,
                floats=slab * nsl + nsb * max(Cs, Cl))


def gw_edges(p):
    e = {"tiling" + p["tiling"], f"bands{p['nbands']}"}
    if p["units"] == 1:
        e.add("units1")
    if p["ups"] == 1 and p["units"] > 1 and p["units"] < p["target"]:
        e.add("ups1")
    if p["units"] % p["ups"] != 0:
        e.add("last_slice_short")
    if any(k != w for k, w in zip(p["k4"], p["widths"])):
        e.add("padded_kstep")
    if p["nsb"] > 1:
        e.add("nsb>1")
    return e


# ---------------------------------------------------------------------------- case tables
def _seed(cid):
    return SEEDS.get(cid, zlib.crc32(cid.encode()) & 0x7fffffff)


# a case whose first draw missed the float32 condition gets another seed here (none so far)
SEEDS = {}


def _dg(preset, gh, gw, B=2, cg=None, cout=None, ph=0, pw=0, act=ACT_NONE, scale=1.0, split=None, add="none",
        edges=(), tag=""):
    """A data-gradient case on the tiled grid gh x gw.  ph / pw: rows / columns the other side
    is short of twice the grid (T2: Ho = 2 Hg - ph; S2: the stored gradient Hg = 2 Ho - ph)."""
    mode = DG_GEO[preset][0]
    c = DG_CH[preset]
    cg, cout = cg or c[0], cout or c[1]
    if mode == T2:
        Hg, Wg, Ho, Wo = gh, gw, 2 * gh - ph, 2 * gw - pw
    elif mode == S2:
        Hg, Wg, Ho, Wo = 2 * gh - ph, 2 * gw - pw, gh, gw
    else:
        Hg, Wg, Ho, Wo = gh, gw, gh, gw
    cid = f"dg{preset}-{B}x{cg}>{cout}-{gh}x{gw}" + (f"-off{ph}.{pw}" if ph or pw else "") + \
        ("-relu" if act == ACT_RELU else "-tanh" if act == ACT_TANH else "") + (f"-scale{scale:g}" if scale != 1.0 else "") + \
        (f"-split{split}" if split else "") + (f"-add.{add}" if add != "none" else "") + tag
    return dict(id=cid, preset=preset, mode=mode, B=B, cg=cg, cout=cout, gh=gh, gw=gw, Hg=Hg, Wg=Wg, Ho=Ho, Wo=Wo,
                act=act, scale=scale, split=split or cout, add=add, edges=set(edges))


# a. every preset at the forward test's grids for the preset of the same geometry (GRIDS_A of
# tests/test_gpu_gconv_fwd.py): an uneven last band that used to overrun the window rows, and the
# smallest grid with an empty tile in the last band.  32 at 17x39 is one full band (39 columns, as
# the forward preset 4); 36: 17x39 (20 | 19) and 3x43 (22 | 21: the last band's 63 pixels leave its
# second tile empty), the grid of fewest pixels with an empty tile under its geometry.
DG_GRIDS_A = [(32, 17, 39, "full_band"), (32, 3, 43, "empty_tile"), (33, 27, 160, "uneven_last_band"),
              (33, 4, 129, "empty_tile"), (34, 14, 23, "uneven_last_band"), (34, 4, 33, "empty_tile"),
              (35, 17, 37, "uneven_last_band"), (35, 3, 43, "empty_tile"), (36, 17, 39, "uneven_last_band"),
              (36, 3, 43, "empty_tile")]
DG_A = [_dg(p, gh, gw, edges=[e]) for p, gh, gw, e in DG_GRIDS_A]
# the band-edge set (GRIDS_B): one full band, one pixel more, 1x1, one row at full band width, 9x2
DG_BAND = []
for _p in (32, 33, 34, 35, 36):
    _bw = gc_bwmax(DG_GEO[_p][0], DG_GEO[_p][3])
    DG_BAND += [_dg(_p, 5, _bw, edges=["full_band"]), _dg(_p, 5, _bw + 1, edges=["band_plus_one"]), _dg(_p, 1, 1, edges=["npx_shrunk"]),
                _dg(_p, 1, _bw, edges=["full_band"]), _dg(_p, 9, 2, edges=["npx_shrunk"])]
# b. shapes only nlspn_gconv_dgrad has: the stride-2 gradient stored cropped (different crops for
# rows and columns), the transposed adjoint one row / column short; channel edges
DG_SHAPES = [_dg(p, 6, 41, ph=ph, pw=pw) for p in (34, 35) for ph, pw in ((0, 1), (1, 7), (7, 0), (7, 7))] + \
            [_dg(p, 6, 41, ph=ph, pw=pw) for p in (32, 33) for ph, pw in ((0, 0), (0, 1), (1, 0), (1, 1))]
DG_CHANNELS = [_dg(p, 7, 21, cg=20, ph=1 if p != 36 else 0, pw=1 if p != 36 else 0, tag="-cg20") for p in (32, 33, 34, 35, 36)] + \
              [_dg(p, 7, 21, cout=72 if DG_CO_TILE[p] == 64 else 8, tag="-cout") for p in (32, 33, 34, 35, 36)]
# c. the epilogue
DG_EPI = [_dg(p, 7, 21, act=ACT_RELU, add=a, ph=1, pw=0) for p in (32, 33, 34, 35) for a in ("none", "sep")] + \
         [_dg(36, 7, 21, act=ACT_RELU), _dg(36, 7, 21, act=ACT_RELU, add="sep", scale=0.1)] + \
         [_dg(p, 7, 21, act=ACT_TANH, scale=0.1, add=a) for p, a in ((32, "none"), (35, "sep"), (36, "none"), (34, "alias"))] + \
         [_dg(32, 7, 21, split=16, add="sep"), _dg(34, 7, 21, split=64, add="sep", scale=0.1), _dg(35, 7, 21, split=4),
          _dg(33, 7, 21, split=12, add="alias"),
          # the ConvGRU's two calls (_GruFn.backward): convq's adjoint into d(rh) and dx, then
          # [convz; convr]'s added into dh and dx in place
          _dg(36, 17, 39, B=1, cg=128, cout=256, split=128, tag="-convq"),
          _dg(36, 17, 39, B=1, cg=256, cout=256, split=128, add="alias", tag="-convzr")]
DG_CASES = DG_A + DG_BAND + DG_SHAPES + DG_CHANNELS + DG_EPI
DG_BY_ID = {c["id"]: c for c in DG_CASES}
assert len(DG_BY_ID) == len(DG_CASES)


def _gw(name, stride, B, Cs, c0, c1, small, large=None, bfl=False, scale=1.0, edges=()):
    return dict(id=name, stride=stride, B=B, Cs=Cs, c0=c0, c1=c1, Hs=small[0], Ws=small[1],
                Hl=(large or small)[0], Wl=(large or small)[1], bfl=bfl, scale=scale, edges=set(edges))


# d. the f32 weight gradient: every tiling x (one pixel, k4 = 4 with a padded pixel, one full band,
# two bands 33 | 32, three bands 44 | 44 | 42) and the slice edges; the large size of a stride-2
# case from {2 Hs, 2 Hs - 1, 2 Hs - 7} x {2 Ws, 2 Ws - 1, 2 Ws - 7}
GW_CASES = [
    _gw("s1-40-32+16-1x1-units1", 1, 1, 40, 32, 16, (1, 1), edges=["tiling1222", "units1", "padded_kstep"]),
    _gw("s1-24-16+24-7x3-ups1", 1, 2, 24, 16, 24, (7, 3), scale=0.1, edges=["tiling1222", "ups1", "padded_kstep"]),
    _gw("s1-128-128+128-3x13-ups1", 1, 2, 128, 128, 128, (3, 13), edges=["tiling1222", "ups1", "padded_kstep"]),
    _gw("s1-40-32+16-4x64-full-band", 1, 1, 40, 32, 16, (4, 64), edges=["tiling1222", "bands1"]),
    _gw("s1-40-32+16-3x65-two-bands", 1, 2, 40, 32, 16, (3, 65), scale=0.1, edges=["tiling1222", "bands2", "padded_kstep"]),
    _gw("s1-24-16+24-2x130-three-bands", 1, 1, 24, 16, 24, (2, 130), edges=["tiling1222", "bands3", "padded_kstep"]),
    _gw("s1-24-16+24-43x3-last-slice-short", 1, 7, 24, 16, 24, (43, 3), edges=["tiling1222", "last_slice_short"]),
    _gw("s2-24-40-13x18-odd", 2, 2, 24, 40, 0, (13, 18), (25, 35), edges=["tiling2222", "ups1", "padded_kstep"]),
    _gw("s2-72-17-1x65-two-bands", 2, 2, 72, 17, 0, (1, 65), (2, 130), scale=0.1, edges=["tiling2222", "bands2"]),
    _gw("s2-24-40-5x130-three-bands-crop7", 2, 1, 24, 40, 0, (5, 130), (3, 253), bfl=True, edges=["tiling2222", "bands3"]),
    _gw("s2-72-17-7x3", 2, 2, 72, 17, 0, (7, 3), (14, 5), scale=0.1, edges=["tiling2222", "padded_kstep"]),
    _gw("s2-24-40-4x64-full-band", 2, 1, 24, 40, 0, (4, 64), (8, 127), edges=["tiling2222", "bands1"]),
    _gw("s2-72-17-1x1-units1", 2, 1, 72, 17, 0, (1, 1), (2, 2), edges=["tiling2222", "units1"]),
    _gw("s2-24-40-257x3-last-slice-short", 2, 1, 24, 40, 0, (257, 3), (514, 6), edges=["tiling2222", "last_slice_short"]),
    _gw("s2-40-16-13x18", 2, 2, 40, 16, 0, (13, 18), (26, 36), edges=["tiling2241", "ups1"]),
    _gw("s2-17-9-4x64-full-band-crop7", 2, 2, 17, 9, 0, (4, 64), (1, 121), bfl=True, edges=["tiling2241", "bands1"]),
    _gw("s2-40-16-3x65-two-bands", 2, 2, 40, 16, 0, (3, 65), (5, 129), edges=["tiling2241", "bands2"]),
    _gw("s2-17-9-1x1-units1", 2, 1, 17, 9, 0, (1, 1), (1, 1), edges=["tiling2241", "units1"]),
    _gw("s2-40-16-2x130-three-bands", 2, 1, 40, 16, 0, (2, 130), (4, 260), edges=["tiling2241", "bands3"]),
    _gw("s2-17-9-5x3", 2, 2, 17, 9, 0, (5, 3), (9, 6), scale=0.1, edges=["tiling2241", "padded_kstep"]),
    _gw("s2-40-16-171x3-last-slice-short", 2, 3, 40, 16, 0, (171, 3), (342, 5), edges=["tiling2241", "last_slice_short"]),
    _gw("s2-16-1-13x18", 2, 2, 16, 1, 0, (13, 18), (25, 36), edges=["tiling2111", "ups1"]),
    _gw("s2-16-9-9x65-two-bands-crop7", 2, 2, 16, 9, 0, (9, 65), (18, 123), scale=0.1, edges=["tiling2111", "bands2"]),
    _gw("s2-16-8-28x36-bias-large-nsb1", 2, 2, 16, 8, 0, (28, 36), (49, 65), bfl=True, edges=["tiling2111", "ups1"]),
    _gw("s2-8-16-3x130-three-bands", 2, 1, 8, 16, 0, (3, 130), (6, 259), edges=["tiling2111", "bands3"]),
    _gw("s2-16-9-1x1-units1", 2, 1, 16, 9, 0, (1, 1), (2, 1), edges=["tiling2111", "units1"]),
    _gw("s2-16-1-4x64-full-band", 2, 1, 16, 1, 0, (4, 64), (8, 128), edges=["tiling2111", "bands1"]),
    _gw("s2-8-16-1x3", 2, 2, 8, 16, 0, (1, 3), (2, 6), edges=["tiling2111", "padded_kstep"]),
    _gw("s2-16-1-171x1-last-slice-short", 2, 3, 16, 1, 0, (171, 1), (342, 2), edges=["tiling2111", "last_slice_short"]),
    _gw("s2-16-8-48x48-bias-small-nsb2", 2, 2, 16, 8, 0, (48, 48), (96, 96), edges=["tiling2111", "nsb>1"]),
    _gw("s2-16-8-48x48-bias-large-nsb2", 2, 2, 16, 8, 0, (48, 48), (96, 96), bfl=True, edges=["tiling2111", "nsb>1"]),
]
GW_BY_ID = {c["id"]: c for c in GW_CASES}
assert len(GW_BY_ID) == len(GW_CASES)


def gw_plan_of(case):
    return gw_plan(case["stride"], case["Cs"], case["c0"] + case["c1"], case["B"], case["Hs"], case["Ws"], case["Hl"], case["Wl"])


# e. the gate derivatives.  stage 0 in GruConvs._act_backward's calling form (B = hc = H = 1)
GATE_CASES = [dict(id="gates-stage1-3x128x5x7", stage=1, B=3, hc=128, H=5, W=7, act=ACT_NONE),
              dict(id="gates-stage2-3x128x5x7", stage=2, B=3, hc=128, H=5, W=7, act=ACT_NONE),
              dict(id="gates-stage0-relu", stage=0, B=1, hc=1, H=1, W=3 * 37 * 11, act=ACT_RELU),
              dict(id="gates-stage0-tanh", stage=0, B=1, hc=1, H=1, W=3 * 37 * 11, act=ACT_TANH),
              dict(id="gates-stage0-none", stage=0, B=1, hc=1, H=1, W=3 * 37 * 11, act=ACT_NONE)]
GATE_BY_ID = {c["id"]: c for c in GATE_CASES}

# The compact batches of tests/test_gpu_big_offsets.py (3 items, hc = 128, 8 x 8): by id only, so that
# the operand, reference and bar functions below serve them; the per-element tests above keep their lists.
BIG_GATES = dict(id="gates-big-3x128x8x8", stage=2, B=3, hc=128, H=8, W=8, act=ACT_NONE)
BIG_DG_Q = _dg(36, 8, 8, B=3, cg=128, cout=256, split=128, tag="-big-convq")
BIG_DG_ZR = _dg(36, 8, 8, B=3, cg=256, cout=256, split=128, add="alias", tag="-big-convzr")
GATE_BY_ID[BIG_GATES["id"]] = BIG_GATES
DG_BY_ID[BIG_DG_Q["id"]] = BIG_DG_Q
DG_BY_ID[BIG_DG_ZR["id"]] = BIG_DG_ZR

RELU_PLANTS = (0.0, -0.0, 2.0 ** -126, -1.5, -(2.0 ** -126), -0.0)
TANH_PLANTS = (1.0, -1.0, 1.0 - 2.0 ** -24, -(1.0 - 2.0 ** -24), 1.0 - 2.0 ** -23, -(1.0 - 3 * 2.0 ** -24))


def plant(t, values):
    """The special values at the first elements and the last one of t (in place)."""
    f = t.view(-1)
    assert f.numel() > len(values)
    f[:len(values)] = torch.tensor(values, dtype=t.dtype)
    f[-1] = values[1]
    return t


# ---------------------------------------------------------------------------- data gradient
@functools.lru_cache(maxsize=None)
def dgrad_operands(cid):
    """The f32 operands of a case: g (B, cg, Hg, Wg); w, the forward layer's own weight tensor
    ((cg, cout, 3, 3): the conv's (out, in) for the T2 / S1 adjoints; (cout, cg, 3, 3): the
    transposed conv's (in, out) for the S2 adjoints); ysave / add (B, cout, Ho, Wo) or None."""
    c = DG_BY_ID[cid]
    gen = torch.Generator().manual_seed(_seed(cid))
    g = torch.randn((c["B"], c["cg"], c["Hg"], c["Wg"]), generator=gen)
    wshape = (c["cout"], c["cg"], 3, 3) if c["mode"] == S2 else (c["cg"], c["cout"], 3, 3)
    w = torch.randn(wshape, generator=gen) / math.sqrt(4.0 * c["cg"])
    oshape = (c["B"], c["cout"], c["Ho"], c["Wo"])
    ysave = add = None
    if c["act"] == ACT_RELU:
        ysave = plant(torch.relu(torch.randn(oshape, generator=gen)), RELU_PLANTS)
    elif c["act"] == ACT_TANH:
        ysave = plant(torch.tanh(2.0 * torch.randn(oshape, generator=gen)), TANH_PLANTS)
    if c["add"] != "none":
        add = torch.randn(oshape, generator=gen)
    return dict(g=g, w=w, ysave=ysave, add=add)


def dgrad_linear(c, g, w):
    """The adjoint alone: the gradient with respect to x (B, cout, Ho, Wo) of the forward layer
    under the upstream gradient g, in g's dtype."""
    x = torch.zeros((c["B"], c["cout"], c["Ho"], c["Wo"]), dtype=g.dtype, requires_grad=True)
    if c["mode"] == T2:    # the adjoint of a stride-2 conv
        y = F.conv2d(x, w, stride=2, padding=1)
    elif c["mode"] == S2:  # of a transposed conv whose output is stored cropped
        y = F.conv_transpose2d(x, w, stride=2, padding=1, output_padding=1)[..., :c["Hg"], :c["Wg"]]
    else:
        y = F.conv2d(x, w, padding=1)
    assert y.shape == g.shape, (c["id"], y.shape, g.shape)
    return torch.autograd.grad(y, x, g)[0]


def dact(ysave, act, dtype):
    if act == ACT_RELU:
        return (ysave > 0).to(dtype)
    y = ysave.to(dtype)
    return 1 - y * y


def dgrad_apply(c, lin, ysave, add, dtype):
    """* scale * act'(ysave) + add, in dtype and in the kernel's order."""
    u = lin * torch.tensor(c["scale"], dtype=torch.float32).to(dtype)
    if c["act"] == ACT_RELU:
        u = torch.where(ysave > 0, u, torch.zeros((), dtype=dtype))
    elif c["act"] == ACT_TANH:
        u = u * dact(ysave, ACT_TANH, dtype)
    if add is not None:
        u = u + add.to(dtype)
    return u


def dgrad_terms(c):
    """n of every output element (a number, or (Ho, Wo) by output phase)."""
    if c["mode"] != T2:
        return 9 * c["cg"]
    return c["cg"] * (1 + torch.arange(c["Ho"])[:, None] % 2) * (1 + torch.arange(c["Wo"])[None, :] % 2)


@functools.lru_cache(maxsize=None)
def dgrad_reference(cid, perturb=None):
    """ref, X, c and e per element of a case (float64, (B, cout, Ho, Wo))."""
    c = DG_BY_ID[cid]
    o = dgrad_operands(cid)
    g, w, add = o["g"].double(), o["w"].double(), o["add"]
    if perturb == "nonneg":    # (every term non-negative: the bound is the gradient)
        g, w, add = g.abs(), w.abs(), None if add is None else add.abs()
    if perturb == "flip_tap":  # (shows the test can fail: one tap of the adjoint moved)
        w = w.clone()
        w[0, 0, 0, 0], w[0, 0, 2, 2] = w[0, 0, 2, 2].clone(), w[0, 0, 0, 0].clone()
    lin, xlin = dgrad_linear(c, g, w), dgrad_linear(c, g.abs(), w.abs())
    scale = float(torch.tensor(c["scale"], dtype=torch.float32))
    ref = dgrad_apply(c, lin, o["ysave"], add, torch.float64)
    X = abs(scale) * xlin
    if c["act"] != ACT_NONE:
        X = X * dact(o["ysave"], c["act"], torch.float64).abs()
    if add is not None:
        X = X + add.double().abs()
    n = dgrad_terms(c)
    cc = torch.clamp(torch.as_tensor((n + 4) * U, dtype=torch.float64), max=C_MFMA)
    e = 3 * U * abs(scale) * xlin if c["act"] == ACT_TANH else torch.zeros(())
    return dict(ref=ref, X=X, c=cc, e=e, xlin=xlin)


def dgrad_float32(cid):
    c = DG_BY_ID[cid]
    o = dgrad_operands(cid)
    return dgrad_apply(c, dgrad_linear(c, o["g"], o["w"]), o["ysave"], o["add"], torch.float32)


# ---------------------------------------------------------------------------- weight / bias gradient
def wgrad_reference(stride, s, l, dtype=torch.float64):
    """dW and sum |s| |l| per element of the correlation (l zero outside its stored size), in dtype."""
    s, l = s.to(dtype), l.to(dtype)
    B, Cs, Hs, Ws = s.shape
    Hl, Wl = l.shape[2:]
    R, Cw = stride * (Hs - 1) + 3, stride * (Ws - 1) + 3
    lp = F.pad(l, (1, Cw - 1 - Wl, 1, R - 1 - Hl))
    dw = torch.zeros((Cs, l.shape[1], 3, 3), dtype=dtype)
    mag = torch.zeros_like(dw)
    for ky in range(3):
        for kx in range(3):
            lw = lp[:, :, ky:ky + stride * (Hs - 1) + 1:stride, kx:kx + stride * (Ws - 1) + 1:stride]
            dw[:, :, ky, kx] = torch.einsum("bshw,blhw->sl", s, lw)
            mag[:, :, ky, kx] = torch.einsum("bshw,blhw->sl", s.abs(), lw.abs())
    return dw, mag


@functools.lru_cache(maxsize=None)
def wgrad_operands(cid):
    c = GW_BY_ID[cid]
    gen = torch.Generator().manual_seed(_seed(cid))
    s = torch.randn((c["B"], c["Cs"], c["Hs"], c["Ws"]), generator=gen)
    l = torch.relu(torch.randn((c["B"], c["c0"] + c["c1"], c["Hl"], c["Wl"]), generator=gen) + 0.5)
    if c["bfl"]:  # (the large tensor is then the output gradient: signed)
        l = torch.randn(l.shape, generator=gen)
    return s, l


@functools.lru_cache(maxsize=None)
def wgrad_case_reference(cid, perturb=None):
    """dW: ref, X, c (Cs, Cl, 3, 3); db: ref, X, c per channel.  float64, scale included."""
    c = GW_BY_ID[cid]
    s, l = wgrad_operands(cid)
    p = gw_plan_of(c)
    scale = float(torch.tensor(c["scale"], dtype=torch.float32))
    if perturb == "skip_last_slice":  # (shows the test can fail: the last K slice's units left out)
        first = (p["nsl"] - 1) * p["ups"]  # unit = (image * Hs + row) * nbands + band
        s = s.clone()
        for u in range(first, p["units"]):
            row, band = divmod(u, p["nbands"])
            s[row // c["Hs"], :, row % c["Hs"], band * p["bw"]:(band + 1) * p["bw"]] = 0
    dw, mag = wgrad_reference(c["stride"], s, l)
    cnt = wgrad_reference(c["stride"], torch.ones_like(s[:, :1]), torch.ones_like(l[:, :1]))[0]  # in-range terms per tap
    cw = torch.clamp((cnt + p["nsl"] + 2) * U, max=C_MFMA).expand_as(dw)
    gsrc = l if c["bfl"] else s
    db = gsrc.double().sum((0, 2, 3))
    nb = gsrc.shape[0] * gsrc.shape[2] * gsrc.shape[3]
    return dict(dw=scale * dw, Xw=abs(scale) * mag, cw=cw, db=db, Xb=gsrc.double().abs().sum((0, 2, 3)),
                cb=min(C_MFMA, (nb + p["nsb"] + 2) * U))


def wgrad_float32(cid):
    c = GW_BY_ID[cid]
    s, l = wgrad_operands(cid)
    dw = wgrad_reference(c["stride"], s, l, torch.float32)[0] * torch.tensor(c["scale"], dtype=torch.float32)
    return dw, (l if c["bfl"] else s).sum((0, 2, 3))


# ---------------------------------------------------------------------------- gate derivatives
@functools.lru_cache(maxsize=None)
def gate_operands(cid):
    c = GATE_BY_ID[cid]
    gen = torch.Generator().manual_seed(_seed(cid))
    shape = (c["B"], c["hc"], c["H"], c["W"])
    r = lambda: torch.randn(shape, generator=gen)  # noqa: E731
    if c["stage"] == 0:
        y = torch.relu(r()) if c["act"] == ACT_RELU else torch.tanh(2.0 * r())
        plant(y, RELU_PLANTS if c["act"] == ACT_RELU else TANH_PLANTS)
        return dict(dhn=r(), z=y)
    # The gates are drawn where a correct float32 evaluation stays within a quarter of C_GATES
    # (the condition of tests/test_gconv_bwd_cpu.py).  Its worst case over X, one unit roundoff
    # 2^-24 per rounding: du_q (3 - 2 q^2) / (1 + q^2), du_z 5 (1 - z) / (1 + z), du_r
    # 4 (1 - r) / (1 + r); within 2 for |q| >= 1/2, z >= 3/7, r >= 1/3.  Gates drawn as
    # sigmoid / tanh of N(0, 1) reach 2.1 .. 2.4 at every seed (q near 0, small z, small r).
    u = lambda lo, hi: lo + (hi - lo) * torch.rand(shape, generator=gen)  # noqa: E731
    o = dict(dhn=r(), drh=r(), z=u(0.45, 1.0), r=u(0.35, 1.0), q=u(0.5, 1.0) * torch.sign(r()), h=torch.tanh(r()))
    # planted in the LAST image (b > 0: the e + b chw index): exact 0 and 1 gates, q = +-1, q = h, r = 1/2
    for k, vals in (("z", (0.0, 1.0)), ("r", (0.0, 1.0, 0.5)), ("q", (1.0, -1.0))):
        o[k][-1].view(-1)[:len(vals)] = torch.tensor(vals)
    o["q"][-1].view(-1)[5:9] = o["h"][-1].view(-1)[5:9]
    return o


def gate_formulas(cid, dtype, stage=None):
    """name -> (value, X) of the outputs of the case's stage (or of `stage` on the case's
    operands) evaluated in dtype (include/nlspn_prop.h)."""
    c = dict(GATE_BY_ID[cid])
    c["stage"] = c["stage"] if stage is None else stage
    o = {k: v.to(dtype) for k, v in gate_operands(cid).items()}
    g = o["dhn"]
    if c["stage"] == 0:
        y = o["z"]
        if c["act"] == ACT_RELU:
            return {"duq": (torch.where(y > 0, g, torch.zeros((), dtype=dtype)), torch.where(y > 0, g.abs(), torch.zeros((), dtype=dtype)))}
        if c["act"] == ACT_TANH:
            return {"duq": (g * (1 - y * y), g.abs() * (1 + y * y))}
        return {"duq": (g, g.abs())}
    z, h = o["z"], o["h"]
    if c["stage"] == 1:
        q = o["q"]
        return {"duq": (g * z * (1 - q * q), g.abs() * z * (1 + q * q)),
                "duz": (g * (q - h) * (z * (1 - z)), g.abs() * (q.abs() + h.abs()) * z * (1 + z))}
    d, r = o["drh"], o["r"]
    return {"dur": (d * h * (r * (1 - r)), d.abs() * h.abs() * r * (1 + r)),
            "dh": (g * (1 - z) + d * r, g.abs() * (1 + z) + d.abs() * r)}


# ---------------------------------------------------------------------------- the comparison
def ratio(got, ref, X, e=0.0):
    """The worst (|got - ref| - e) / X over all elements (NaN counts as infinite)."""
    err = (got.double() - ref).abs()
    return float(((err - e).clamp(min=0) / (X + 1e-300)).nan_to_num(nan=float("inf")).max())


def check(name, got, ref, X, c, e=0.0, record=None):
    """Every element: finite and |got - ref| <= c * X + e (numbers or tensors per element).
    Returns the worst (err - e) / X, recorded as gconv_bwd_elem/<name>."""
    got = got.detach().double().cpu()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    worst = ratio(got, ref, X, e)
    if record:
        record(f"gconv_bwd_elem/{name}", worst)
    ok = torch.isfinite(got) & ((got - ref).abs() <= c * X + e)
    if not bool(ok.all()):
        idx = (~ok).nonzero()
        raise AssertionError(f"{name}: {idx.shape[0]} of {ok.numel()} elements outside c = {float(torch.as_tensor(c).max()):g} "
                             f"(worst ratio {worst:.3g}, {int((~torch.isfinite(got)).sum())} not finite), "
                             f"first at {idx[:6].tolist()}")
    return worst


# ---------------------------------------------------------------------------- guarded device buffers
def guarded(t, dev, shrink_rows=0):
    """t on the device as a view into a NaN buffer, GUARD NaNs before and after it.
    shrink_rows (shows the test can fail): the last rows of the view are NaN too."""
    if t is None:
        return None
    n = t.numel()
    buf = torch.full((n + 2 * GUARD,), float("nan"), device=dev, dtype=torch.float32)
    v = buf[GUARD:GUARD + n].view(t.shape)
    v.copy_(t)
    if shrink_rows:
        v[-1, -1, -shrink_rows:] = float("nan")
    return v


def guarded_out(shape, dev, fill=None):
    """(buffer, view): the view pre-filled with NaN (or with `fill`, a CPU tensor) between two
    runs of GUARD sentinels."""
    n = math.prod(shape)
    buf = torch.full((n + 2 * GUARD,), SENT, device=dev, dtype=torch.float32)
    v = buf[GUARD:GUARD + n].view(*shape)
    if fill is None:
        v.fill_(float("nan"))
    else:
        v.copy_(fill)
    return buf, v


def guards_intact(buf):
    return bool((buf[:GUARD] == SENT).all()) and bool((buf[-GUARD:] == SENT).all())
