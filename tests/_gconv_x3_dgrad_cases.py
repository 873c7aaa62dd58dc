"""Cases, references and bars of the per-element tests of the split-bf16 data gradients
(nlspn_gconv_x3_dgrad, the NLSPN_GCX3_DG_* presets of csrc/nlspn_gconv_plan.h), shared by
tests/test_gconv_x3_dgrad_cpu.py (CPU) and tests/test_gpu_gconv_x3_dgrad.py (GPU).  Built on
tests/_gconv_bwd_cases.py: the seeded operands, the float64 adjoint (torch.autograd.grad of the
FORWARD operation, never the packing helpers) and the guarded buffers are that module's; the
cases of this table are entered into its DG_BY_ID by id, as its own BIG_* cases are, so that its
operand and reference functions serve them.

Per case three things, all float64 per element:
    unsplit     act'(ysave) * scale * sum w g (+ add) on the f32 operands: bc.dgrad_reference
    emulation   the same with the three products the kernel forms of the very operands passed,
                sum (w_hi g_hi + w_hi g_lo + w_lo g_hi), hi / lo = split_bf16 of each operand;
                by linearity adjoint(g_hi + g_lo; w_hi) + adjoint(g_hi; w_lo)
    X           |scale| |act'(ysave)| sum |w||g| + |add|

Bars.  The split itself (CPU, every element): |emulation - unsplit| <= 2^-15 X, the contract of
include/nlspn_prop.h (|a - hi - lo| <= 2^-17 |a| per operand, the dropped lo lo <= 2^-16 |w g|).
The kernel against the emulation (GPU): |got - emulation| <= c X + e with
c = min(2e-6, (3 n + 4) 2^-24), n the element's (channel, tap) terms, three products each (the x3
forward's bar, tests/test_gpu_gconv_x3_fwd.py, with the data gradient's + 4 of
tests/_gconv_bwd_cases.py); Tanh adds e = 3 * 2^-24 |scale| sum |w||g|.  Against the unsplit
float64 reference the bar is c X + e + 2^-15 X.  None is derived from the kernels under test.

Edge claims: `edges` names what a case's grid does under gc_tile; the CPU test checks every claim
against the launcher's own function (tests/gconv_x3_dg_plan_check.cpp, `tile`).
"""
import functools

import torch

import _gconv_bwd_cases as bc
from nlspn_eccv20_amd.gru import split_bf16

DG_T2, DG_T2_C16, DG_S2, DG_S1 = 80, 81, 82, 83
PRESETS = (DG_T2, DG_T2_C16, DG_S2, DG_S1)
NAMES = {DG_T2: "DG_T2", DG_T2_C16: "DG_T2_C16", DG_S2: "DG_S2", DG_S1: "DG_S1"}
MODE = {DG_T2: bc.T2, DG_T2_C16: bc.T2, DG_S2: bc.S2, DG_S1: bc.S1}
XP = {DG_T2: 40, DG_T2_C16: 80, DG_S2: 40, DG_S1: 40}   # the window pitch: gc_bwmax below
CO_TILE = {DG_T2: 64, DG_T2_C16: 16, DG_S2: 64, DG_S1: 64}
# (cg, cout): three 16-channel chunks in (both LDS stages and the odd last trip), one co tile out
CH = {DG_T2: (48, 64), DG_T2_C16: (48, 16), DG_S2: (48, 64), DG_S1: (48, 64)}
BWMAX = {p: bc.gc_bwmax(MODE[p], XP[p]) for p in PRESETS}
assert BWMAX == {DG_S1: 38, DG_S2: 19, DG_T2: 39, DG_T2_C16: 79}
SPLIT_BOUND = 2.0 ** -15


def _dg(preset, gh, gw, B=2, cg=None, cout=None, ph=0, pw=0, act=bc.ACT_NONE, scale=1.0, split=None, add="none",
        edges=(), tag="", dxs=False):
    """A case on the tiled grid gh x gw (bc._dg's fields).  ph / pw: rows / columns the output is
    short of twice the grid (T2 only: a stride-2-mode gradient stored cropped is not served)."""
    mode = MODE[preset]
    cg, cout = cg or CH[preset][0], cout or CH[preset][1]
    assert not (ph or pw) or mode == bc.T2
    if mode == bc.T2:
        Hg, Wg, Ho, Wo = gh, gw, 2 * gh - ph, 2 * gw - pw
    elif mode == bc.S2:
        Hg, Wg, Ho, Wo = 2 * gh, 2 * gw, gh, gw
    else:
        Hg, Wg, Ho, Wo = gh, gw, gh, gw
    cid = f"x3dg{preset}-{B}x{cg}>{cout}-{gh}x{gw}" + (f"-off{ph}.{pw}" if ph or pw else "") + \
        ("-relu" if act == bc.ACT_RELU else "-tanh" if act == bc.ACT_TANH else "") + (f"-scale{scale:g}" if scale != 1.0 else "") + \
        (f"-split{split}" if split else "") + (f"-add.{add}" if add != "none" else "") + ("-dxs" if dxs else "") + tag
    return dict(id=cid, preset=preset, mode=mode, B=B, cg=cg, cout=cout, gh=gh, gw=gw, Hg=Hg, Wg=Wg, Ho=Ho, Wo=Wo,
                act=act, scale=scale, split=split or cout, add=add, edges=set(edges), dxs=dxs)


# one full band, one pixel more, the tile shrunk to one pixel: every preset
BAND = [c for p in PRESETS for c in (_dg(p, 5, BWMAX[p], edges=["full_band"]), _dg(p, 5, BWMAX[p] + 1, edges=["band_plus_one"]),
                                     _dg(p, 1, 1, edges=["npx_shrunk"]))]
# 17 x 39 and 3 x 43 under the 64-channel transposed and the stride-2 tilings.  Under DG_T2 (39-wide
# bands) 17 x 39 is one full band in several tiles and 3 x 43 two bands 22 | 21 whose last band's 63
# pixels leave its second tile empty; under DG_S2 (19-wide bands) 17 x 39 is three even bands with
# the tile cut to the window rows and 3 x 43 three bands 15 | 15 | 13.  An empty tile under DG_S2's
# geometry: 4 x 33 (17 | 16), the grid tests/_gconv_bwd_cases.py uses for the same geometry.
GRIDS = [_dg(DG_T2, 17, 39, edges=["full_band", "tiles>1"]), _dg(DG_T2, 3, 43, edges=["uneven_last_band", "empty_tile"]),
         _dg(DG_S2, 17, 39, edges=["npx_shrunk", "tiles>1"]), _dg(DG_S2, 3, 43, edges=["uneven_last_band"]),
         _dg(DG_S2, 4, 33, edges=["uneven_last_band", "empty_tile"])]
# gradient channels no multiple of the 16-channel chunk; a partial co tile
CHANNELS = [_dg(p, 7, 21, cg=20, tag="-cg20") for p in PRESETS] + \
           [_dg(p, 7, 21, cout=72 if CO_TILE[p] == 64 else 8, tag="-cout", edges=["partial_co_tile"]) for p in PRESETS]
# the transposed adjoints' output one row and / or one column short
CROP = [_dg(p, 6, 41, ph=ph, pw=pw) for p in (DG_T2, DG_T2_C16) for ph, pw in ((0, 1), (1, 0), (1, 1))]
# the epilogue: ReLU and Tanh on the saved output, scale 0.25, no addend / a separate one
EPI = [_dg(p, 7, 21, act=act, scale=0.25, add=a, ph=1 if p != DG_S2 else 0)
       for p in (DG_T2, DG_T2_C16, DG_S2) for act in (bc.ACT_RELU, bc.ACT_TANH) for a in ("none", "sep")]
# the ConvGRU's two calls (_GruFn.backward): convq's adjoint into d(rh) and dx, then [convz; convr]'s
# added into dh and dx in place
GRU = [_dg(DG_S1, 8, 8, B=3, cg=128, cout=256, split=128, tag="-convq"),
       _dg(DG_S1, 8, 8, B=3, cg=256, cout=256, split=128, add="alias", tag="-convzr")]
# the split copy of the output beside the f32 one (a partial last 8-channel block: cout 20)
DXS = [_dg(DG_T2, 7, 21, dxs=True), _dg(DG_S2, 7, 21, dxs=True), _dg(DG_T2, 7, 21, cout=20, ph=1, pw=1, dxs=True),
       _dg(DG_S2, 7, 21, act=bc.ACT_RELU, add="sep", dxs=True)]
CASES = BAND + GRIDS + CHANNELS + CROP + EPI + GRU + DXS
BY_ID = {c["id"]: c for c in CASES}
assert len(BY_ID) == len(CASES)
assert not set(BY_ID) & set(bc.DG_BY_ID)
bc.DG_BY_ID.update(BY_ID)   # (by id only: bc.dgrad_operands / dgrad_reference then serve these cases)


def edges_of(case, t):
    """The edges a case's grid hits, from what gc_tile planned (t: the `tile` report of
    tests/gconv_x3_dg_plan_check.cpp)."""
    e = set()
    if t["nbands"] > 1 and t["bwl"] < t["bw"]:
        e.add("uneven_last_band")
    if t["empty_last"]:
        e.add("empty_tile")
    if case["gw"] == t["bwmax"]:
        e.add("full_band")
    if case["gw"] == t["bwmax"] + 1 and t["nbands"] == 2:
        e.add("band_plus_one")
    if t["npx"] < t["npx_full"]:
        e.add("npx_shrunk")
    if t["tpb"] > 1:
        e.add("tiles>1")
    if case["cout"] % t["wgco"] != 0:
        e.add("partial_co_tile")
    return e


def split_f64(x):
    """(hi, lo) of split_bf16 as float64."""
    hi, lo = split_bf16(x)
    return hi.double(), lo.double()


@functools.lru_cache(maxsize=None)
def reference(cid):
    """Per element (float64, (B, cout, Ho, Wo)): ref (unsplit), emu (the three split products),
    X, the kernel's bar c and e, and the term count's bound on the split."""
    c = BY_ID[cid]
    o = bc.dgrad_operands(cid)
    R = bc.dgrad_reference(cid)
    ghi, glo = split_f64(o["g"])
    whi, wlo = split_f64(o["w"])
    lin = bc.dgrad_linear(c, ghi + glo, whi) + bc.dgrad_linear(c, ghi, wlo)
    emu = bc.dgrad_apply(c, lin, o["ysave"], o["add"], torch.float64)
    n = bc.dgrad_terms(c)
    cc = torch.clamp(torch.as_tensor((3 * n + 4) * bc.U, dtype=torch.float64), max=bc.C_MFMA)
    return dict(ref=R["ref"], emu=emu, X=R["X"], c=cc, e=R["e"])
