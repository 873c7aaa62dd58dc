"""GRU-mode convolutions on the HIP kernels (the reference's forced
default mode, src/config.py:225-228).

One GRU-mode iteration of the reference (src/model/nlspnmodel.py:365-373) runs, per
iteration after the first,
    dep_feat = encode_dep(new_pred / max_depth)          (:366, modules :134-138)
    aff_feat = encode_aff(aff)            (first update)   (:368-369, :127-132)
    aff_feat = GRU(h=aff_feat, x=dep_feat)               (:371, ConvGRU :386-403)
    aff      = _aff_head(aff_feat)                       (:373, decode_aff :140-143 + _clip_as)
``GruConvs`` runs every one of those convolutions as ``nlspn_gconv`` launches
(``csrc/nlspn_gconv.h``): f32-input MFMA implicit GEMMs reading NCHW in place, bias and
ReLU / Tanh / the GRU's sigmoid-tanh-blend in their epilogues, the crop written directly —
9 launches per iteration where the module path issues ~40 (convolutions, bias adds, ReLUs,
cats, sigmoids, tanh, blends, layout copies), the last one also normalising the affinity
(``nlspn_gconv_affnorm``: no separate normalisation launch).  The 1- / 9-channel first encoder convs run on a
VALU kernel (as MFMA tiles their K would be mostly padding).  Numerics: exact f32 products and f32
accumulation; only the summation order differs from MIOpen's (RMSE vs the reference's
GRU-mode fixtures well inside their 1e-4 bar, tests/test_gpu_gru.py).

Training runs on the same kernels.  With gradients enabled every layer chain and the ConvGRU
cell is a ``torch.autograd.Function`` (``_ChainFn``, ``_GruFn``) taking the modules' own
``weight`` / ``bias`` parameters, whose backward issues (``csrc/nlspn_gconv_bwd.h``):
  * data gradients as forward launches of the ADJOINT layer kind on adjoint-packed weights
    (a stride-2 conv's adjoint is the transposed conv of the same tensor and vice versa; a
    stride-1 conv's is the conv with flipped taps and transposed channels), whose epilogue
    multiplies by the activation derivative of the layer below (from its saved output), so
    every launch hands the next one a pre-activation gradient;
  * weight / bias gradients as an MFMA implicit GEMM over pixels, split over workgroups into
    f32 slabs that a second launch sums in a fixed order (no atomics: bit-reproducible);
  * the ConvGRU's gate derivatives as two pointwise launches around the candidate's data
    gradient; the training forward is the inference launches plus stores of r and q.
The forward values are those of the inference launches, bit for bit.  Under gradients
``decode_aff`` returns the raw taps (the differentiable ``affinity_normalization`` follows).

Weights are packed once per weight version into the kernels' layout and cached
(``GruConvs.pack``), the adjoint packs beside the forward ones on the first call under
gradients.  ``GruConvs.stats`` counts the launches per kind.

Opt-in at inference (``NLSPNModel.gru_precision = "fp16"``) the same layers run on the f16
matrix cores (``nlspn_gconv16``, ``csrc/nlspn_gconv16.h``): half operands (weights rounded once
when packed by ``pack_conv16`` / ``pack_convt16``, activations once in the epilogue that produces
them), f32 accumulation and epilogues, the ConvGRU state carried in f32 beside an f16 copy,
activations between the layers in the ``c8`` layout (``to_c8`` / ``from_c8``: tests and
boundaries only).  ``encode_dep16`` / ``encode_aff16`` / ``gru16`` / ``decode_aff16`` are the
variants; the f16 packs live in the f32 packs' cache entry (``pack16``), ``stats["fwd16"]``
counts their launches.  The last decoder layer stays the f32 ``nlspn_gconv_affnorm``.

``gru_precision = "bf16x3"`` runs them on the bf16 matrix cores instead, with f32-class operands
(``nlspn_gconv_x3``, ``csrc/nlspn_gconv_x3.h``): every f32 operand is the pair ``hi = bf16(a)``,
``lo = bf16(a - hi)`` (``split_bf16``) and the kernels accumulate ``w_hi x_hi + w_hi x_lo +
w_lo x_hi`` in f32.  Weights are split once when packed (``pack_conv_x3`` / ``pack_convt_x3``),
activations once in the epilogue that produces them; between the layers they travel in the
``c8x2`` layout (``to_c8x2`` / ``from_c8x2``: tests and boundaries only).  ``encode_dep_x3`` /
``encode_aff_x3`` / ``gru_x3`` / ``decode_aff_x3`` mirror the f16 methods, the packs live in the
same cache entry (``pack_x3``) and ``stats["fwd_x3"]`` counts the launches.

Opt-in under gradients (``GruConvs.wgrad_precision = "bf16x3"``, set through
``NLSPNModel.gru_wgrad_precision``) the weight gradients run on the bf16 matrix cores with each
f32 operand split into two bf16 parts (``nlspn_gconv_wgrad_bf16x3``, ``csrc/nlspn_gwgrad16.h``);
everything else of the backward is the same launches, and ``stats["wgrad_x3"]`` counts them.

Opt-in under gradients as well (``GruConvs.wgrad_narrow = True``, set through
``NLSPNModel.gru_wgrad_narrow``): the weight gradients of the stride-2 layers whose channel
counts are both <= 16 (1 / 9 -> 16 and 16 -> 8; ``nlspn_gconv_wgrad_narrow_covers``) take the
streaming kernel (``nlspn_gconv_wgrad_narrow``, ``csrc/nlspn_gwnarrow.h``: exact f32 products,
two launches per call, the bias gradient from the staged operand), whatever ``wgrad_precision``
is; every other layer keeps its entry and its bits.  ``stats["wgrad_narrow"]`` counts its launches.

Opt-in under gradients as well (``GruConvs.dgrad_precision = "bf16x3"``, set through
``NLSPNModel.gru_dgrad_precision``): the data gradients ``nlspn_gconv_x3_dgrad_covers`` accepts (the
wide layers' and both ConvGRU adjoints) run on the split-bf16 convolution kernels
(``nlspn_gconv_x3_dgrad``: the forward family's body with the derivative epilogue) on adjoint
weights packed split (``pack_adjoint_x3`` / ``pack_adjoint_s1_x3``, cached beside the f32 adjoint
packs when the mode first needs them).  A gradient is brought into ``c8x2`` where it enters a chain
in f32 (``nlspn_gconv_x3_split``) and handed on split from one data gradient to the next; every
other launch of the backward is unchanged.  ``stats["dgrad_x3"]`` / ``stats["split_x3"]`` count
the new launches, ``stats["dgrad"]`` keeps counting the f32 entry's.
"""
from __future__ import annotations

import ctypes
import functools
import typing

import torch
import torch.nn as nn

from . import _lib

__all__ = ["GruConvs", "pack_adjoint", "pack_adjoint_s1", "pack_adjoint_x3", "pack_adjoint_s1_x3", "unpack_conv", "unpack_convt", "to_c8", "from_c8",
           "pack_conv16", "pack_convt16", "unpack_conv16", "unpack_convt16", "split_bf16", "to_c8x2", "from_c8x2",
           "pack_conv_x3", "pack_convt_x3", "unpack_conv_x3", "unpack_convt_x3", "GC_S2", "GC_S2_C16", "GC_GRU1", "GC_GRU2", "GC_T2", "GC_T2_C16", "GC_S2_SMALL"]

GC_S2, GC_S2_C16, GC_GRU1, GC_GRU2, GC_T2, GC_T2_C16, GC_S2_SMALL = range(7)
# the data-gradient presets (NLSPN_GC_DG_*): the adjoint kind's tiling, derivative epilogue
GC_DG_T2, GC_DG_T2_C16, GC_DG_S2, GC_DG_S2_C16, GC_DG_S1 = range(32, 37)
# the f16-operand presets (NLSPN_GC16_*, csrc/nlspn_gconv16.h)
GC16_S2, GC16_GRU1, GC16_GRU2, GC16_T2, GC16_T2_C16, GC16_S2_SMALL = range(48, 54)
# the split-bf16 presets (NLSPN_GCX3_*, csrc/nlspn_gconv_x3.h)
GCX3_S2, GCX3_GRU1, GCX3_GRU2, GCX3_T2, GCX3_T2_C16, GCX3_S2_SMALL = range(64, 70)
# the split-bf16 data-gradient presets (NLSPN_GCX3_DG_*): the adjoint kind's x3 tiling, derivative epilogue
GCX3_DG_T2, GCX3_DG_T2_C16, GCX3_DG_S2, GCX3_DG_S1 = range(80, 84)
ACT_NONE, ACT_RELU, ACT_TANH = 0, 1, 2
# the transposed conv's taps per output phase (py, px), in the kernel's order
# (nlspn_gconv.h gc_tap): ky = 1 (py = 0) or 0, 2 (py = 1); likewise kx
_T_TAPS = [[(ky, kx) for ky in ((0, 2) if py else (1,)) for kx in ((0, 2) if px else (1,))]
           for py in (0, 1) for px in (0, 1)]


class _Family(typing.NamedTuple):
    """A preset family: the pack-layout query of the C ABI, the weight dtype and the inner
    channel block (the f32 kernels read [co_tile][cin_pad][tap][co]; the f16 ones the same with
    the input channels in blocks of 8 innermost, [co_tile][cin_pad/8][tap][co][8]), and its
    presets by layer kind (s2_c16 / t2_c16: at most 16 output channels; small: the VALU kernel).
    ``split``: every f32 weight goes in as two bf16 parts, per 8 input channels a hi block then
    a lo block ([co_tile][2 cin_pad / 8][tap][co][8]: the c8x2 layout's channel order).
    ``dg_query`` / ``dg``: the pack-layout query of the family's data-gradient presets ``dg``."""
    query: str
    dtype: torch.dtype
    block: int
    s2: int
    s2_c16: int
    t2: int
    t2_c16: int
    small: int
    gru1: int
    gru2: int
    split: bool = False
    dg_query: str = ""
    dg: tuple = ()


_F32 = _Family("nlspn_gconv_pack_layout", torch.float32, 1, GC_S2, GC_S2_C16, GC_T2, GC_T2_C16, GC_S2_SMALL, GC_GRU1, GC_GRU2)
# (the f16 stride-2 conv has one tiling for every width)
_F16 = _Family("nlspn_gconv16_pack_layout", torch.float16, 8, GC16_S2, GC16_S2, GC16_T2, GC16_T2_C16, GC16_S2_SMALL,
               GC16_GRU1, GC16_GRU2)
_X3 = _Family("nlspn_gconv_x3_pack_layout", torch.bfloat16, 8, GCX3_S2, GCX3_S2, GCX3_T2, GCX3_T2_C16, GCX3_S2_SMALL,
              GCX3_GRU1, GCX3_GRU2, split=True, dg_query="nlspn_gconv_x3_dgrad_pack_layout",
              dg=(GCX3_DG_T2, GCX3_DG_T2_C16, GCX3_DG_S2, GCX3_DG_S1))
_TAPS = [[(ky, kx) for ky in range(3) for kx in range(3)]]  # a conv: one part, all nine taps


def _layout_of(fam, layer):
    """(output-channel tile, input-channel chunk, transposed) of a preset of family ``fam``."""
    lib = _lib.get()  # a query: no device, no launch
    co, cc, tr = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    _lib.check(getattr(lib, fam.dg_query if layer in fam.dg else fam.query)(layer, ctypes.byref(co), ctypes.byref(cc), ctypes.byref(tr)))
    return co.value, cc.value, bool(tr.value)


def split_bf16(x: torch.Tensor):
    """(hi, lo) of an f32 tensor, both bfloat16: hi = x rounded to nearest-even, lo = the f32
    difference x - hi rounded to nearest-even.  |x - hi - lo| <= 2^-17 |x|."""
    x = x.float()
    hi = x.to(torch.bfloat16)
    return hi, (x - hi.float()).to(torch.bfloat16)


def _split_blocks(w):
    """(N, C, T) f32, C a multiple of 8 -> (N, 2 C, T) bf16: per 8-channel block its hi part, then its lo part."""
    N, C, T = w.shape
    hi, lo = split_bf16(w)
    return torch.stack([hi.reshape(N, C // 8, 8, T), lo.reshape(N, C // 8, 8, T)], 2).reshape(N, 2 * C, T)


def _pad_bias(bias, cout, n, device):
    b = torch.zeros(n, device=device, dtype=torch.float32)
    if bias is not None:
        b[:cout] = bias.detach().float()
    return b


def _pack(fam, transposed, weight, bias, layer):
    """The packed weights and padded f32 bias of a conv ((Cout, Cin, 3, 3)) or transposed conv
    ((Cin, Cout, 3, 3)) for a preset of family ``fam``: converted to the family's dtype first
    (half: one rounding to nearest-even; a split family: split_bf16, the hi and lo blocks
    interleaved), then per part (a conv: one; a transposed conv: its four output phases, one
    after another) [co_tile][cin_pad / block][tap][co][block]."""
    wgco, cc, tr = _layout_of(fam, layer)
    assert tr == transposed
    dtype, cb = (torch.float32 if fam.split else fam.dtype), fam.block
    wd = weight.detach().to(dtype)
    if transposed:
        wd = wd.transpose(0, 1)
    cout, cin = wd.shape[:2]
    ct = (cout + wgco - 1) // wgco
    cp = (cin + cc - 1) // cc * cc
    parts = []
    for taps in (_T_TAPS if transposed else _TAPS):
        w = torch.zeros((ct * wgco, cp, len(taps)), device=weight.device, dtype=dtype)
        for t, (ky, kx) in enumerate(taps):
            w[:cout, :cin, t] = wd[:, :, ky, kx]
        if fam.split:
            w = _split_blocks(w)
        parts.append(w.reshape(ct, wgco, w.shape[1] // cb, cb, len(taps)).permute(0, 2, 4, 1, 3).contiguous().reshape(-1))
    return torch.cat(parts), _pad_bias(bias, cout, ct * wgco, weight.device)


def _unpack(fam, transposed, w, cout, cin, layer):
    """Inverse of _pack: the module's (Cout, Cin, 3, 3) or (Cin, Cout, 3, 3) tensor, in w's dtype
    (a split family: hi + lo in f32)."""
    wgco, cc, _ = _layout_of(fam, layer)
    cb = fam.block
    ct, cp = (cout + wgco - 1) // wgco, (cin + cc - 1) // cc * cc
    cpk = 2 * cp if fam.split else cp  # the packed channels: a hi and a lo block per 8
    out = torch.zeros((cout, cin, 3, 3), device=w.device, dtype=torch.float32 if fam.split else w.dtype)
    o = 0
    for taps in (_T_TAPS if transposed else _TAPS):
        n = ct * cpk * len(taps) * wgco
        part = w[o:o + n].reshape(ct, cpk // cb, len(taps), wgco, cb).permute(0, 3, 1, 4, 2).reshape(ct * wgco, cpk, len(taps))
        if fam.split:
            part = part.float().reshape(ct * wgco, cp // 8, 2, 8, len(taps)).sum(2).reshape(ct * wgco, cp, len(taps))
        for t, (ky, kx) in enumerate(taps):
            out[:, :, ky, kx] = part[:cout, :cin, t]
        o += n
    return out.transpose(0, 1).contiguous() if transposed else out


# the public packers: (weight, bias, layer) -> (packed weights, padded bias), and their inverses
# (w, cout, cin, layer) / transposed (w, cin, cout, layer) -> the module's tensor
_layout, _layout16 = functools.partial(_layout_of, _F32), functools.partial(_layout_of, _F16)
pack_conv, pack_convt = functools.partial(_pack, _F32, False), functools.partial(_pack, _F32, True)
pack_conv16, pack_convt16 = functools.partial(_pack, _F16, False), functools.partial(_pack, _F16, True)
pack_conv_x3, pack_convt_x3 = functools.partial(_pack, _X3, False), functools.partial(_pack, _X3, True)
unpack_conv, unpack_conv16 = functools.partial(_unpack, _F32, False), functools.partial(_unpack, _F16, False)
unpack_conv_x3 = functools.partial(_unpack, _X3, False)


def unpack_convt(w, cin, cout, layer):
    return _unpack(_F32, True, w, cout, cin, layer)


def unpack_convt16(w, cin, cout, layer):
    return _unpack(_F16, True, w, cout, cin, layer)


def unpack_convt_x3(w, cin, cout, layer):
    return _unpack(_X3, True, w, cout, cin, layer)


def _conv_of(seq):
    return seq[0] if isinstance(seq, nn.Sequential) else seq


def _has_relu(seq):
    return isinstance(seq, nn.Sequential) and any(isinstance(m, nn.ReLU) for m in seq)


class _Layer:
    # conv: the module (its parameters receive the gradients); adj / dg: the adjoint-packed
    # weights and the data-gradient preset (training, GruConvs._pack_adjoints)
    # adjx / dgx: the same for the split-bf16 data gradients (GruConvs._pack_adjoints_x3), or None
    __slots__ = ("layer", "w", "b", "cin", "cout", "act", "conv", "adj", "dg", "adjx", "dgx")

    def __init__(self, layer, w, b, cin, cout, act, conv=None):
        self.layer, self.w, self.b, self.cin, self.cout, self.act = layer, w, b, cin, cout, act
        self.conv, self.adj, self.dg, self.adjx, self.dgx = conv, None, None, None, None


def _make_layer(fam, conv, act, valu):
    """The packed layer of a stride-2 conv / transposed conv module in family ``fam``: at most 16
    output channels take the *_C16 preset; with ``valu`` a 1 / 9 -> 16 conv (16 output, at most
    16 input channels) takes the VALU kernel, which reads the module's own f32 weight layout."""
    transposed, narrow = isinstance(conv, nn.ConvTranspose2d), conv.out_channels <= 16
    if valu and not transposed and conv.out_channels == 16 and conv.in_channels <= 16:
        return _Layer(fam.small, conv.weight.detach().float().contiguous(), conv.bias.detach().float().contiguous(),
                      conv.in_channels, conv.out_channels, act, conv)
    kind = (fam.t2_c16 if narrow else fam.t2) if transposed else (fam.s2_c16 if narrow else fam.s2)
    w, b = _pack(fam, transposed, conv.weight, conv.bias, kind)
    return _Layer(kind, w, b, conv.in_channels, conv.out_channels, act, conv)


def _chain_layers(fam, seq, last_act=None):
    """The layers of a module chain (the first conv may take the VALU kernel); last_act: the
    activation of the last one when it is not the module's ReLU."""
    out = [_make_layer(fam, _conv_of(s), ACT_RELU if _has_relu(s) else ACT_NONE, i == 0) for i, s in enumerate(seq)]
    if last_act is not None:
        out[-1].act = last_act
    return out


def _gru_layers(fam, g):
    """The ConvGRU's two launches: [convz; convr; convq] over (h, x), then convq's h half over r h."""
    hc = g.convz.out_channels
    w1 = torch.cat([g.convz.weight, g.convr.weight, g.convq.weight], 0)
    b1 = torch.cat([g.convz.bias, g.convr.bias, g.convq.bias], 0)
    return (_Layer(fam.gru1, *_pack(fam, False, w1, b1, fam.gru1), 2 * hc, 3 * hc, ACT_NONE),
            _Layer(fam.gru2, *_pack(fam, False, g.convq.weight[:, :hc], g.convq.bias, fam.gru2), hc, hc, ACT_NONE))


def pack_adjoint(conv):
    """(preset, packed weights) of the data gradient of a stride-2 conv / transposed conv
    module: the adjoint of a conv is the transposed conv of the same (Cout, Cin, 3, 3) tensor,
    the adjoint of a transposed conv the conv reading its (Cin, Cout, 3, 3) tensor as (out, in)."""
    if isinstance(conv, nn.ConvTranspose2d):
        dg = GC_DG_S2_C16 if conv.in_channels <= 16 else GC_DG_S2
        return dg, pack_conv(conv.weight, None, dg)[0]
    dg = GC_DG_T2_C16 if conv.in_channels <= 16 else GC_DG_T2
    return dg, pack_convt(conv.weight, None, dg)[0]


def pack_adjoint_s1(weight):
    """A stride-1 (Cout, Cin, 3, 3) conv's data gradient: the conv with the taps flipped and
    the channels transposed, packed for GC_DG_S1."""
    return pack_conv(weight.detach().transpose(0, 1).flip(2, 3), None, GC_DG_S1)[0]


def pack_adjoint_x3(conv):
    """pack_adjoint for the split-bf16 data gradients (nlspn_gconv_x3_dgrad): the same adjoint
    tensor packed with pack_convt_x3 / pack_conv_x3 for the NLSPN_GCX3_DG_* preset of its kind
    (one stride-2-mode preset for every width)."""
    if isinstance(conv, nn.ConvTranspose2d):
        return GCX3_DG_S2, pack_conv_x3(conv.weight, None, GCX3_DG_S2)[0]
    dg = GCX3_DG_T2_C16 if conv.in_channels <= 16 else GCX3_DG_T2
    return dg, pack_convt_x3(conv.weight, None, dg)[0]


def pack_adjoint_s1_x3(weight):
    """pack_adjoint_s1's tensor (taps flipped, channels transposed) packed split for GCX3_DG_S1."""
    return pack_conv_x3(weight.detach().transpose(0, 1).flip(2, 3), None, GCX3_DG_S1)[0]


# ---------------------------------------------------------------------- f16 operands (nlspn_gconv16.h)
def to_c8(x: torch.Tensor) -> torch.Tensor:
    """(B, C, H, W) -> the kernels' c8 layout (B, ceil(C/8), H, W, 8) in half, pad channels zero;
    one rounding to nearest-even.  For tests and boundaries, never on the hot path."""
    B, C, H, W = x.shape
    nb = (C + 7) // 8
    y = torch.zeros((B, nb * 8, H, W), device=x.device, dtype=torch.float16)
    y[:, :C] = x.to(torch.float16)
    return y.reshape(B, nb, 8, H, W).permute(0, 1, 3, 4, 2).contiguous()


def from_c8(y: torch.Tensor, C: int) -> torch.Tensor:
    """Inverse of to_c8: the (B, C, H, W) half tensor of a c8 tensor."""
    B, nb, H, W, _ = y.shape
    return y.permute(0, 1, 4, 2, 3).reshape(B, nb * 8, H, W)[:, :C].contiguous()


# ---------------------------------------------------------------------- split bf16 operands (nlspn_gconv_x3.h)
def to_c8x2(x: torch.Tensor) -> torch.Tensor:
    """(B, C, H, W) f32 -> the kernels' c8x2 layout, one (B, ceil(C/8), 2, H, W, 8) bfloat16 tensor:
    per 8-channel block the hi part's cells, then the lo part's (split_bf16), pad channels zero.
    For tests and boundaries, never on the hot path."""
    B, C, H, W = x.shape
    nb = (C + 7) // 8
    y = torch.zeros((B, nb * 8, H, W), device=x.device, dtype=torch.float32)
    y[:, :C] = x.float()
    return torch.stack([p.reshape(B, nb, 8, H, W).permute(0, 1, 3, 4, 2) for p in split_bf16(y)], 2).contiguous()


def from_c8x2(y: torch.Tensor, C: int, parts: bool = False):
    """Inverse of to_c8x2: the (B, C, H, W) f32 sum hi + lo of a c8x2 tensor (exact: the sum of two
    bf16 values of a split fits f32); with ``parts`` the (hi, lo) pair of bfloat16 tensors instead."""
    B, nb, _, H, W, _ = y.shape
    hi, lo = (y[:, :, s].permute(0, 1, 4, 2, 3).reshape(B, nb * 8, H, W)[:, :C].contiguous() for s in (0, 1))
    return (hi, lo) if parts else hi.float() + lo.float()


class _Mode(typing.NamedTuple):
    """An inference precision of the matrix-core families: its _Family (weight / activation dtype,
    split or not), C entry, pack-cache key and stats counter."""
    fam: _Family
    entry: str
    key: str
    stat: str

    def empty(self, B, C, H, W, device):
        """An uninitialised activation of C channels in the family's layout (c8 / c8x2)."""
        shape = (B, (C + 7) // 8, 2, H, W, 8) if self.fam.split else (B, (C + 7) // 8, H, W, 8)
        return torch.empty(shape, device=device, dtype=self.fam.dtype)


_M16 = _Mode(_F16, "nlspn_gconv16", "f16", "fwd16")
_MX3 = _Mode(_X3, "nlspn_gconv_x3", "x3", "fwd_x3")


class _ChainFn(torch.autograd.Function):
    """A chain of stride-2 convs or transposed convs (encode_dep, encode_aff, decode_aff; one
    layer: that layer) on the HIP kernels, forward and backward.  params: weight, bias per layer."""

    @staticmethod
    def forward(ctx, gc, layers, in_div, crop, x, *params):
        acts = [x.contiguous()]
        for i, L in enumerate(layers):
            if isinstance(L.conv, nn.ConvTranspose2d):
                acts.append(gc._convt(L, acts[-1], crop=crop if i == len(layers) - 1 else None))
            else:
                acts.append(gc._conv_s2(L, acts[-1], in_div=in_div if i == 0 else 1.0))
        ctx.gc, ctx.layers, ctx.in_div = gc, layers, in_div
        ctx.save_for_backward(*acts)
        return acts[-1]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        gc, layers, acts = ctx.gc, ctx.layers, ctx.saved_tensors
        g = g.contiguous()
        if layers[-1].act != ACT_NONE:  # the chain's last activation (the layers below: in the dgrad epilogues)
            g = gc._act_backward(g, acts[-1], layers[-1].act)
        grads = []
        gs = None  # g as c8x2, when a split-bf16 data gradient wrote it for the next one
        for i in reversed(range(len(layers))):
            L, xin = layers[i], acts[i]
            scale = 1.0 / ctx.in_div if i == 0 else 1.0
            grads[:0] = gc._wgrad(L, xin, g, scale)
            if i > 0 or ctx.needs_input_grad[4]:
                below = (layers[i - 1], acts[i - 1]) if i > 1 or (i == 1 and ctx.needs_input_grad[4]) else None
                g, gs = gc._dgrad(L, g, xin, layers[i - 1].act if i > 0 else ACT_NONE, scale, gs, below)
            else:
                g = None
        return (None, None, None, None, g, *grads)


class _GruFn(torch.autograd.Function):
    """The ConvGRU cell (nlspnmodel.py:398-403) on the HIP kernels, forward and backward."""

    @staticmethod
    def forward(ctx, gc, P, h, x, wz, bz, wr, br, wq, bq):
        h, x = h.contiguous(), x.contiguous()
        hc = P["hc"]
        B, _, H, W = h.shape
        z, r, rh, qx, q, hn = (torch.empty_like(h) for _ in range(6))
        g1, g2 = P["gru1"], P["gru2"]
        _lib.call("nlspn_gconv_gru_train", h.device, 1, h, x, x.shape[1], g1.w, g1.b, h, z, rh, qx, None, r, None,
                  B, H, W, hc, _lib.STREAM)
        _lib.call("nlspn_gconv_gru_train", h.device, 2, rh, None, 0, g2.w, g2.b, h, z, None, qx, hn, None, q,
                  B, H, W, hc, _lib.STREAM)
        gc.stats["fwd"] += 2
        ctx.gc, ctx.P = gc, P
        ctx.save_for_backward(h, x, z, r, q, rh)
        return hn

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dhn):
        gc, P = ctx.gc, ctx.P
        h, x, z, r, q, rh = ctx.saved_tensors
        hc = P["hc"]
        B, _, H, W = h.shape
        dev = h.device
        dhn = dhn.contiguous()
        duq, drh, dh, dx = torch.empty_like(h), torch.empty_like(h), torch.empty_like(h), torch.empty_like(x)
        duzr = torch.empty((B, 2 * hc, H, W), device=dev, dtype=torch.float32)
        cio = hc + x.shape[1]
        # "bf16x3": both adjoints on nlspn_gconv_x3_dgrad, the gate stages' f32 outputs split on entry
        x3 = gc._dgrad_x3() and "adj_q_x3" in P and all(
            gc._covers(GCX3_DG_S1, c, cio, H, W, H, W) for c in (hc, 2 * hc))
        _lib.call("nlspn_gconv_gru_gates_backward", dev, 1, dhn, z, None, q, h, None, duq, duzr, None, 0, B, hc, H, W,
                  _lib.STREAM)
        # convq's adjoint: d(r h) and its share of dx
        if x3:
            _lib.call("nlspn_gconv_x3_dgrad", dev, GCX3_DG_S1, gc._split(duq), hc, P["adj_q_x3"], None, None, None, drh,
                      dx, hc, None, B, H, W, cio, H, W, ACT_NONE, 1.0, _lib.STREAM)
        else:
            _lib.call("nlspn_gconv_dgrad", dev, GC_DG_S1, duq, hc, P["adj_q"], None, None, None, drh, dx, hc, B, H, W,
                      cio, H, W, ACT_NONE, 1.0, _lib.STREAM)
        _lib.call("nlspn_gconv_gru_gates_backward", dev, 2, dhn, z, r, None, h, drh, None, duzr, dh, 0, B, hc, H, W,
                  _lib.STREAM)
        # [convz; convr]'s adjoint, added into dh and dx in place
        if x3:
            _lib.call("nlspn_gconv_x3_dgrad", dev, GCX3_DG_S1, gc._split(duzr), 2 * hc, P["adj_zr_x3"], None, dh, dx, dh,
                      dx, hc, None, B, H, W, cio, H, W, ACT_NONE, 1.0, _lib.STREAM)
        else:
            _lib.call("nlspn_gconv_dgrad", dev, GC_DG_S1, duzr, 2 * hc, P["adj_zr"], None, dh, dx, dh, dx, hc, B, H, W,
                      cio, H, W, ACT_NONE, 1.0, _lib.STREAM)
        gc.stats["gates_bwd"] += 2
        gc.stats["dgrad_x3" if x3 else "dgrad"] += 2
        dwq, dbq = gc._wgrad_raw(1, duq, rh, x, False, 1.0)
        dwzr, dbzr = gc._wgrad_raw(1, duzr, h, x, False, 1.0)
        return None, None, dh, dx, dwzr[:hc], dbzr[:hc], dwzr[hc:], dbzr[hc:], dwq, dbq


class GruConvs:
    """The packed GRU-mode convolutions of one NLSPNModel (encode_dep, encode_aff, ConvGRU,
    decode_aff), one entry per device, rebuilt when any parameter changes (storage pointer
    or version counter)."""

    def __init__(self):
        self._entries = {}
        self._ws = {}  # (device, stream) -> the weight-gradient workspace
        # "bf16x3": the weight gradients on the bf16 matrix cores with split operands
        # (nlspn_gconv_wgrad_bf16x3, csrc/nlspn_gwgrad16.h); "fp32" (default): nlspn_gconv_wgrad
        self.wgrad_precision = "fp32"
        # True: the layers nlspn_gconv_wgrad_narrow_covers accepts (stride 2, both channel counts
        # <= 16) take nlspn_gconv_wgrad_narrow (csrc/nlspn_gwnarrow.h), whatever wgrad_precision is
        self.wgrad_narrow = False
        # "bf16x3": the data gradients nlspn_gconv_x3_dgrad_covers accepts (the wide layers' and the
        # ConvGRU's) on the split-bf16 convolution kernels (nlspn_gconv_x3_dgrad,
        # csrc/nlspn_gconv_x3.h); "fp32" (default): nlspn_gconv_dgrad everywhere
        self.dgrad_precision = "fp32"
        self.reset_stats()

    def reset_stats(self):
        """Launch counts per kind since the last reset: ``fwd`` (forward launches), ``dgrad``,
        ``wgrad`` (kernel launches of the weight / bias gradients) and ``gates_bwd``; ``gru_fwd``
        counts ConvGRU cell forwards; ``fwd16`` the forward launches of the f16-operand family;
        ``wgrad_x3`` the weight / bias gradient launches of the ``"bf16x3"`` mode, counted as
        ``wgrad`` counts the f32 entry's; ``fwd_x3`` the forward launches of the split-bf16 family;
        ``wgrad_narrow`` the launches of the narrow layers' streaming entry (two per call);
        ``dgrad_x3`` the data-gradient launches of the ``"bf16x3"`` data-gradient mode (``dgrad``
        keeps counting the f32 entry's) and ``split_x3`` its f32 -> c8x2 launches."""
        self.stats = {"fwd": 0, "dgrad": 0, "wgrad": 0, "gates_bwd": 0, "gru_fwd": 0, "fwd16": 0, "wgrad_x3": 0,
                      "fwd_x3": 0, "wgrad_narrow": 0, "dgrad_x3": 0, "split_x3": 0}

    @staticmethod
    def supported(model) -> bool:
        """The reference's GRU-mode architecture (nlspnmodel.py:122-143): 3x3 convs, stride 2
        encoders, stride-2 transposed decoders, a ConvGRU with hidden channels a multiple of
        128, float32 CUDA weights."""
        if not getattr(model.args, "use_GRU", False):
            return False
        hc = model.args.GRU_hidden_dim
        if hc % 128 != 0 or model.args.GRU_input_dim != hc:
            return False
        convs = [_conv_of(s) for s in list(model.encode_dep) + list(model.encode_aff)[:3]]
        convts = [_conv_of(s) for s in model.decode_aff]
        for c in convs:
            if not isinstance(c, nn.Conv2d) or c.kernel_size != (3, 3) or c.stride != (2, 2) or c.padding != (1, 1) \
                    or c.bias is None or c.groups != 1 or c.dilation != (1, 1):
                return False
        for c in convts:
            if not isinstance(c, nn.ConvTranspose2d) or c.kernel_size != (3, 3) or c.stride != (2, 2) \
                    or c.padding != (1, 1) or c.output_padding != (1, 1) or c.bias is None or c.groups != 1:
                return False
        g = model.GRU
        w = g.convz.weight
        return w.is_cuda and w.dtype == torch.float32

    @staticmethod
    def _pack_adjoints(model, packed):
        with torch.no_grad():
            for L in packed["dep"] + packed["aff"] + packed["dec"]:
                L.dg, L.adj = pack_adjoint(L.conv)
            g = model.GRU
            packed["adj_q"] = pack_adjoint_s1(g.convq.weight)
            packed["adj_zr"] = pack_adjoint_s1(torch.cat([g.convz.weight, g.convr.weight], 0))

    @staticmethod
    def _pack_adjoints_x3(model, packed):
        """The split-bf16 adjoint packs beside the f32 ones (same entry, same invalidation key)."""
        with torch.no_grad():
            for L in packed["dep"] + packed["aff"] + packed["dec"]:
                L.dgx, L.adjx = pack_adjoint_x3(L.conv)
            g = model.GRU
            packed["adj_q_x3"] = pack_adjoint_s1_x3(g.convq.weight)
            packed["adj_zr_x3"] = pack_adjoint_s1_x3(torch.cat([g.convz.weight, g.convr.weight], 0))

    def pack(self, model):
        P = self._pack_f32(model)
        # (packed when the mode first needs them: under gradients with dgrad_precision = "bf16x3")
        if torch.is_grad_enabled() and self.dgrad_precision == "bf16x3" and "adj_q_x3" not in P:
            self._pack_adjoints_x3(model, P)
        return P

    def _pack_f32(self, model):
        params = [p for m in (model.encode_dep, model.encode_aff, model.GRU, model.decode_aff) for p in m.parameters()]
        key = (params[0].device, tuple((p.data_ptr(), p._version) for p in params))
        e = self._entries.get(params[0].device)
        if e is not None and e[0] == key:
            if torch.is_grad_enabled() and "adj_q" not in e[1]:
                self._pack_adjoints(model, e[1])
            return e[1]
        with torch.no_grad():
            dep = _chain_layers(_F32, list(model.encode_dep))
            aff = _chain_layers(_F32, list(model.encode_aff)[:3], ACT_TANH)  # encode_aff's Tanh (:131)
            dec = _chain_layers(_F32, list(model.decode_aff))
            g = model.GRU
            gru1, gru2 = _gru_layers(_F32, g)
            hc = g.convz.out_channels
        packed = {"dep": dep, "aff": aff, "dec": dec, "gru1": gru1, "gru2": gru2, "hc": hc,
                  "gru_params": [g.convz.weight, g.convz.bias, g.convr.weight, g.convr.bias, g.convq.weight, g.convq.bias]}
        if torch.is_grad_enabled():
            self._pack_adjoints(model, packed)
        self._entries[params[0].device] = (key, packed)
        return packed

    def pack16(self, model):
        """The f16 packs (pack_conv16 / pack_convt16) beside the f32 ones, in the same cache entry
        under the same invalidation key, packed when first needed."""
        return self._pack_mode(_M16, model, "fp16")

    def pack_x3(self, model):
        """The split-bf16 packs (pack_conv_x3 / pack_convt_x3), cached as pack16's are."""
        return self._pack_mode(_MX3, model, "bf16x3")

    def _pack_mode(self, M, model, name):
        P = self.pack(model)
        if M.key in P:
            return P
        # (the chains start on the VALU kernel, which reads f32 NCHW, and end on the f32 last
        # decoder layer: the reference's architecture; anything else has no such kernel)
        first = [_conv_of(seq[0]) for seq in (model.encode_dep, model.encode_aff)]
        if any(c.out_channels != 16 or c.in_channels > 16 for c in first) or len(model.decode_aff) < 2:
            raise NotImplementedError(f"gru_precision = '{name}' needs the reference's GRU-mode layers (1 / 9 -> 16 first "
                                      "encoder convs, at least two decoder layers)")
        with torch.no_grad():
            gru1, gru2 = _gru_layers(M.fam, model.GRU)
            P[M.key] = {"dep": _chain_layers(M.fam, list(model.encode_dep)),
                        "aff": _chain_layers(M.fam, list(model.encode_aff)[:3], ACT_TANH),
                        "dec": _chain_layers(M.fam, list(model.decode_aff)[:-1]), "gru1": gru1, "gru2": gru2}
        return P

    # ------------------------------------------------------------------ f16 / split-bf16 launches (inference)
    # M: the mode (_M16 / _MX3); "c8" below stands for the mode's activation layout (c8 / c8x2)
    def _runm(self, M, L, x0, c0, B, Hi, Wi, x1=None, c1=0, yh=None, y32=None, ohs=0, ows=0, in_div=1.0, h=None, zb=None,
              rhh=None, qxb=None, hout32=None, houth=None, hc=0):
        _lib.call(M.entry, x0.device, L.layer, x0, c0, x1, c1, L.w, L.b, yh, y32, h, zb, rhh, qxb, hout32,
                  houth, B, Hi, Wi, L.cout, ohs, ows, L.act, in_div, hc, _lib.STREAM)
        self.stats[M.stat] += 1

    def _encm(self, M, layers, x, in_div, both):
        """A stride-2 encoder chain: f32 NCHW in, c8 between the layers and out (both: the last
        layer also writes f32 NCHW: (y32, y16))."""
        B, _, Hi, Wi = x.shape
        y32 = None
        for i, L in enumerate(layers):
            Ho, Wo = (Hi - 1) // 2 + 1, (Wi - 1) // 2 + 1
            y = M.empty(B, L.cout, Ho, Wo, x.device)
            if both and i == len(layers) - 1:
                y32 = torch.empty((B, L.cout, Ho, Wo), device=x.device, dtype=torch.float32)
            self._runm(M, L, x, L.cin, B, Hi, Wi, yh=y, y32=y32, ohs=Ho, ows=Wo, in_div=in_div if i == 0 else 1.0)
            x, Hi, Wi = y, Ho, Wo
        return (y32, x) if both else x

    def _grum(self, M, P, state, xh):
        self.stats["gru_fwd"] += 1
        h, hh = state
        hc = P["hc"]
        B, _, H, W = h.shape
        z, qx, hn = torch.empty_like(h), torch.empty_like(h), torch.empty_like(h)
        rhh, hnh = torch.empty_like(hh), torch.empty_like(hh)
        F = P[M.key]
        self._runm(M, F["gru1"], hh, hc, B, H, W, x1=xh, c1=hc, h=h, zb=z, rhh=rhh, qxb=qx, hc=hc)
        self._runm(M, F["gru2"], rhh, hc, B, H, W, h=h, zb=z, qxb=qx, hout32=hn, houth=hnh, hc=hc)
        return hn, hnh

    def _decm(self, M, P, state, crop, gamma, kind):
        x = state[1]
        B, Hi, Wi = x.shape[0], x.shape[-3], x.shape[-2]
        layers = P[M.key]["dec"]
        y32 = None
        for i, L in enumerate(layers):
            Ho, Wo = 2 * Hi, 2 * Wi
            last = i == len(layers) - 1
            if last:
                y32 = torch.empty((B, L.cout, Ho, Wo), device=x.device, dtype=torch.float32)
                self._runm(M, L, x, L.cin, B, Hi, Wi, y32=y32, ohs=Ho, ows=Wo)
            else:
                y = M.empty(B, L.cout, Ho, Wo, x.device)
                self._runm(M, L, x, L.cin, B, Hi, Wi, yh=y, ohs=Ho, ows=Wo)
                x = y
            Hi, Wi = Ho, Wo
        Pl = dict(P)
        Pl["dec"] = P["dec"][-1:]
        return self.decode_aff(Pl, y32, crop, gamma=gamma, kind=kind)

    def encode_dep16(self, P, new_pred, max_depth):
        """encode_dep(new_pred / max_depth) on the f16 matrix cores: the c8 features."""
        return self._encm(_M16, P["f16"]["dep"], new_pred.contiguous().float(), float(max_depth), False)

    def encode_aff16(self, P, aff):
        """encode_aff on the f16 matrix cores: the initial state (h f32, its c8 copy)."""
        return self._encm(_M16, P["f16"]["aff"], aff.contiguous().float(), 1.0, True)

    def gru16(self, P, state, x16):
        """ConvGRU on the f16 matrix cores: state = (h f32, h c8), x16 the c8 input; the new state."""
        return self._grum(_M16, P, state, x16)

    def decode_aff16(self, P, state, crop, gamma=None, kind=None):
        """decode_aff on the f16 matrix cores up to its last layer's f32 NCHW input; the last
        layer (16 -> K, the crop and the fused normalisation) is the f32 family's, unchanged."""
        return self._decm(_M16, P, state, crop, gamma, kind)

    def encode_dep_x3(self, P, new_pred, max_depth):
        """encode_dep(new_pred / max_depth) on the bf16 matrix cores, split operands: the c8x2 features."""
        return self._encm(_MX3, P["x3"]["dep"], new_pred.contiguous().float(), float(max_depth), False)

    def encode_aff_x3(self, P, aff):
        """encode_aff, split operands: the initial state (h f32, its c8x2 copy)."""
        return self._encm(_MX3, P["x3"]["aff"], aff.contiguous().float(), 1.0, True)

    def gru_x3(self, P, state, xs):
        """ConvGRU, split operands: state = (h f32, h c8x2), xs the c8x2 input; the new state."""
        return self._grum(_MX3, P, state, xs)

    def decode_aff_x3(self, P, state, crop, gamma=None, kind=None):
        """decode_aff, split operands, up to its last layer's f32 NCHW input; the last layer is
        the f32 family's, unchanged (as decode_aff16)."""
        return self._decm(_MX3, P, state, crop, gamma, kind)

    # ------------------------------------------------------------------ launches
    @staticmethod
    def _run(L, x0, c0, x1=None, c1=0, out=None, ohs=None, ows=None, in_div=1.0, h=None, zb=None, rhb=None,
             qxb=None, hout=None, hc=0):
        B, _, Hi, Wi = x0.shape
        _lib.call("nlspn_gconv", x0.device, L.layer, x0, c0, x1, c1, L.w, L.b, out, h, zb, rhb, qxb, hout,
                  B, Hi, Wi, L.cout, ohs or 0, ows or 0, L.act, in_div, hc, _lib.STREAM)

    def _conv_s2(self, L, x, in_div=1.0):
        B, _, Hi, Wi = x.shape
        Ho, Wo = (Hi - 1) // 2 + 1, (Wi - 1) // 2 + 1
        y = torch.empty((B, L.cout, Ho, Wo), device=x.device, dtype=torch.float32)
        self._run(L, x, L.cin, out=y, ohs=Ho, ows=Wo, in_div=in_div)
        self.stats["fwd"] += 1
        return y

    def _convt(self, L, x, crop=None):
        B, _, Hi, Wi = x.shape
        Ho, Wo = 2 * Hi, 2 * Wi
        ohs, ows = (min(crop[0], Ho), min(crop[1], Wo)) if crop else (Ho, Wo)
        y = torch.empty((B, L.cout, ohs, ows), device=x.device, dtype=torch.float32)
        self._run(L, x, L.cin, out=y, ohs=ohs, ows=ows)
        self.stats["fwd"] += 1
        return y

    def encode_dep(self, P, new_pred, max_depth):
        """encode_dep(new_pred / max_depth) (:366): the division in the first conv's loads."""
        if torch.is_grad_enabled():
            return self._chain(P["dep"], new_pred, in_div=float(max_depth))
        x = new_pred.contiguous().float()
        for i, L in enumerate(P["dep"]):
            x = self._conv_s2(L, x, in_div=float(max_depth) if i == 0 else 1.0)
        return x

    def encode_aff(self, P, aff):
        if torch.is_grad_enabled():
            return self._chain(P["aff"], aff)
        x = aff.contiguous().float()
        for L in P["aff"]:
            x = self._conv_s2(L, x)
        return x

    def gru(self, P, h, x):
        """ConvGRU (:398-403): h' = (1 - z) h + z q."""
        self.stats["gru_fwd"] += 1
        if torch.is_grad_enabled():
            return _GruFn.apply(self, P, h, x, *P["gru_params"])
        h, x = h.contiguous(), x.contiguous()
        hc = P["hc"]
        z, rh, qx = (torch.empty_like(h) for _ in range(3))
        hn = torch.empty_like(h)
        self._run(P["gru1"], h, hc, x, x.shape[1], h=h, zb=z, rhb=rh, qxb=qx, hc=hc)
        self._run(P["gru2"], rh, hc, h=h, zb=z, qxb=qx, hout=hn, hc=hc)
        self.stats["fwd"] += 2
        return hn

    def decode_aff(self, P, h, crop, gamma=None, kind=None):
        """decode_aff + _clip_as (:228-250): the last layer stores only the cropped rows / columns.
        With ``gamma`` / ``kind`` (and K = 8 raw taps) the last layer also normalises them
        (_affinity_normalization + _aff_insert, :179-201, :261-269) in its epilogue
        (nlspn_gconv_affnorm): the (B, K+1, H, W) affinity, bit-equal to the conv followed by
        ``affinity_normalization``, without the raw planes' round trip or a launch.  Otherwise
        the raw (B, K, H, W) taps (always under gradients: the differentiable
        ``affinity_normalization`` follows)."""
        if torch.is_grad_enabled():
            return self._chain(P["dec"], h, crop=crop)
        x = h
        for L in P["dec"][:-1]:
            x = self._convt(L, x)
        L = P["dec"][-1]
        if gamma is None or L.cout != 8 or L.layer != GC_T2_C16:
            return self._convt(L, x, crop=crop)
        B, _, Hi, Wi = x.shape
        ohs, ows = (min(crop[0], 2 * Hi), min(crop[1], 2 * Wi)) if crop else (2 * Hi, 2 * Wi)
        g = gamma.detach().reshape(-1)[:1].to(device=x.device, dtype=torch.float32).contiguous()
        y = torch.empty((B, L.cout + 1, ohs, ows), device=x.device, dtype=torch.float32)
        _lib.call("nlspn_gconv_affnorm", x.device, x, L.cin, L.w, L.b, y, g, _lib.AFF_KINDS[kind],
                  B, Hi, Wi, L.cout, ohs, ows, L.act, _lib.STREAM)
        self.stats["fwd"] += 1
        return y

    # ------------------------------------------------------------------ training
    def _chain(self, layers, x, in_div=1.0, crop=None):
        """The layers on the HIP kernels under autograd (_ChainFn): the modules' parameters receive dW / db."""
        params = [p for L in layers for p in (L.conv.weight, L.conv.bias)]
        return _ChainFn.apply(self, layers, in_div, crop, x.float(), *params)

    def layer(self, conv, x, act=ACT_NONE, in_div=1.0, crop=None):
        """One stride-2 conv / transposed conv module with activation ``act`` on the HIP kernels,
        differentiable: a one-layer chain packed on the spot (tests; the model uses the cached packs)."""
        with torch.no_grad():
            L = _make_layer(_F32, conv, act, True)
            L.dg, L.adj = pack_adjoint(conv)
            if self.dgrad_precision == "bf16x3":
                L.dgx, L.adjx = pack_adjoint_x3(conv)
        return self._chain([L], x, in_div=in_div, crop=crop)

    def _act_backward(self, g, y, act):
        out = torch.empty_like(g)
        _lib.call("nlspn_gconv_gru_gates_backward", g.device, 0, g, y, None, None, None, None, out, None, None, act,
                  1, 1, 1, g.numel(), _lib.STREAM)
        self.stats["dgrad"] += 1
        return out

    def _dgrad_x3(self):
        """Whether the data gradients take the split-bf16 entry where it covers them."""
        if self.dgrad_precision not in ("fp32", "bf16x3"):
            raise ValueError(f"dgrad_precision must be 'fp32' or 'bf16x3', got {self.dgrad_precision!r}")
        return self.dgrad_precision == "bf16x3"

    @staticmethod
    def _covers(dgx, cg, cout, Hg, Wg, Ho, Wo):
        return bool(_lib.get().nlspn_gconv_x3_dgrad_covers(dgx, cg, cout, Hg, Wg, Ho, Wo))

    def _split(self, g):
        """An f32 NCHW gradient as c8x2 (nlspn_gconv_x3_split): where it enters a chain in f32."""
        B, C, H, W = g.shape
        gs = _MX3.empty(B, C, H, W, g.device)
        _lib.call("nlspn_gconv_x3_split", g.device, g, gs, B, C, H, W, _lib.STREAM)
        self.stats["split_x3"] += 1
        return gs

    def _dgrad(self, L, g, xin, act_below, scale, gs=None, below=None):
        """dL/d(pre-activation of the layer below) = act_below'(xin) * scale * adjoint(L)(g), and
        its c8x2 copy or None.  gs: g as c8x2 when the data gradient before wrote it; below: the
        (layer, input) whose data gradient follows, or None: with dgrad_precision = "bf16x3" a
        covered launch also writes the split copy when that next one is covered too."""
        B, cg, Hg, Wg = g.shape
        dx = torch.empty_like(xin)
        _, cout, Ho, Wo = xin.shape
        ysave = xin if act_below != ACT_NONE else None
        if self._dgrad_x3() and L.dgx is not None and self._covers(L.dgx, cg, cout, Hg, Wg, Ho, Wo):
            dxs = None
            if below is not None and below[0].dgx is not None and self._covers(
                    below[0].dgx, cout, below[1].shape[1], Ho, Wo, *below[1].shape[2:]):
                dxs = _MX3.empty(B, cout, Ho, Wo, g.device)
            _lib.call("nlspn_gconv_x3_dgrad", g.device, L.dgx, self._split(g) if gs is None else gs, cg, L.adjx, ysave,
                      None, None, dx, None, cout, dxs, B, Hg, Wg, cout, Ho, Wo, act_below, scale, _lib.STREAM)
            self.stats["dgrad_x3"] += 1
            return dx, dxs
        _lib.call("nlspn_gconv_dgrad", g.device, L.dg, g, cg, L.adj, ysave, None,
                  None, dx, None, cout, B, Hg, Wg, cout, Ho, Wo, act_below, scale, _lib.STREAM)
        self.stats["dgrad"] += 1
        return dx, None

    def _wgrad(self, L, xin, g, scale):
        if isinstance(L.conv, nn.ConvTranspose2d):  # small = the input, large = the (cropped) output gradient
            return self._wgrad_raw(2, xin, g, None, True, scale)
        return self._wgrad_raw(2, g, xin, None, False, scale)

    def _wgrad_raw(self, stride, s, l0, l1, bias_from_large, scale):
        """(dW (Cs, Cl, 3, 3), db) of nlspn_gconv_wgrad (wgrad_precision = "bf16x3": of
        nlspn_gconv_wgrad_bf16x3; wgrad_narrow and a shape nlspn_gconv_wgrad_narrow_covers accepts:
        of nlspn_gconv_wgrad_narrow): s the small tensor, l0 (+ l1) the large one."""
        if self.wgrad_precision not in ("fp32", "bf16x3"):
            raise ValueError(f"wgrad_precision must be 'fp32' or 'bf16x3', got {self.wgrad_precision!r}")
        if not isinstance(self.wgrad_narrow, bool):
            raise ValueError(f"wgrad_narrow must be a bool, got {self.wgrad_narrow!r}")
        x3 = self.wgrad_precision == "bf16x3"
        name = "nlspn_gconv_wgrad_bf16x3" if x3 else "nlspn_gconv_wgrad"
        lib = _lib.get()
        B, Cs, Hs, Ws = s.shape
        c0, c1 = l0.shape[1], 0 if l1 is None else l1.shape[1]
        narrow = self.wgrad_narrow and bool(lib.nlspn_gconv_wgrad_narrow_covers(stride, Cs, c0, c1))
        if narrow:
            name = "nlspn_gconv_wgrad_narrow"
        Hl, Wl = l0.shape[2:]
        need = getattr(lib, name + "_workspace_bytes")(stride, Cs, c0 + c1, B, Hs, Ws, Hl, Wl)
        key = (s.device, torch.cuda.current_stream(s.device).cuda_stream)
        ws = self._ws.get(key)
        if ws is None or ws.numel() * 4 < need:
            ws = self._ws[key] = torch.empty((need + 3) // 4, device=s.device, dtype=torch.float32)
        dw = torch.empty((Cs, c0 + c1, 3, 3), device=s.device, dtype=torch.float32)
        db = torch.empty(c0 if bias_from_large else Cs, device=s.device, dtype=torch.float32)
        _lib.call(name, s.device, stride, s, Cs, l0, c0, l1, c1, dw, db, int(bias_from_large), scale,
                  ws, ws.numel() * 4, B, Hs, Ws, Hl, Wl, _lib.STREAM)
        if narrow:
            self.stats["wgrad_narrow"] += 2
        else:
            self.stats["wgrad_x3" if x3 else "wgrad"] += 4
        return dw, db
