"""Head epilogue on the HIP kernel: the decoder's last three 3x3
convolutions as one kernel.

Reference: src/model/nlspnmodel.py:296-315 —
    pred_init  = id_dec0(cat(id_fd1, fe1))        ReLU      (:297, id_dec0 :68)
    off_aff    = off_aff_dec0(cat(off_aff_fd1, fe1))         (:301, off_aff_dec0 :74/:76)
    confidence = cf_dec0(cat(cf_fd1, fe1))        Sigmoid   (:313, cf_dec0 :83-86)
``head_epilogue`` reads fe1 and the three decoder outputs in place (no concatenated
copies) and computes all three convolutions with bias and activation in one launch
(``nlspn_head_epilogue``, ``csrc/nlspn_heads.h``): f32 operands on the matrix cores,
exact f32 products, f32 accumulation.  Inference only (no autograd formula): the model
calls it when gradients are off; training keeps the torch convolutions.

The three convolutions' weights are packed once per weight version into the kernel's
layout (``nlspn_head_pack_weights``) and cached on the module.

``precision="bf16x3"`` (opt-in; default ``"fp32"``) runs the same epilogues on the bf16
matrix cores with every f32 MFMA operand split into two bf16 parts
(``nlspn_head_epilogue_x3``, ``csrc/nlspn_heads_x3.h``): weights split when packed, fe1 and
off_aff_fd1 while staged, three products per term (lo lo dropped), f32 accumulation; the
one-channel id / cf decoder halves, bias, activations and the fused prologue are the f32
kernel's code.  ``stats`` counts the launches per precision.
"""
from __future__ import annotations

import ctypes

import torch
import torch.nn as nn

from . import _lib

__all__ = ["head_epilogue", "head_epilogue_prologue", "HeadWeights", "PRECISIONS", "stats"]

PRECISIONS = ("fp32", "bf16x3")
# kernel launches per precision (epilogue and fused-prologue entries alike), so a test can prove
# which kernel ran
stats = {"fp32": 0, "bf16x3": 0}
# per precision: (packed-size entry, pack entry, epilogue entry, fused-prologue entry, dtype of wm)
_ENTRIES = {
    "fp32": ("nlspn_head_packed_size", "nlspn_head_pack_weights", "nlspn_head_epilogue",
             "nlspn_head_epilogue_prologue", torch.float32),
    "bf16x3": ("nlspn_head_x3_packed_size", "nlspn_head_x3_pack_weights", "nlspn_head_epilogue_x3",
               "nlspn_head_epilogue_prologue_x3", torch.bfloat16),
}


def _check_precision(precision):
    if precision not in PRECISIONS:
        raise ValueError(f"precision must be 'fp32' or 'bf16x3', got {precision!r}")
    return precision


def _conv_of(m):
    """The nn.Conv2d of a head (a bare conv, or the first layer of conv_bn_relu /
    cf_dec0's Sequential)."""
    if m is None or isinstance(m, nn.Conv2d):
        return m
    return m[0]


class _Packed:
    __slots__ = ("key", "wm", "wv", "bias", "C", "nout", "keep")


class HeadWeights:
    """The packed weights of (off_aff_dec0, id_dec0, cf_dec0), one entry per (device,
    precision), rebuilt when any of the convolutions' parameters change (storage pointer or tensor
    version counter).  An entry is never mutated after it is built, so DataParallel
    replicas sharing this cache from their threads each get their own device's entry."""

    def __init__(self):
        self._entries = {}

    @staticmethod
    def _check(conv, name, nout=None):
        if conv is None:
            return
        if conv.kernel_size != (3, 3) or conv.stride != (1, 1) or conv.padding != (1, 1) or conv.dilation != (1, 1) \
                or conv.groups != 1 or conv.bias is None:
            raise RuntimeError(f"{name} must be a 3x3 / stride 1 / pad 1 convolution with bias (conv_bn_relu(..., "
                               "bn=False), nlspnmodel.py:68-86)")
        if nout is not None and conv.out_channels != nout:
            raise RuntimeError(f"{name} must have {nout} output channel(s), has {conv.out_channels}")
        if conv.weight.dtype != torch.float32 or not conv.weight.is_cuda:
            raise RuntimeError(f"{name} weights must be float32 CUDA tensors")

    def get(self, oa, idc, cfc, precision="fp32") -> _Packed:
        size_fn, pack_fn, _, _, wm_dtype = _ENTRIES[_check_precision(precision)]
        self._check(oa, "off_aff_dec0")
        self._check(idc, "id_dec0", 1)
        self._check(cfc, "cf_dec0", 1)
        C2 = oa.in_channels
        for c, n in ((idc, "id_dec0"), (cfc, "cf_dec0")):
            if c is not None and c.in_channels != C2:
                raise RuntimeError(f"{n} must read {C2} channels like off_aff_dec0, reads {c.in_channels}")
        params = [t for c in (oa, idc, cfc) if c is not None for t in (c.weight, c.bias)]
        key = (tuple((t.data_ptr(), t._version) for t in params), idc is None, cfc is None)
        dev = oa.weight.device
        e = self._entries.get((dev, precision))
        if e is not None and e.key == key:
            return e
        C, nout = C2 // 2, oa.out_channels
        lib = _lib.get()
        nm, nv, nb = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        _lib.check(getattr(lib, size_fn)(C, nout, ctypes.byref(nm), ctypes.byref(nv), ctypes.byref(nb)))
        e = _Packed()
        e.wm = torch.empty(nm.value, dtype=wm_dtype, device=dev)
        e.wv = torch.empty(nv.value, dtype=torch.float32, device=dev)
        e.bias = torch.empty(nb.value, dtype=torch.float32, device=dev)
        w = lambda c: None if c is None else c.weight.detach().contiguous()  # noqa: E731
        b = lambda c: None if c is None else c.bias.detach().contiguous()  # noqa: E731
        e.keep = [w(oa), b(oa), w(idc), b(idc), w(cfc), b(cfc)]  # alive until the pack kernel has run
        _lib.call(pack_fn, dev, *e.keep, e.wm, e.wv, e.bias, C, nout, _lib.STREAM)
        e.key, e.C, e.nout = key, C, nout
        self._entries[(dev, precision)] = e
        return e


def _mb(nout):
    """M-blocks of nout + 2 columns (hx3_mb, csrc/nlspn_heads_x3_plan.h): 1, 2, 3 or 5."""
    mb = (nout + 2 + 31) // 32
    if mb > 5:
        raise ValueError(f"nout={nout} (at most 158)")
    return mb if mb <= 3 else 5


def pack_wm_x3_reference(oa, idc=None, cfc=None):
    """What nlspn_head_x3_pack_weights writes into wm, built with torch on the weights' device
    (the tests' yardstick for the pack kernel; not on the hot path): bf16
    [source 2][chunk C/16][tap 9][M-block][part 2][lane 64][8], lane (l32, h) of M-block m
    holding column 32 m + l32, channels 16 chunk + 8 h + j; part 0 = rne_bf16(w), part 1 =
    rne_bf16(w - hi).  Columns: 0..nout-1 off_aff_dec0, nout id_dec0 and nout + 1 cf_dec0
    (source 0 = fe1 only), zeros past them."""
    C, nout = oa.in_channels // 2, oa.out_channels
    mb = _mb(nout)
    w = oa.weight.detach().float()
    dense = torch.zeros((2, C, 9, 32 * mb), dtype=torch.float32, device=w.device)  # [s][c][t][co]
    dense[0, :, :, :nout] = w[:, C:].reshape(nout, C, 9).permute(1, 2, 0)
    dense[1, :, :, :nout] = w[:, :C].reshape(nout, C, 9).permute(1, 2, 0)
    for k, c in enumerate((idc, cfc)):
        if c is not None:
            dense[0, :, :, nout + k] = c.weight.detach().float()[0, C:].reshape(C, 9)
    hi = dense.to(torch.bfloat16)
    lo = (dense - hi.float()).to(torch.bfloat16)
    parts = torch.stack((hi, lo), 0).view(2, 2, C // 16, 2, 8, 9, mb, 32)  # [part][s][chunk][h][j][t][m][l32]
    return parts.permute(1, 2, 5, 6, 0, 3, 7, 4).contiguous().view(-1)


def unpack_wm_x3(wm, C, nout):
    """(hi, lo) of a packed wm as dense bf16 [source 2][C][tap 9][32 MB columns]."""
    mb = _mb(nout)
    v = wm.view(2, C // 16, 9, mb, 2, 2, 32, 8).permute(4, 0, 1, 5, 7, 2, 3, 6)  # [part][s][chunk][h][j][t][m][l32]
    v = v.reshape(2, 2, C, 9, 32 * mb)
    return v[0], v[1]


def _sources(fe1, off_aff_fd1, id_fd1, cf_fd1, bad):
    """The decoder outputs the kernel reads, made contiguous: each present one a float32
    CUDA tensor of fe1's shape, else `bad(name, tensor, shape)` gives the caller's message."""
    srcs = (fe1, off_aff_fd1, id_fd1, cf_fd1)
    for n, t in zip(("fe1", "off_aff_fd1", "id_fd1", "cf_fd1"), srcs):
        if t is not None and (not t.is_cuda or t.dtype != torch.float32 or t.shape != fe1.shape):
            raise RuntimeError(bad(n, t, tuple(fe1.shape)))
    return [None if t is None else t.contiguous() for t in srcs]


def head_epilogue(fe1, off_aff_fd1, off_aff_dec0, id_fd1=None, id_dec0=None, cf_fd1=None, cf_dec0=None,
                  weights: HeadWeights | None = None, precision: str = "fp32"):
    """(pred_init, off_aff, confidence) of nlspnmodel.py:297-315 from the decoder outputs.
    ``id_fd1``/``id_dec0`` and ``cf_fd1``/``cf_dec0`` may be None (that head is skipped
    and None returned for it).  ``precision``: "fp32" or "bf16x3" (module docstring)."""
    entry = _ENTRIES[_check_precision(precision)][2]
    oa, idc, cfc = _conv_of(off_aff_dec0), _conv_of(id_dec0), _conv_of(cf_dec0)
    if (id_fd1 is None) != (idc is None) or (cf_fd1 is None) != (cfc is None):
        raise RuntimeError("each head needs both its decoder output and its convolution")
    weights = (weights or HeadWeights()).get(oa, idc, cfc, precision)  # this device's packed entry
    B, C, H, W = fe1.shape
    if C != weights.C:
        raise RuntimeError(f"fe1 has {C} channels, the head convolutions expect {weights.C} + {weights.C}")
    srcs = _sources(fe1, off_aff_fd1, id_fd1, cf_fd1, lambda n, t, shape: (
        f"{n} must be a float32 CUDA tensor" if not t.is_cuda or t.dtype != torch.float32 else
        f"{n} must be {shape} (the _concat crop is done by the caller), got {tuple(t.shape)}"))
    dev = fe1.device
    off_aff = torch.empty((B, weights.nout, H, W), dtype=torch.float32, device=dev)
    pred_init = torch.empty((B, 1, H, W), dtype=torch.float32, device=dev) if id_fd1 is not None else None
    conf = torch.empty((B, 1, H, W), dtype=torch.float32, device=dev) if cf_fd1 is not None else None
    _lib.call(entry, dev, _lib.DTYPE_F32, *srcs, weights.wm, weights.wv, weights.bias, off_aff,
              pred_init, conf, B, C, H, W, weights.nout, _lib.STREAM)
    stats[precision] += 1
    return pred_init, off_aff, conf


def head_epilogue_prologue(fe1, off_aff_fd1, off_aff_dec0, id_fd1, id_dec0, dep, gamma, affinity="TGASS",
                           cf_fd1=None, cf_dec0=None, preserve_input=True, always_clip=False,
                           weights: HeadWeights | None = None, precision: str = "fp32") -> dict:
    """The three head convolutions with the propagation prologue fused into their
    epilogue (3x3, K = 8, offsets on; nlspnmodel.py:297-348): returns {'pred_init',
    'offset' (_off_insert, :324), 'aff' (normalised + reference tap, :325),
    'confidence' (blended, :328-334, or None), 'p0' (iteration 1's input, :341-348)} —
    what nlspn_propagate's step 1 would produce from the raw head outputs, bit for bit.
    Feed them to propagation.propagate_normalized.  ``precision`` as head_epilogue's."""
    entry = _ENTRIES[_check_precision(precision)][3]
    oa, idc, cfc = _conv_of(off_aff_dec0), _conv_of(id_dec0), _conv_of(cf_dec0)
    if (cf_fd1 is None) != (cfc is None) or id_fd1 is None or idc is None:
        raise RuntimeError("the fused prologue needs id_fd1/id_dec0, and cf_fd1 with cf_dec0")
    if oa.out_channels != 24:
        raise RuntimeError("the fused prologue is the 3x3 / K=8 / offset geometry (off_aff_dec0 -> 24 channels)")
    if affinity not in _lib.AFF_KINDS:
        raise NotImplementedError(affinity)
    weights = (weights or HeadWeights()).get(oa, idc, cfc, precision)
    B, C, H, W = fe1.shape
    srcs = _sources(fe1, off_aff_fd1, id_fd1, cf_fd1,
                    lambda n, t, shape: f"{n} must be a float32 CUDA tensor of shape {shape}")
    if preserve_input and (dep is None or tuple(dep.shape) != (B, 1, H, W)):
        raise RuntimeError("preserve_input requires dep of shape (B, 1, H, W)")
    dep = None if dep is None else dep.contiguous().float()
    g = _lib.gamma_f32(gamma)
    dev = fe1.device
    e = lambda c: torch.empty((B, c, H, W), dtype=torch.float32, device=dev)  # noqa: E731
    out = {"pred_init": e(1), "offset": e(18), "aff": e(9), "confidence": e(1) if cf_fd1 is not None else None,
           "p0": e(1)}
    _lib.call(entry, dev, _lib.DTYPE_F32, *srcs, weights.wm, weights.wv, weights.bias, dep, g,
              out["pred_init"], out["confidence"], out["aff"], out["offset"], out["p0"],
              B, C, H, W, 3, 3, _lib.AFF_KINDS[affinity], _lib.flags(preserve_input, always_clip), _lib.STREAM)
    stats[precision] += 1
    return out
