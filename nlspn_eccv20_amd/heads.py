"""Head epilogue on the HIP kernel: the decoder's last three 3x3
convolutions as one kernel.

Reference: src/model/nlspnmodel.py:296-315 —
    pred_init  = id_dec0(cat(id_fd1, fe1))        ReLU      (:297, id_dec0 :68)
    off_aff    = off_aff_dec0(cat(off_aff_fd1, fe1))         (:301, off_aff_dec0 :74/:76)
    confidence = cf_dec0(cat(cf_fd1, fe1))        Sigmoid   (:313, cf_dec0 :83-86)
``head_epilogue`` reads fe1 and the three decoder outputs in place (no concatenated
copies) and computes all three convolutions with bias and activation in one launch
(``nlspn_head_epilogue``, ``csrc/nlspn_heads.h``): f32 operands on the matrix cores,
exact f32 products, f32 accumulation.  The model calls it when gradients are off; training
keeps the torch convolutions unless ``NLSPNModel.native_head_train`` is set (below).

The three convolutions' weights are packed once per weight version into the kernel's
layout (``nlspn_head_pack_weights``) and cached on the module.

``precision="bf16x3"`` (opt-in; default ``"fp32"``) runs the same epilogues on the bf16
matrix cores with every f32 MFMA operand split into two bf16 parts
(``nlspn_head_epilogue_x3``, ``csrc/nlspn_heads_x3.h``): weights split when packed, fe1 and
off_aff_fd1 while staged, three products per term (lo lo dropped), f32 accumulation; the
one-channel id / cf decoder halves, bias, activations and the fused prologue are the f32
kernel's code.  ``stats`` counts the launches per precision.

Training (opt-in: ``head_epilogue(..., differentiable=True)``, ``NLSPNModel.native_head_train``).
Under gradients the same f32 launch is the forward of a ``torch.autograd.Function``
(``_HeadFn``): it saves the four sources, ``pred_init`` and ``conf`` (no concatenated copies)
and its backward issues (``csrc/nlspn_heads_bwd.h``)
  * ``nlspn_head_backward_pre``: the pre-activation gradient ``gpre`` (B, nout + 2, H, W), rows
    in the forward kernel's column order (off_aff, id, cf), the ReLU mask and the sigmoid
    derivative taken from the saved outputs;
  * the two wide data gradients (fe1, off_aff_fd1) as one launch of the stride-1 adjoint
    preset of the GRU-mode convolutions (``nlspn_gconv_dgrad(GC_DG_S1, ...)``) on the stacked
    weight packed by ``gru.pack_adjoint_s1``, cached in ``HeadWeights``;
  * ``nlspn_head_dgrad_single``: the one-row adjoints into id_fd1 / cf_fd1 on the VALU;
  * ``nlspn_head_wgrad``: dW / db of the three modules, an f32 matrix-core implicit GEMM over
    pixels cut into slices whose slabs further launches sum in a fixed order (no atomics:
    bit-reproducible).
``ctx.needs_input_grad`` skips the data-gradient or the weight-gradient launches nobody needs;
``train_stats`` counts the launches.  f32 only: ``precision="bf16x3"`` with a
gradient-requiring differentiable call raises.
"""
from __future__ import annotations

import ctypes

import torch
import torch.nn as nn

from . import _lib

__all__ = ["head_epilogue", "head_epilogue_prologue", "HeadWeights", "PRECISIONS", "stats", "train_stats"]

PRECISIONS = ("fp32", "bf16x3")
# kernel launches per precision (epilogue and fused-prologue entries alike), so a test can prove
# which kernel ran
stats = {"fp32": 0, "bf16x3": 0}
# launches of the differentiable path's backward per piece: pre (nlspn_head_backward_pre), dgrad
# (the wide data gradients' nlspn_gconv_dgrad), dgrad_single, wgrad (nlspn_head_wgrad calls)
train_stats = {"pre": 0, "dgrad": 0, "dgrad_single": 0, "wgrad": 0}
_GC_DG_S1 = 36  # NLSPN_GC_DG_S1
_ws = {}  # (device, stream) -> the weight-gradient workspace
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


class _Adjoint:
    __slots__ = ("key", "wadj")


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

    def adjoint(self, oa, idc, cfc) -> torch.Tensor:
        """The wide data gradients' weights of this device: the stacked (nout + 2, 2C, 3, 3)
        weight (rows off_aff_dec0, id_dec0, cf_dec0; the decoder halves of the id / cf rows
        zeroed, an absent head's row zero) packed by gru.pack_adjoint_s1, cached under get()'s
        (pointer, version) key rule."""
        from .gru import pack_adjoint_s1

        ws = [c.weight for c in (oa, idc, cfc) if c is not None]
        key = (tuple((t.data_ptr(), t._version) for t in ws), idc is None, cfc is None)
        dev = oa.weight.device
        e = self._entries.get((dev, "adjoint"))
        if e is not None and e.key == key:
            return e.wadj
        C, nout = oa.in_channels // 2, oa.out_channels
        with torch.no_grad():
            wst = torch.zeros((nout + 2, 2 * C, 3, 3), dtype=torch.float32, device=dev)
            wst[:nout] = oa.weight.detach()
            for k, c in enumerate((idc, cfc)):
                if c is not None:
                    wst[nout + k, C:] = c.weight.detach()[0, C:]
            e = _Adjoint()
            e.key, e.wadj = key, pack_adjoint_s1(wst)
        self._entries[(dev, "adjoint")] = e
        return e.wadj


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


def _launch(entry, precision, weights, srcs, B, C, H, W):
    """The head-epilogue launch on contiguous sources: (pred_init, off_aff, conf)."""
    fe1, _, id_fd1, cf_fd1 = srcs
    dev = fe1.device
    off_aff = torch.empty((B, weights.nout, H, W), dtype=torch.float32, device=dev)
    pred_init = torch.empty((B, 1, H, W), dtype=torch.float32, device=dev) if id_fd1 is not None else None
    conf = torch.empty((B, 1, H, W), dtype=torch.float32, device=dev) if cf_fd1 is not None else None
    _lib.call(entry, dev, _lib.DTYPE_F32, *srcs, weights.wm, weights.wv, weights.bias, off_aff,
              pred_init, conf, B, C, H, W, weights.nout, _lib.STREAM)
    stats[precision] += 1
    return pred_init, off_aff, conf


def _workspace(dev, need):
    key = (dev, torch.cuda.current_stream(dev).cuda_stream)
    ws = _ws.get(key)
    if ws is None or ws.numel() * 4 < need:
        ws = _ws[key] = torch.empty((need + 3) // 4, device=dev, dtype=torch.float32)
    return ws


class _HeadFn(torch.autograd.Function):
    """The head epilogue under autograd: the f32 inference launch forward, the pieces of
    csrc/nlspn_heads_bwd.h backward.  Inputs: the four sources (id_fd1 / cf_fd1 may be None),
    then weight, bias of off_aff_dec0, id_dec0, cf_dec0 (None for an absent head)."""

    @staticmethod
    def forward(ctx, packed, cache, convs, fe1, fd_oa, fd_id, fd_cf, *params):
        B, C, H, W = fe1.shape
        srcs = [fe1, fd_oa, fd_id, fd_cf]
        pred_init, off_aff, conf = _launch("nlspn_head_epilogue", "fp32", packed, srcs, B, C, H, W)
        ctx.cache, ctx.convs, ctx.nout = cache, convs, packed.nout
        ctx.set_materialize_grads(False)  # an unused output's gradient stays None: zero rows of gpre, no zeros tensor
        ctx.has = (fd_id is not None, fd_cf is not None)
        # (the weights too: autograd then refuses a backward after an in-place update of them)
        named = dict(zip(("fe1", "fd_oa", "fd_id", "fd_cf", "pred_init", "conf", "w_oa", "w_id", "w_cf"),
                         srcs + [pred_init, conf] + list(params[0::2])))
        ctx.names = [n for n, t in named.items() if t is not None]
        ctx.save_for_backward(*[named[n] for n in ctx.names])
        return tuple(t for t in (pred_init, off_aff, conf) if t is not None)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *gouts):
        has_id, has_cf = ctx.has
        saved = dict(zip(ctx.names, ctx.saved_tensors))
        fe1, fd_oa, fd_id, fd_cf, pred_init, conf, w_id, w_cf = (
            saved.get(n) for n in ("fe1", "fd_oa", "fd_id", "fd_cf", "pred_init", "conf", "w_id", "w_cf"))
        gouts = list(gouts)
        g_pi = gouts.pop(0) if has_id else None
        g_oa = gouts.pop(0)
        g_cf = gouts.pop(0) if has_cf else None
        g_pi, g_oa, g_cf = (None if g is None else g.contiguous().float() for g in (g_pi, g_oa, g_cf))
        oa, idc, cfc = ctx.convs
        B, C, H, W = fe1.shape
        nout, dev = ctx.nout, fe1.device
        gpre = torch.empty((B, nout + 2, H, W), dtype=torch.float32, device=dev)
        _lib.call("nlspn_head_backward_pre", dev, g_oa, g_pi, g_cf, pred_init if g_pi is not None else None,
                  conf if g_cf is not None else None, gpre, B, H, W, nout, _lib.STREAM)
        train_stats["pre"] += 1
        need = ctx.needs_input_grad  # (packed, cache, convs, fe1, fd_oa, fd_id, fd_cf, w_oa, b_oa, w_id, b_id, w_cf, b_cf)
        d_fe1 = d_oa = d_id = d_cf = None
        if need[3] or need[4]:
            d_fe1, d_oa = torch.empty_like(fe1), torch.empty_like(fd_oa)
            wadj = (ctx.cache or HeadWeights()).adjoint(oa, idc, cfc)
            _lib.call("nlspn_gconv_dgrad", dev, _GC_DG_S1, gpre, nout + 2, wadj, None, None, None, d_oa, d_fe1, C, B, H, W,
                      2 * C, H, W, 0, 1.0, _lib.STREAM)
            train_stats["dgrad"] += 1
        want_id, want_cf = has_id and need[5], has_cf and need[6]
        if want_id or want_cf:
            d_id = torch.empty_like(fe1) if want_id else None
            d_cf = torch.empty_like(fe1) if want_cf else None
            _lib.call("nlspn_head_dgrad_single", dev, gpre, w_id.detach().contiguous() if want_id else None,
                      w_cf.detach().contiguous() if want_cf else None, d_id, d_cf, B, C, H, W, nout, _lib.STREAM)
            train_stats["dgrad_single"] += 1
        grads = [None] * 6
        if any(need[7:]):
            e = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)  # noqa: E731
            dw_oa, db_oa = e(nout, 2 * C, 3, 3), e(nout)
            dw_id, db_id = (e(1, 2 * C, 3, 3), e(1)) if has_id else (None, None)
            dw_cf, db_cf = (e(1, 2 * C, 3, 3), e(1)) if has_cf else (None, None)
            ws = _workspace(dev, _lib.get().nlspn_head_wgrad_workspace_bytes(B, C, H, W, nout))
            _lib.call("nlspn_head_wgrad", dev, gpre, fe1, fd_oa, fd_id, fd_cf, dw_oa, db_oa, dw_id, db_id, dw_cf, db_cf,
                      ws, ws.numel() * 4, B, C, H, W, nout, _lib.STREAM)
            train_stats["wgrad"] += 1
            grads = [g if n else None for g, n in zip((dw_oa, db_oa, dw_id, db_id, dw_cf, db_cf), need[7:])]
        return (None, None, None, d_fe1 if need[3] else None, d_oa if need[4] else None, d_id, d_cf, *grads)


def head_epilogue(fe1, off_aff_fd1, off_aff_dec0, id_fd1=None, id_dec0=None, cf_fd1=None, cf_dec0=None,
                  weights: HeadWeights | None = None, precision: str = "fp32", differentiable: bool = False):
    """(pred_init, off_aff, confidence) of nlspnmodel.py:297-315 from the decoder outputs.
    ``id_fd1``/``id_dec0`` and ``cf_fd1``/``cf_dec0`` may be None (that head is skipped
    and None returned for it).  ``precision``: "fp32" or "bf16x3" (module docstring).
    ``differentiable``: with gradients enabled and a source or parameter requiring grad, the
    call is recorded for autograd (_HeadFn: the same f32 launch, bit-equal outputs, the HIP
    backward); "bf16x3" then raises RuntimeError (its kernels are inference only).  False
    (default): the outputs carry no grad_fn, whatever the inputs require."""
    entry = _ENTRIES[_check_precision(precision)][2]
    oa, idc, cfc = _conv_of(off_aff_dec0), _conv_of(id_dec0), _conv_of(cf_dec0)
    if (id_fd1 is None) != (idc is None) or (cf_fd1 is None) != (cfc is None):
        raise RuntimeError("each head needs both its decoder output and its convolution")
    params = [t for c in (oa, idc, cfc) for t in ((None, None) if c is None else (c.weight, c.bias))]
    train = differentiable and torch.is_grad_enabled() and any(
        t is not None and t.requires_grad for t in [fe1, off_aff_fd1, id_fd1, cf_fd1] + params)
    if train and precision != "fp32":
        raise RuntimeError(f"head_epilogue: precision {precision!r} is inference only; the differentiable path is 'fp32'")
    cache = weights
    weights = (weights or HeadWeights()).get(oa, idc, cfc, precision)  # this device's packed entry
    B, C, H, W = fe1.shape
    if C != weights.C:
        raise RuntimeError(f"fe1 has {C} channels, the head convolutions expect {weights.C} + {weights.C}")
    srcs = _sources(fe1, off_aff_fd1, id_fd1, cf_fd1, lambda n, t, shape: (
        f"{n} must be a float32 CUDA tensor" if not t.is_cuda or t.dtype != torch.float32 else
        f"{n} must be {shape} (the _concat crop is done by the caller), got {tuple(t.shape)}"))
    if train:
        outs = list(_HeadFn.apply(weights, cache, (oa, idc, cfc), *srcs, *params))
        pred_init = outs.pop(0) if id_fd1 is not None else None
        off_aff = outs.pop(0)
        return pred_init, off_aff, (outs.pop(0) if cf_fd1 is not None else None)
    return _launch(entry, precision, weights, srcs, B, C, H, W)


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
