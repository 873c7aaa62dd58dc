"""GPU: the host wrappers' argument errors, characterised.  Every wrapper checks
``is_cuda`` first, so its other messages are reachable only with device tensors.
tests/golden/host_errors.json holds, per case of the table below, the exception class
and the full message text, recorded from the wrappers as they were before their C-ABI
calls were routed through ``_lib.call``: a change of the host layer must leave every
one of them as it is.

Every case raises before a propagation / convolution launch (the ``head_epilogue``
source-shape case first packs the head weights, one small launch).  Tensors are
B=2, H=8, W=12, K=8.  The DCN backward has no offset / mask shape check of its own (it
sizes its outputs from them), so those two cases exist for the forward only.
"""
import json
import os

import pytest
import torch
import torch.nn as nn

from nlspn_eccv20_amd import (affinity_normalization, dcn, prop_step, propagate, propagate_normalized)
from nlspn_eccv20_amd.heads import head_epilogue, head_epilogue_prologue
from nlspn_eccv20_amd.s2d import s2d_front

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, H, W, K = 2, 8, 12, 8

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "host_errors.json")) as _f:
    GOLDEN = {c["id"]: c for c in json.load(_f)}


def _t(*shape, dtype=torch.float32):
    return torch.rand(shape, device=DEV).to(dtype)


def _strided(*shape):
    """A (B, 1, H, W) slice of a 2-channel tensor: contiguous planes, not contiguous."""
    return _t(shape[0], 2, *shape[2:])[:, :1]


def build_cases():
    """{case id: thunk raising the characterised error}."""
    cases = {}

    # ------------------------------------------------------------- propagate
    def prop(**kw):
        a = dict(pred_init=_t(B, 1, H, W), dep=_t(B, 1, H, W), confidence=_t(B, 1, H, W), aff=_t(B, K, H, W),
                 offset=_t(B, 2 * K, H, W), gamma=torch.tensor([4.0], device=DEV))
        opts = dict(prop_time=2)
        for k, v in kw.items():
            (a if k in a else opts)[k] = v
        return lambda: propagate(*a.values(), **opts)

    cases["propagate/aff_channels"] = prop(aff=_t(B, K - 1, H, W))
    cases["propagate/pred_init_noncontiguous"] = prop(pred_init=_strided(B, 1, H, W))
    cases["propagate/dep_dtype"] = prop(dep=_t(B, 1, H, W, dtype=torch.float16))
    cases["propagate/preserve_input_without_dep"] = prop(dep=None)
    cases["propagate/unknown_affinity"] = prop(affinity="XYZ")
    cases["propagate/even_kernel"] = prop(kernel=(2, 2))
    cases["propagate/fp64"] = prop(**{k: _t(B, c, H, W, dtype=torch.float64) for k, c in
                                      (("pred_init", 1), ("dep", 1), ("confidence", 1), ("aff", K),
                                       ("offset", 2 * K))})
    # rejected by the C ABI (NlspnError), through the wrapper
    cases["propagate/9x9_no_instantiation"] = prop(kernel=(9, 9), aff=_t(B, 80, H, W), offset=_t(B, 160, H, W))

    # ------------------------------------------------------------- prop_step (out= : the ctypes mirror)
    def step(**kw):
        a = dict(feat=_t(B, 1, H, W), confidence=_t(B, 1, H, W), dep=_t(B, 1, H, W), aff=_t(B, K + 1, H, W),
                 offset=_t(B, 2 * (K + 1), H, W))
        opts = dict(out=_t(B, 1, H, W))
        for k, v in kw.items():
            (a if k in a else opts)[k] = v
        return lambda: prop_step(*a.values(), **opts)

    cases["prop_step/offset_channels_inserted"] = step(offset=_t(B, 2 * K, H, W))
    cases["prop_step/offset_channels_raw"] = step(offset_layout="raw")
    cases["prop_step/confidence_noncontiguous"] = step(confidence=_strided(B, 1, H, W))

    # ------------------------------------------------------------- propagate_normalized / affinity_normalization
    cases["propagate_normalized/aff_planes"] = lambda: propagate_normalized(
        _t(B, 1, H, W), _t(B, 1, H, W), _t(B, 1, H, W), _t(B, K, H, W), _t(B, 2 * (K + 1), H, W), prop_time=2)
    cases["affinity_normalization/gamma_not_tensor"] = lambda: affinity_normalization(_t(B, K, H, W), 4.0)

    # ------------------------------------------------------------- dcn
    def dcn_args(backward, **kw):
        C, Cout = 4, 6
        a = dict(input=_t(B, C, H, W), weight=_t(Cout, C, 3, 3), bias=_t(Cout), offset=_t(B, 18, H, W),
                 mask=_t(B, 9, H, W))
        if backward:
            a["grad_output"] = _t(B, Cout, H, W)
        a.update(kernel_h=3, kernel_w=3, stride_h=1, stride_w=1, pad_h=1, pad_w=1, dilation_h=1, dilation_w=1,
                 group=1, deformable_group=1, im2col_step=64)
        assert set(kw) <= set(a)
        a.update(kw)
        fn = dcn.modulated_deform_conv_backward if backward else dcn.modulated_deform_conv_forward
        return lambda: fn(*a.values())

    for name, bwd in (("dcn_forward", False), ("dcn_backward", True)):
        cases[f"{name}/kernel_vs_weight"] = dcn_args(bwd, kernel_h=5)
        cases[f"{name}/channels_vs_group"] = dcn_args(bwd, group=2)
        cases[f"{name}/mixed_dtype"] = dcn_args(bwd, offset=_t(B, 18, H, W, dtype=torch.float16))
    cases["dcn_forward/offset_shape"] = dcn_args(False, offset=_t(B, 16, H, W))
    cases["dcn_forward/mask_shape"] = dcn_args(False, mask=_t(B, 8, H, W))
    cases["dcn_backward/group_divisibility"] = dcn_args(True, group=4)
    cases["dcn_backward/grad_output_batch"] = dcn_args(True, grad_output=_t(B + 1, 6, H, W))
    cases["dcn_backward/grad_output_channels"] = dcn_args(True, grad_output=_t(B, 5, H, W))
    cases["dcn_backward/grad_output_shape"] = dcn_args(True, grad_output=_t(B, 6, H - 1, W))

    # ------------------------------------------------------------- heads
    C = 16
    conv = lambda nout: nn.Conv2d(2 * C, nout, 3, padding=1).to(DEV)  # noqa: E731
    oa, idc = conv(24), conv(1)
    fe1, fd = _t(B, C, H, W), _t(B, C, H, W)
    cases["head_epilogue/conv_without_decoder_output"] = lambda: head_epilogue(fe1, fd, oa, None, idc)
    cases["head_epilogue/source_shape"] = lambda: head_epilogue(fe1, fd, oa, _t(B, C, H, W + 1), idc)
    cases["head_epilogue_prologue/off_aff_channels"] = lambda: head_epilogue_prologue(
        fe1, fd, conv(16), fd, idc, _t(B, 1, H, W), torch.tensor([4.0], device=DEV))

    # ------------------------------------------------------------- s2d
    w1, b1, w2, b2 = _t(8, 6, 1, 1), _t(8), _t(16, 8, 1, 1), _t(16)
    cases["s2d_front/two_channel_dep"] = lambda: s2d_front(_t(B, 2, H, W), w1, b1, w2, b2)
    cases["s2d_front/pool_convs_shapes"] = lambda: s2d_front(_t(B, 1, H, W), _t(8, 5, 1, 1), b1, w2, b2)
    return cases


def run_case(thunk):
    """(exception class name, message) of a case; the generator of the golden file uses it too."""
    with torch.no_grad():
        try:
            thunk()
        except Exception as e:  # noqa: BLE001
            return type(e).__name__, str(e)
    return None, None


@pytest.fixture(scope="module")
def cases():
    return build_cases()


def test_case_table_matches_golden(cases):
    assert sorted(cases) == sorted(GOLDEN) and len(cases) >= 30


@pytest.mark.parametrize("case_id", sorted(GOLDEN))
def test_host_error(cases, case_id):
    got = run_case(cases[case_id])
    print(case_id, got)
    assert got == (GOLDEN[case_id]["exception"], GOLDEN[case_id]["message"])
