"""CPU: every "too large" refusal of the C ABI is reached with arguments alone (sizes beyond the
limit, dummy non-null pointers) and answers NLSPN_EINVAL with its message before any device call.

The kernels address WITHIN one batch item (or one image's channels of a source) with 32-bit
buffer offsets and reach the item through a 64-bit base, b * stride.  The guards below are what
keeps the 32-bit part in range; tests/test_gpu_big_offsets.py holds the 64-bit part.

These tests run only where no GPU is visible: there a guard that failed to fire ends in a HIP
"no device" error (NLSPN_EHIP), not in a launch on made-up pointers.

Batch strides: check_item_bytes bounds the dense item H * W * (3K + 4) * es.  A caller's batch
stride may exceed the dense one (a padded item); that is safe without a stride term in the guard,
because no kernel multiplies a stride into a 32-bit offset: every use is
``static_cast<const T *>(p) + (long long)b * stride`` (nlspn_step.h, nlspn_resident.h,
nlspn_backward.h, nlspn_bwd_resident.h, nlspn_affnorm.h), and the 32-bit offsets behind that base
are plane * H * W * es + pixel * es <= the dense item.  test_padded_stride_passes_the_guard pins the
host side of it: a stride of 2^40 elements is accepted.
"""
import ctypes

import pytest
import torch

from nlspn_eccv20_amd import _lib

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="guards are probed with dummy pointers: no GPU may be visible")

P = ctypes.c_void_p(16)  # never dereferenced: the guard refuses first
H, W = 8192, 4096        # 2^25 pixels: (3 * 8 + 4) planes of f32 are 3.76e9 bytes
HW = H * W
ITEM = "image too large: one batch item's planes must stay below 2 GiB"


def _lib_call(name, *args):
    lib = _lib.get()
    rc = getattr(lib, name)(*args)
    return rc, lib.nlspn_last_error().decode()


def _refused(name, msg, *args):
    rc, err = _lib_call(name, *args)
    assert rc == _lib.EINVAL and msg in err, (name, rc, err)


# ------------------------------------------------------------------ check_item_bytes
def _step(dtype, h, w, B=1, aff_bs=None, off_bs=None):
    return ("nlspn_prop_step", dtype, P, None, P, P, 9 * h * w if aff_bs is None else aff_bs, P,
            16 * h * w if off_bs is None else off_bs, 1, P, None, B, h, w, 3, 3, 1, None)


def test_item_bytes_forward():
    _refused(_step(0, H, W)[0], ITEM, *_step(0, H, W)[1:])
    _refused("nlspn_propagate", ITEM, 0, P, P, P, P, 8 * HW, P, 16 * HW, P, P, P, P, None, P, P, 1, H, W, 3, 3, 3, 3, 1, None)
    _refused("nlspn_propagate_normalized", ITEM, 0, P, P, P, P, P, P, P, P, 1, H, W, 3, 3, 3, 1, None)
    # f16 storage: twice the pixels
    _refused("nlspn_propagate", ITEM, 1, P, P, P, P, 16 * HW, P, 32 * HW, P, P, P, P, None, P, P, 1, 2 * H, W, 3, 3, 3, 3, 1,
             None)


def test_item_bytes_backward_and_step_backward():
    _refused("nlspn_propagate_backward", ITEM, 0, P, P, P, P, 8 * HW, P, 16 * HW, P, P, P, P, P, P, P, P, P, 0, P, 0, P, P,
             1, H, W, 3, 3, 3, 3, 1, None)
    _refused("nlspn_prop_step_backward", ITEM, 0, P, P, P, P, 9 * HW, P, 16 * HW, P, P, P, P, P, P, 1, H, W, 3, 3, 1, None)


@pytest.mark.parametrize("dtype,es", [(0, 4), (1, 2)])
def test_item_bytes_boundary(dtype, es):
    """The last width that fits and the first that does not: 28 planes of w pixels against 2^31 - 1."""
    w = (2 ** 31 - 1) // (28 * es)
    rc, err = _lib_call(*_step(dtype, 1, w))
    assert rc == _lib.EHIP and "too large" not in err, (rc, err)  # past every guard: the launch finds no device
    rc, err = _lib_call(*_step(dtype, 1, w + 1))
    assert rc == _lib.EINVAL and ITEM in err, (rc, err)


def test_padded_stride_passes_the_guard():
    rc, err = _lib_call(*_step(0, 8, 64, B=2, aff_bs=1 << 40, off_bs=1 << 40))
    assert rc == _lib.EHIP and "too large" not in err, (rc, err)


def test_grid_too_large():
    """2^30 + 1 images of two 4 x 64 tile rows: more workgroups than a grid dimension holds."""
    a = _step(0, 8, 64, B=(1 << 30) + 1)
    _refused(a[0], "grid too large", *a[1:])
    rc, err = _lib_call(*_step(0, 4, 64, B=(1 << 31) - 1))  # one tile per image: 2^31 - 1 fit
    assert rc == _lib.EHIP and "too large" not in err, (rc, err)


# ------------------------------------------------------------------ heads and S2D
B30 = 1 << 30


def test_input_too_large_heads_and_s2d():
    msg = "input too large"
    # 2^30 images of two 8 x 32 tiles
    _refused("nlspn_head_epilogue", msg, 0, P, P, P, P, P, P, P, P, P, P, B30, 16, 16, 32, 24, None)
    _refused("nlspn_head_epilogue_prologue", msg, 0, P, P, P, P, P, P, P, P, P, P, P, P, P, P, B30, 16, 16, 32, 3, 3, 3, 1, None)
    _refused("nlspn_head_epilogue_x3", msg, 0, P, P, P, P, P, P, P, P, P, P, B30, 16, 16, 32, 24, None)
    _refused("nlspn_head_epilogue_prologue_x3", msg, 0, P, P, P, P, P, P, P, P, P, P, P, P, P, P, B30, 16, 16, 32, 3, 3, 3, 1,
             None)
    # the split-bf16 kernel's 16 planes of a round: H * W below 2^25
    _refused("nlspn_head_epilogue_x3", msg, 0, P, P, P, P, P, P, P, P, P, P, 1, 16, H, W, 24, None)
    _refused("nlspn_head_epilogue_prologue_x3", msg, 0, P, P, P, P, P, P, P, P, P, P, P, P, P, P, 1, 16, H, W, 3, 3, 3, 1, None)
    # 2^30 images of two 16 x 64 tiles
    _refused("nlspn_s2d_pyramid", msg, 0, P, P, P, P, P, P, None, B30, 32, 64, None)


# ------------------------------------------------------------------ GRU-mode convolutions
G = 4096  # 64 channels of 4096 x 4096 f32: 2^32 bytes in one image of a source


@pytest.mark.parametrize("layer,c,cout,ho,hc", [
    (0, 64, 64, G // 2, 0),      # NLSPN_GC_S2
    (4, 64, 64, 2 * G, 0),       # NLSPN_GC_T2
    (3, 128, 128, G, 128),       # NLSPN_GC_GRU2
])
def test_gconv_too_large(layer, c, cout, ho, hc):
    _refused("nlspn_gconv", "gconv: problem too large", layer, P, c, None, 0, P, P, P, P, P, P, P, P, 1, G, G, cout, ho, ho, 0,
             1.0, hc, None)


def test_gconv16_and_x3_too_large():
    _refused("nlspn_gconv16", "gconv16: problem too large", 48, P, 64, None, 0, P, P, P, None, None, None, None, None, None,
             None, 1, 2 * G, 2 * G, 64, G, G, 0, 1.0, 0, None)
    _refused("nlspn_gconv_x3", "gconv_x3: problem too large", 64, P, 64, None, 0, P, P, P, None, None, None, None, None, None,
             None, 1, 2 * G, G, 64, G, G // 2, 0, 1.0, 0, None)


@pytest.mark.parametrize("layer,ho", [(32, 2 * G), (36, G)])  # NLSPN_GC_DG_T2, NLSPN_GC_DG_S1
def test_gconv_dgrad_too_large(layer, ho):
    _refused("nlspn_gconv_dgrad", "gconv dgrad: problem too large", layer, P, 64, P, None, None, None, P, None, 64, 1, G, G,
             64, ho, ho, 0, 1.0, None)


def test_gconv_wgrad_too_large():
    msg = "gconv wgrad: problem too large"
    many = (1, P, 64, P, 64, None, 0, P, None, 0, 1.0, P, 1 << 62, 1 << 20, 1 << 11, 64, 1 << 11, 64, None)  # 2^31 row units
    _refused("nlspn_gconv_wgrad", msg, *many)
    _refused("nlspn_gconv_wgrad_bf16x3", msg, *many)
    _refused("nlspn_gconv_wgrad_narrow", msg, 2, P, 16, P, 16, None, 0, P, None, 0, 1.0, P, 1 << 62, 1 << 20, 1 << 11, 64,
             1 << 12, 128, None)
    lib = _lib.get()
    assert lib.nlspn_gconv_wgrad_workspace_bytes(1, 64, 64, 1 << 20, 1 << 11, 64, 1 << 11, 64) == 0
    # the split-bf16 kernel's 32-bit staging offsets: a plane of 2^28 pixels
    _refused("nlspn_gconv_wgrad_bf16x3", msg, 1, P, 64, P, 64, None, 0, P, None, 0, 1.0, P, 1 << 62, 1, 1 << 14, 1 << 14,
             1 << 14, 1 << 14, None)
