"""CPU: the "problem too large" refusals of nlspn_gconv_x3_dgrad are reached with arguments alone
(sizes beyond the limit, dummy non-null pointers) and answer NLSPN_EINVAL with their message
before any device call, as tests/test_capi_guards_cpu.py holds for the other entries.

The kernel reaches the gradient's cells of one image through a 32-bit buffer offset
(nb0 * Hg * Wg * 16 bytes, nb0 the cell blocks: two per eight channels) and the workgroups
through a 32-bit grid index; the guard keeps both in range.  These tests run only where no GPU is
visible: there a guard that failed to fire ends in a HIP "no device" error (NLSPN_EHIP), not in a
launch on made-up pointers.
"""
import ctypes

import pytest
import torch

from nlspn_eccv20_amd import _lib

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="guards are probed with dummy pointers: no GPU may be visible")

P = ctypes.c_void_p(16)  # never dereferenced: the guard refuses first
G = 4096                 # 64 channels of 4096 x 2048 as c8x2: 16 cell blocks x 2^23 cells x 16 bytes = 2^31
MSG = "gconv_x3 dgrad: problem too large"


def _call(layer, cg, Hg, Wg, cout, Ho, Wo, B=1):
    lib = _lib.get()
    rc = lib.nlspn_gconv_x3_dgrad(layer, P, cg, P, None, None, None, P, None, cout, None, B, Hg, Wg, cout, Ho, Wo, 0, 1.0, None)
    return rc, lib.nlspn_last_error().decode()


@pytest.mark.parametrize("layer,hg,wg,ho,wo", [
    (80, G, G // 2, 2 * G, G),      # NLSPN_GCX3_DG_T2
    (82, G, G // 2, G // 2, G // 4),  # NLSPN_GCX3_DG_S2
    (83, G, G // 2, G, G // 2),     # NLSPN_GCX3_DG_S1
])
def test_gradient_past_the_buffer_descriptor(layer, hg, wg, ho, wo):
    rc, err = _call(layer, 64, hg, wg, 64, ho, wo)
    assert rc == _lib.EINVAL and MSG in err, (rc, err)


def test_one_row_less_passes_the_guard():
    rc, err = _call(83, 64, G - 1, G // 2, 64, G - 1, G // 2)
    assert rc == _lib.EHIP and "too large" not in err, (rc, err)  # past every guard: the launch finds no device


def test_grid_too_large():
    # 2^31 workgroups: 2^15 co tiles x 2^16 images of one 1 x 1 tile
    rc, err = _call(83, 24, 1, 1, 64 << 15, 1, 1, B=1 << 16)
    assert rc == _lib.EINVAL and MSG in err, (rc, err)
