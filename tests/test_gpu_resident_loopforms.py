"""GPU: the two forms of the resident kernel's iteration loop (nlspn_resident.h
prop_resident_kernel COPY).  A launch whose main waves copy nothing (the helper launch, the
default) runs the build without the loop's copy code; NLSPN_RES_HELPER=0 runs the build with it.

Bar: BIT-EXACT on all five outputs (pred, every pred_inter, aff, offset, confidence) between the
helper launch (COPY = false), the launch under NLSPN_RES_HELPER=0 (COPY = true) and the
per-iteration step launches (NLSPN_RESIDENT=0), with the build (quad-owning threads) and the
helper choice asserted through nlspn_resident_config / nlspn_resident_helper.

Shapes: the smallest that still hand off across parts on a thread-per-quad build, through
NLSPN_RES_GRID (NLSPN_RES_SPLIT=0 keeps a thread per quad): 256 quads per part (the run-time
thread-count build), 576 (the 576-thread build), C3's two image groups (the GROUPS build), and
fp16.  T: 2 has no poison store, 3 has one, 5 is the general case with the leftover offset planes
copied at T - 1, 20 is longer than the 2(K+1) offset planes.  3x3 taps, learned offsets (the
strided [:, :2K] slice of the head tensor), preserve_input, TGASS.
"""
import contextlib
import ctypes
import os

import numpy as np
import pytest
import torch

from nlspn_eccv20_amd import PropagationPlan, _lib, propagate
from nlspn_eccv20_amd.synthetic import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OUTS = ("pred", "pred_inter_tensor", "offset", "aff", "confidence")
F32, F16 = torch.float32, torch.float16
K = 8


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    for k, v in kv.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _helper(B, H, W, dtype, T):
    """(helper form selected, threads per workgroup of the first resident launch)"""
    blk = ctypes.c_int()
    ok = _lib.get().nlspn_resident_helper(0 if dtype == F32 else 1, B, H, W, 3, 3, T, 1, 1, ctypes.byref(blk))
    return bool(ok), blk.value


def _block(B, H, W, dtype, T):
    """the planner's quad-owning threads (nlspn_resident_config's block)"""
    b = ctypes.c_int()
    assert _lib.get().nlspn_resident_config(0 if dtype == F32 else 1, B, H, W, 3, 3, T, 1, None, ctypes.byref(b), None)
    return b.value


def _inputs(B, H, W, dtype=F32, seed=3):
    s = synth(B, H, W, K, seed=seed, off_sigma=2.0, density=0.05)
    cu = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV, dtype)  # noqa: E731
    oa = cu(s["off_aff"])
    return (cu(s["pred_init"]), cu(s["dep"]), cu(s["conf"]), oa[:, 2 * K:], oa[:, :2 * K], torch.tensor([4.0], device=DEV))


_shared = {}


def _cached(B, H, W, dtype=F32):
    """inputs computed once per shape and shared (never written by a test)"""
    key = (B, H, W, dtype)
    if key not in _shared:
        _shared[key] = _inputs(B, H, W, dtype=dtype)
    return _shared[key]


def _bits_equal(x, y):
    it = torch.int32 if x.dtype == F32 else torch.int16
    return x.dtype == y.dtype and x.shape == y.shape and torch.equal(x.contiguous().view(it), y.contiguous().view(it))


def _same(a, b, what):
    for k in OUTS:
        assert a[k] is not None and b[k] is not None and _bits_equal(a[k], b[k]), (what, k)


def _check(B, H, W, T, nt, grid, dtype=F32):
    inp = _cached(B, H, W, dtype)
    with _env(NLSPN_RES_GRID=grid, NLSPN_RES_SPLIT="0", NLSPN_RESIDENT="1", NLSPN_RES_HELPER=None):
        assert _block(B, H, W, dtype, T) == nt
        assert _helper(B, H, W, dtype, T) == (True, nt + 64)
        a = propagate(*inp, prop_time=T)
        with _env(NLSPN_RES_HELPER="0"):
            assert _helper(B, H, W, dtype, T) == (False, nt)
            h = propagate(*inp, prop_time=T)
        with _env(NLSPN_RESIDENT="0"):
            assert _helper(B, H, W, dtype, T) == (False, 0)
            s = propagate(*inp, prop_time=T)
    torch.cuda.synchronize()
    _lib.check_resident()  # no launch aborted
    assert a["offset"].shape[1] == 2 * (K + 1)
    _same(a, h, "no-copy loop (helper launch) vs the loop with the copy")
    _same(a, s, "no-copy loop (helper launch) vs the step launches")


@pytest.mark.parametrize("T", [2, 3, 5, 20])
def test_run_time_thread_count_build(T):
    """B = 2, 32 x 128 in 2 x 2 parts of 16 x 16 = 256 quads: the build that reads its thread
    count at run time."""
    _check(2, 32, 128, T, 256, "2,2")


@pytest.mark.parametrize("T", [2, 3, 5, 20])
def test_576_thread_build(T):
    """B = 1, 48 x 192 in 2 x 2 parts of 24 x 24 = 576 quads: C2's build."""
    _check(1, 48, 192, T, 576, "2,2")


def test_group_loop_build():
    """C3's shape: two image groups in one launch of the 576-thread GROUPS build; the loop form is
    the same for both groups."""
    _check(4, 240, 1216, 5, 576, None)


@pytest.mark.parametrize("T", [3, 5])
def test_fp16(T):
    """fp16 storage in C2's build (the LDS row rewrite after iteration 1 sits in both loop forms)."""
    _check(1, 48, 192, T, 576, "2,2", dtype=F16)


def test_plan_replays_alternating_inputs_no_stale_reads():
    """A plan of the no-copy loop replayed over inputs refilled in place from two data sets in
    turn: every output is that replay's (no cell of the previous replay's planes is read), and no
    launch aborted."""
    T = 5
    ia, ib = _cached(1, 48, 192), _inputs(1, 48, 192, seed=32)
    with _env(NLSPN_RES_GRID="2,2", NLSPN_RES_SPLIT="0", NLSPN_RES_HELPER=None):
        with _env(NLSPN_RESIDENT="0"):
            ra = {k: v.clone() for k, v in propagate(*ia, prop_time=T).items() if k in OUTS}
            rb = {k: v.clone() for k, v in propagate(*ib, prop_time=T).items() if k in OUTS}
        buf = [x.clone() for x in ia]
        oa = torch.empty(1, 3 * K, 48, 192, device=DEV)  # the head tensor: aff and offset are its slices
        buf[3], buf[4] = oa[:, 2 * K:], oa[:, :2 * K]
        with _env(NLSPN_RESIDENT="1"):
            assert _helper(1, 48, 192, F32, T) == (True, 640)
            plan = PropagationPlan(*buf, prop_time=T)
        for i in range(6):
            src, ref = (ia, ra) if i % 2 == 0 else (ib, rb)
            for d, x in zip(buf, src):
                d.copy_(x)
            o = plan.replay()
            torch.cuda.synchronize()
            _same(o, ref, f"replay {i}")
        plan.check()
        plan.close()
