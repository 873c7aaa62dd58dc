"""GPU: the resident kernel's helper wave (nlspn_resident.h kResHelper).  The builds that
copied the output dict's inserted offsets in their iteration loop launch one more wave, which
owns no quad and copies them instead.

Bar: BIT-EXACT on all five outputs (pred, pred_inter_tensor, offset, aff, confidence) against
the same launch without the helper (NLSPN_RES_HELPER=0) and against the per-iteration step
launches (NLSPN_RESIDENT=0), and the helper form asserted selected (and not selected under the
switch) through nlspn_resident_helper.  Small shapes reach the builds of the bench configs
through NLSPN_RES_GRID; every case passes the raw offsets as the strided [:, :2K] slice of the
(B, 3K, H, W) head tensor.
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


def _helper(B, H, W, dtype=F32, conf=True, T=18, kernel=(3, 3), off_out=True):
    """(helper form selected, threads per workgroup of the first resident launch)"""
    blk = ctypes.c_int()
    ok = _lib.get().nlspn_resident_helper(0 if dtype == F32 else 1, B, H, W, kernel[0], kernel[1], T, int(conf),
                                          int(off_out), ctypes.byref(blk))
    return bool(ok), blk.value


def _block(B, H, W, dtype=F32, conf=True, T=18, kernel=(3, 3)):
    """the planner's quad-owning threads (nlspn_resident_config's block)"""
    b = ctypes.c_int()
    ok = _lib.get().nlspn_resident_config(0 if dtype == F32 else 1, B, H, W, kernel[0], kernel[1], T, int(conf), None,
                                          ctypes.byref(b), None)
    assert ok
    return b.value


def _inputs(B, H, W, sigma=2.0, seed=3, dtype=F32, K=8):
    s = synth(B, H, W, K, seed=seed, off_sigma=sigma, density=0.05)
    cu = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV, dtype)  # noqa: E731
    oa = cu(s["off_aff"])
    return (cu(s["pred_init"]), cu(s["dep"]), cu(s["conf"]), oa[:, 2 * K:], oa[:, :2 * K], torch.tensor([4.0], device=DEV))


def _bits_equal(x, y):
    it = torch.int32 if x.dtype == F32 else torch.int16
    return x.dtype == y.dtype and x.shape == y.shape and torch.equal(x.contiguous().view(it), y.contiguous().view(it))


def _same(a, b, what):
    for k in OUTS:
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, (what, k)
        else:
            assert _bits_equal(a[k], b[k]), (what, k)


def _check(inp, B, H, W, T, nt, grid=None, dtype=F32, kernel=(3, 3), **kw):
    """The default run (helper asserted selected, nt quad-owning threads) against the run under
    NLSPN_RES_HELPER=0 (asserted not selected) and the step launches, all five outputs."""
    with _env(NLSPN_RES_GRID=grid, NLSPN_RESIDENT="1", NLSPN_RES_HELPER=None):
        assert _block(B, H, W, dtype, T=T, kernel=kernel) == nt
        assert _helper(B, H, W, dtype, T=T, kernel=kernel) == (True, nt + 64)
        a = propagate(*inp, prop_time=T, kernel=kernel, **kw)
        with _env(NLSPN_RES_HELPER="0"):
            assert _helper(B, H, W, dtype, T=T, kernel=kernel) == (False, nt)
            h = propagate(*inp, prop_time=T, kernel=kernel, **kw)
        with _env(NLSPN_RESIDENT="0"):
            assert _helper(B, H, W, dtype, T=T, kernel=kernel) == (False, 0)
            s = propagate(*inp, prop_time=T, kernel=kernel, **kw)
    torch.cuda.synchronize()
    _lib.check_resident()  # no launch aborted
    assert a["offset"] is not None and a["offset"].shape[1] == 2 * (kernel[0] * kernel[1])
    _same(a, h, "helper wave vs the main waves' copy")
    _same(a, s, "helper wave vs the step launches")
    return a


_shared = {}


def _cached(B, H, W, sigma=2.0, dtype=F32, K=8):
    """inputs computed once per shape and shared (never written by a test)"""
    key = (B, H, W, sigma, dtype, K)
    if key not in _shared:
        _shared[key] = _inputs(B, H, W, sigma=sigma, dtype=dtype, K=K)
    return _shared[key]


@pytest.mark.parametrize("dtype", [F32, F16])
@pytest.mark.parametrize("T", [2, 3, 18, 20])
def test_c2_build_full_parts(dtype, T):
    """C2's build (576 threads, compile-time pitch, the prologue in the launch): 4 full parts of
    24 x 24 quads.  T below the 18 planes (the tail at t = T - 1), equal and above; fp16 has the
    LDS row rewrite after iteration 1, which the helper must stay out of."""
    _check(_cached(1, 48, 192, dtype=dtype), 1, 48, 192, T, 576, grid="2,2", dtype=dtype)


@pytest.mark.parametrize("dtype,T", [(F32, 18), (F16, 3)])
def test_c2_build_partial_parts(dtype, T):
    """Parts of 23 x 23 and 23 x 24 quads in the 576-thread build: the helper's quad loop ends
    at the part's own count."""
    _check(_cached(1, 46, 188, dtype=dtype), 1, 46, 188, T, 576, grid="2,2", dtype=dtype)


@pytest.mark.parametrize("dtype,T", [(F32, 2), (F32, 18), (F16, 18)])
def test_run_time_thread_count_build(dtype, T):
    """384 quad-owning threads: the build that reads its thread count at run time (the launch's
    block less the helper wave)."""
    _check(_cached(2, 64, 96, dtype=dtype), 2, 64, 96, T, 384, grid="2,2", dtype=dtype)


@pytest.mark.parametrize("dtype", [F32, F16])
@pytest.mark.parametrize("T", [5, 36])
def test_wide_build_two_threads_per_quad(dtype, T):
    """1x17 (34 planes, two threads per quad, behind a step-1 launch): with the tail and without."""
    _check(_cached(1, 28, 160, dtype=dtype, K=16), 1, 28, 160, T, 576, grid="2,2", dtype=dtype, kernel=(1, 17))


def test_5x5_build():
    _check(_cached(1, 24, 64, K=24), 1, 24, 64, 4, _block_of(1, 24, 64, (5, 5)), dtype=F32, kernel=(5, 5))


def _block_of(B, H, W, kernel):
    with _env(NLSPN_RES_GRID=None, NLSPN_RESIDENT="1"):
        return _block(B, H, W, kernel=kernel)


@pytest.mark.parametrize("B,H,W,dtype,kernel", [(4, 240, 1216, F32, (3, 3)), (16, 228, 304, F16, (1, 17))])
def test_group_loop_builds(B, H, W, dtype, kernel):
    """The GROUPS builds (C3: two image groups, C5: four, in one launch): every group's offsets
    are copied."""
    K = kernel[0] * kernel[1] - 1
    _check(_inputs(B, H, W, dtype=dtype, K=K), B, H, W, 3, 576, dtype=dtype, kernel=kernel)


@pytest.mark.parametrize("kw,sigma", [({"always_clip": True}, 2.0), ({}, 12.0), ({"preserve_input": False}, 2.0)])
def test_flags_and_general_path_beside_helper(kw, sigma):
    """always_clip, and sigma 12 offsets (the fixed halo: far taps take the general path)."""
    _check(_cached(1, 48, 192, sigma=sigma), 1, 48, 192, 6, 576, grid="2,2", **kw)


def test_no_offset_output_no_helper():
    """return_offset=False and fixed-geometry calls: no helper wave, the plain block."""
    inp = _cached(1, 48, 192)
    with _env(NLSPN_RES_GRID="2,2", NLSPN_RESIDENT="1", NLSPN_RES_HELPER=None):
        assert _helper(1, 48, 192, off_out=False) == (False, 576)
        a = propagate(*inp, prop_time=6, return_offset=False)
        with _env(NLSPN_RESIDENT="0"):
            s = propagate(*inp, prop_time=6, return_offset=False)
            f = propagate(inp[0], inp[1], inp[2], inp[3], None, inp[5], prop_time=6)
        g = propagate(inp[0], inp[1], inp[2], inp[3], None, inp[5], prop_time=6)
    torch.cuda.synchronize()
    assert a["offset"] is None and g["offset"] is None
    _same(a, s, "return_offset=False")
    _same(g, f, "no offsets")


def test_small_part_builds_keep_their_setup_copy():
    """The 128-thread and split-quad builds copy in their setup: no helper."""
    with _env(NLSPN_RES_GRID=None, NLSPN_RESIDENT="1", NLSPN_RES_HELPER=None):
        assert _helper(1, 228, 304) == (False, 320)
        with _env(NLSPN_RES_SPLIT="2"):
            assert _helper(1, 228, 304) == (False, 192)
        with _env(NLSPN_RES_SPLIT="0"):
            assert _helper(1, 228, 304) == (False, 128)
        assert _helper(8, 228, 304) == (True, 640) and _helper(4, 240, 1216) == (True, 640)


def test_plan_replays_follow_alternating_offsets():
    """A plan replayed over inputs refilled in place from two data sets in turn: every output,
    `offset` included, is that replay's (the helper's copy belongs to its launch)."""
    T = 18
    ia, ib = _cached(1, 48, 192), _inputs(1, 48, 192, seed=32)
    with _env(NLSPN_RES_GRID="2,2", NLSPN_RES_HELPER=None):
        with _env(NLSPN_RESIDENT="0"):
            ra = {k: v.clone() for k, v in propagate(*ia, prop_time=T).items() if k in OUTS}
            rb = {k: v.clone() for k, v in propagate(*ib, prop_time=T).items() if k in OUTS}
        buf = [x.clone() for x in ia]
        oa = torch.empty(1, 24, 48, 192, device=DEV)  # the head tensor: aff and offset are its slices
        buf[3], buf[4] = oa[:, 16:], oa[:, :16]
        with _env(NLSPN_RESIDENT="1"):
            assert _helper(1, 48, 192) == (True, 640)
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
