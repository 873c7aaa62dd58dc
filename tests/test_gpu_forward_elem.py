"""GPU: every element of every iterate of the propagation forward, bit for bit, in every form.

tests/test_gpu_parity.py holds one step bit-exact against the oracle and the section by an RMSE;
the resident tests hold the forms bit-exact against each other.  All of them draw Gaussian
offsets: no tap on an integer coordinate, on -1, H - 1 or H, in the (-1, 0) and (H - 1, H) rims,
or exactly on the first or last row or column of a tile's LDS window - where the branches of the
five bilinear samplers are (the step kernel's pass A and pass B, the resident kernel's fast path,
fallback and wide-geometry copy, and the window-range test that picks one).  Here the inputs of
tests/_fwd_cases.py put taps there: the tap classes of tests/_bwd_cases.py in every drawn image,
and a ramp image whose taps land on integers and half-integers at every distance up to 30 cells
from their base cell (on, half a cell inside and a cell beyond every window edge of every build).

Bar, float32.  Given the device's own normalised affinities the kernels issue the oracle's IEEE
sequence (-ffp-contract=off), so with _fwd_cases.reference (the float32 oracle's loop, composed;
tests/test_fwd_cases_cpu.py) fed the run's own `aff`, `offset` and `confidence` outputs:

  * every one of the T pred_inter planes and pred: BIT-EQUAL (compared as uint32);
  * offset and confidence: bit-equal to oracle.off_insert and the float32 confidence blend;
  * aff, per element against the float64 oracle.affinity_normalization of the same float32 planes:
    |got - a64| <= c X, X = |a_k| (1 + sum |a_k| for the reference tap), c = min(4 A32, ceiling)
    (_fwd_cases.aff_bar); AS and ASS have no transcendental and the kernels sum in the oracle's
    order (normalize_taps, nlspn_common.h), so they are bit-equal to the float32 oracle's;
  * the form that ran is asserted through nlspn_resident_config / nlspn_resident_helper (printed
    per case), and no resident launch aborted (_lib.check_resident).

A failure names the worst element: index, iteration, border distance, the classes (or ramp
distances) of the pixel's taps, whether it is a clamp-gated cell.

Measured on an MI355X: every run bit-equal; worst aff err / X over the K taps 3.1e-7 at K = 8
(bar 8.3e-7), 3.2e-7 at K = 16, 4.1e-7 at K = 24, 4.4e-7 at K = 48 (bar 2.2e-6), over the
reference tap 2.0e-7 (bars 2.3e-7 .. 8.4e-7); recorded per run as fwd_elem/<run>/aff.

What these (finite) inputs cannot see, by construction of the step kernel: its edge_fix arm for a
tap at exactly -1 acts only when an edge tile's window holds a non-finite f
(test_exact_minus_one_tap_ignores_nonfinite_edge_cells holds it); and a pass-A range test that
admitted a tap exactly on the window's last row would add the row past the window with weight 0.

fp16 storage: one resident case, bit-equal on all five outputs to the fp16 step launches on the
same inputs; no oracle claim for the fp16 loop (tests/test_gpu_step_fp16.py holds one fp16 step
against the oracle on these inputs).
"""
import contextlib
import ctypes
import os

import numpy as np
import pytest
import torch

import _fwd_cases as fc
from nlspn_eccv20_amd import PropagationPlan, _lib, prop_step, propagate
from nlspn_eccv20_amd.propagation import propagate_normalized

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SWITCHES = ("NLSPN_RESIDENT", "NLSPN_RES_FIRST", "NLSPN_RES_SPLIT", "NLSPN_RES_HELPER", "NLSPN_RES_GRID",
            "NLSPN_RES_MERGE", "NLSPN_RES_L2", "NLSPN_RES_OFFCOPY")


@contextlib.contextmanager
def _env(kv):
    """The forward's A/B switches: those in kv set, every other one unset."""
    old = {k: os.environ.get(k) for k in SWITCHES}
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def cu(x, dtype=torch.float32):
    """(a copy: the shared inputs are read-only arrays)"""
    return None if x is None else torch.from_numpy(np.array(x)).to(DEV, dtype)


def host(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _form(c, Bt, T, dtype=0):
    """(resident planned, quad-owning threads, helper selected, threads per workgroup) under the
    current switches, from nlspn_resident_config / nlspn_resident_helper."""
    nt, blk = ctypes.c_int(), ctypes.c_int()
    L = _lib.get()
    ok = L.nlspn_resident_config(dtype, Bt, c["H"], c["W"], c["kh"], c["kw"], T, int(c["conf"]), None, ctypes.byref(nt),
                                 None)
    helper = L.nlspn_resident_helper(dtype, Bt, c["H"], c["W"], c["kh"], c["kw"], T, int(c["conf"]), 1, ctypes.byref(blk))
    return bool(ok), nt.value, bool(helper), blk.value


def assert_form(run_id, c, Bt, T, expect, env, dtype=0):
    """expect: "steps" (no resident launch) or (quad-owning threads, helper wave by default)."""
    ok, nt, helper, blk = _form(c, Bt, T, dtype)
    print(f"fwd_elem {run_id}: {Bt}x{c['H']}x{c['W']} {c['kh']}x{c['kw']} T={T} env={env} -> "
          + (f"resident, {nt} quad-owning threads, helper wave {helper}, block {blk}" if ok else "step launches"))
    if expect == "steps":
        assert (helper, blk) == (False, 0), (run_id, ok, nt, helper, blk)
        assert env.get("NLSPN_RESIDENT") == "0" or not ok, run_id
        return
    want_nt, want_helper = expect
    want_helper = want_helper and env.get("NLSPN_RES_HELPER") != "0"
    assert ok and nt == want_nt, (run_id, ok, nt, want_nt)
    assert (helper, blk) == (want_helper, want_nt + (64 if want_helper else 0)), (run_id, helper, blk)


def describe(name, s, got, exp, t_of=None):
    """The worst element of `got` (..., Bt, 1, H, W) that differs from `exp`, and what it is."""
    c = fc.INPUTS[name]
    H, W = c["H"], c["W"]
    bad = bits(got) != bits(exp)
    with np.errstate(invalid="ignore", over="ignore"):
        err = np.where(bad, np.abs(got.astype(np.float64) - exp.astype(np.float64)), -1.0)
    err[np.isnan(err)] = np.inf
    idx = np.unravel_index(int(np.argmax(err)), err.shape)
    b, y, x = int(idx[-4]), int(idx[-2]), int(idx[-1])
    txt = [f"{int(bad.sum())} of {bad.size} elements differ", f"worst at index (b={b}, y={y}, x={x})"]
    if got.ndim == 5:
        txt.append(f"iteration {int(idx[0]) + 1}" + (f" of {t_of}" if t_of else ""))
        first = np.flatnonzero(bad.reshape(bad.shape[0], -1).any(1))
        txt.append(f"first differing iteration {int(first[0]) + 1}")
    txt.append(f"got {got[idx]!r} expected {exp[idx]!r}")
    txt.append(f"border distance {min(y, H - 1 - y, x, W - 1 - x)}")
    if s["off"] is not None:
        if b == c["B"]:
            txt.append("ramp image, tap distances " + str([float(v) for v in s["dist"][:, y, x]]))
        else:
            h, w = fc.tap_coords(name, s)
            m = fc.classify(h[b, :, y, x], w[b, :, y, x], H, W)
            txt.append("tap classes " + str([fc.class_names(v) or ["common"] for v in m]))
    v = float(s["pred_init"][b, 0, y, x])
    gated = v <= 0 or float(exp[idx]) == 0.0
    txt.append(f"pred_init {v!r}" + (" (clamp-gated cell)" if gated else ""))
    return "; ".join(txt)


_ref = {}


def expected(oracle, name, s, aff, off_ins, conf_b, T):
    """_fwd_cases.reference on the run's own prologue outputs: (iterates 1..T, pred).  Computed once
    per input set for its longest T and shared while the prologue outputs stay bit-equal."""
    c = fc.INPUTS[name]
    key = (bits(aff).tobytes(), None if conf_b is None else bits(conf_b).tobytes(),
           None if off_ins is None else bits(off_ins).tobytes())
    hit = _ref.get(name)
    if hit is None or hit[0] != key:
        oracle.set_threads(16)
        hit = (key, fc.reference(oracle, name, s, aff, off_ins, conf_b, T=c["T"])[0])
        _ref[name] = hit
    inter = hit[1][:T]
    p = inter[T - 1]
    return inter, (p if c["clip"] else np.where(p < 0, np.float32(0), p))


def check_prologue(oracle, record_metric, run_id, name, s, o):
    """offset, confidence and aff of an output dict `o` (host arrays)."""
    c = fc.INPUTS[name]
    fails = []
    if c["offset"]:
        if not np.array_equal(bits(o["offset"]), bits(oracle.off_insert(s["off"]))):
            fails.append("offset: not bit-equal to oracle.off_insert")
    else:
        assert o["offset"] is None
    if c["conf"]:
        if not np.array_equal(bits(o["confidence"]), bits(fc.prologue(name, s)[1])):
            fails.append("confidence: not bit-equal to the float32 blend")
    else:
        assert o["confidence"] is None
    a64 = fc.aff_float64(oracle, name, s)
    r, taps, ref = fc.aff_ratios(name, o["aff"], a64)
    ctap, cref = fc.aff_bar(name)
    record_metric(f"fwd_elem/{run_id}/aff", max(taps, ref))
    print(f"fwd_elem {run_id} aff: worst err/X taps {taps:.3e} (bar {ctap:.3e}), reference tap {ref:.3e} (bar {cref:.3e})")
    if not (taps <= ctap and ref <= cref):
        K = c["kh"] * c["kw"] - 1
        bar = np.full(r.shape[1], ctap)
        bar[K // 2] = cref
        i = np.unravel_index(int(np.argmax(r / bar[None, :, None, None])), r.shape)
        fails.append(f"aff: worst err/X {r[i]:.3e} over the bar at (b={i[0]}, plane={i[1]}, y={i[2]}, x={i[3]}), "
                     f"raw affinities {s['aff'][i[0], :, i[2], i[3]].tolist()}")
    if c["kind"] in ("AS", "ASS"):
        a32 = oracle.affinity_normalization(s["aff"], c["kind"], fc.gamma_of(name))
        if not np.array_equal(bits(o["aff"]), bits(a32)):
            fails.append(f"aff ({c['kind']}): not bit-equal to the float32 oracle's, {int((bits(o['aff']) != bits(a32)).sum())} "
                         "elements differ")
    return fails


def check_outputs(oracle, record_metric, run_id, name, s, o, T):
    """Every assertion on a float32 output dict `o` of the section for input set `name`."""
    c = fc.INPUTS[name]
    o = {k: (None if o[k] is None else host(o[k])) for k in ("pred", "pred_inter_tensor", "aff", "offset", "confidence")}
    assert o["pred_inter_tensor"].shape == (T,) + s["pred_init"].shape and o["pred"].dtype == np.float32
    fails = check_prologue(oracle, record_metric, run_id, name, s, o)
    inter, pred = expected(oracle, name, s, o["aff"], o["offset"], o["confidence"], T)
    if not np.array_equal(bits(o["pred_inter_tensor"]), bits(inter)):
        fails.append("pred_inter: " + describe(name, s, o["pred_inter_tensor"], inter, T))
    if not np.array_equal(bits(o["pred"]), bits(pred)):
        fails.append("pred: " + describe(name, s, o["pred"], pred))
    assert not fails, f"{run_id} ({c['B']}+{int(c['offset'])} images):\n" + "\n".join(fails)


def gpu_inputs(name, s, dtype=torch.float32):
    """The call's tensors: raw offsets and affinities as slices of the (Bt, 3K, H, W) head tensor."""
    c = fc.INPUTS[name]
    K = c["kh"] * c["kw"] - 1
    if c["offset"]:
        oa = cu(np.concatenate([s["off"], s["aff"]], 1), dtype)
        aff, off = oa[:, 2 * K:], oa[:, :2 * K]
    else:
        aff, off = cu(s["aff"], dtype), None
    return (cu(s["pred_init"], dtype), cu(s["dep"], dtype), cu(s["conf"], dtype) if c["conf"] else None, aff, off,
            torch.tensor([fc.gamma_of(name)], device=DEV))


def call_kw(name, T):
    c = fc.INPUTS[name]
    return dict(prop_time=T, affinity=c["kind"], kernel=(c["kh"], c["kw"]), preserve_input=c["preserve"],
                always_clip=c["clip"])


STEPS = {"NLSPN_RESIDENT": "0"}
GRID22 = {"NLSPN_RES_GRID": "2,2"}
# run id -> (input set, T, switches, expected form).  The resident builds' shapes and switches are those
# of tests/test_gpu_resident.py, test_gpu_resident_helper.py and test_gpu_resident_loopforms.py with the
# ramp image as one more batch item; their thread counts are the planner's at the MI355X's 256 CUs.
RUNS = {
    # per-iteration step launches
    "steps_vec_T1": ("g24x40", 1, STEPS, "steps"),
    "steps_vec_T2": ("g24x40", 2, STEPS, "steps"),
    "steps_vec_T6": ("g24x40", 6, STEPS, "steps"),
    "steps_scalar_T1": ("g19x45", 1, STEPS, "steps"),      # W % 4 != 0
    "steps_scalar_T2": ("g19x45", 2, STEPS, "steps"),
    "steps_scalar_T6": ("g19x45", 6, STEPS, "steps"),
    "scalar_default_T6": ("g19x45", 6, {}, "steps"),        # no resident form for W % 4 != 0
    "steps_k17": ("k17", 4, STEPS, "steps"),
    "steps_k5x5": ("k5x5", 4, STEPS, "steps"),
    "steps_k7x7": ("k7x7", 4, STEPS, "steps"),
    "k7x7_default": ("k7x7", 4, {}, "steps"),               # no resident 7x7 build
    "steps_noffset": ("noffset", 4, STEPS, "steps"),
    "steps_far": ("far40x64", 4, STEPS, "steps"),
    # kinds and flags, the default form (a split-quad resident build at this size)
    "AS": ("AS", 4, {}, (320, False)),
    "ASS": ("ASS", 4, {}, (320, False)),
    "TC": ("TC", 4, {}, (320, False)),
    "noconf": ("noconf", 4, {}, (320, False)),
    "nopreserve": ("nopreserve", 4, {}, (320, False)),
    "clip": ("clip", 4, {}, (320, False)),
    "steps_AS": ("AS", 4, STEPS, "steps"),
    "steps_ASS": ("ASS", 4, STEPS, "steps"),
    "steps_TC": ("TC", 4, STEPS, "steps"),
    "steps_noconf": ("noconf", 4, STEPS, "steps"),
    "steps_nopreserve": ("nopreserve", 4, STEPS, "steps"),
    "steps_clip": ("clip", 4, STEPS, "steps"),
    "T24": ("T24", 24, {}, (320, False)),
}
# the resident builds: each in both loop forms and behind a step-1 launch
BUILDS = {
    "default": ("g24x40", 6, {}, (320, False)),                                   # the planner's choice
    "default_T2": ("g24x40", 2, {}, (320, False)),
    "run_time_nt": ("rt32x128", 5, dict(GRID22, NLSPN_RES_SPLIT="0"), (256, True)),
    "nt576": ("c48x192", 5, GRID22, (576, True)),
    "split4": ("split100x120", 4, {}, (320, False)),                              # four threads per quad
    "split2": ("split100x120", 4, {"NLSPN_RES_SPLIT": "2"}, (192, False)),         # two threads per quad
    "nt128": ("split100x120", 4, {"NLSPN_RES_SPLIT": "0"}, (128, False)),          # the same parts, a thread per quad
    "wide_k17": ("wide28x160", 5, GRID22, (576, True)),                            # 1x17, two threads per quad
    "k5x5": ("r5x5_24x64", 4, {}, (256, True)),
    "groups": ("groups240x1216", 3, {}, (576, True)),                              # two image groups, one launch
    "far": ("far40x64", 4, {}, (320, False)),                                      # the general path
}
for _n, (_s, _T, _e, _x) in BUILDS.items():
    RUNS[_n] = (_s, _T, _e, _x)
    RUNS[_n + "-helper0"] = (_s, _T, dict(_e, NLSPN_RES_HELPER="0"), _x)
    RUNS[_n + "-first0"] = (_s, _T, dict(_e, NLSPN_RES_FIRST="0"), _x)


@pytest.mark.parametrize("run_id", list(RUNS))
def test_forward_per_element(oracle, record_metric, run_id):
    name, T, env, expect = RUNS[run_id]
    c = fc.INPUTS[name]
    s = fc.inputs(name)
    Bt = s["pred_init"].shape[0]
    inp = gpu_inputs(name, s)
    with _env(env):
        assert_form(run_id, c, Bt, T, expect, env)
        o = propagate(*inp, **call_kw(name, T))
        torch.cuda.synchronize()
    _lib.check_resident()  # no launch aborted
    check_outputs(oracle, record_metric, run_id, name, s, o, T)


def _oracle_prologue(oracle, name, s):
    """The float32 oracle's prologued planes: p0, blended confidence, normalised affinities,
    inserted offsets."""
    c = fc.INPUTS[name]
    p0, conf_b = fc.prologue(name, s)
    aff = oracle.affinity_normalization(s["aff"], c["kind"], fc.gamma_of(name))
    return p0, conf_b, aff, oracle.off_insert(s["off"])


@pytest.mark.parametrize("layout", ["raw", "inserted"])
def test_prop_step_alone(oracle, layout):
    """One prop_step on the oracle's prologued planes, both offset layouts: bit-equal to one
    iteration of the reference."""
    name = "g24x40"
    c = fc.INPUTS[name]
    s = fc.inputs(name)
    p0, conf_b, aff, off_ins = _oracle_prologue(oracle, name, s)
    inter, _ = fc.reference(oracle, name, s, aff, off_ins, conf_b, T=1)
    off = cu(s["off"]) if layout == "raw" else cu(off_ins)
    out = host(prop_step(cu(p0), cu(conf_b), cu(s["dep"]), cu(aff), off, kernel=(c["kh"], c["kw"]), offset_layout=layout))
    assert np.array_equal(bits(out), bits(inter[0])), describe(name, s, out, inter[0])


@pytest.mark.parametrize("env,expect", [({}, (320, False)), (STEPS, "steps")])
def test_propagate_normalized(oracle, env, expect):
    """propagate_normalized fed the float32 oracle's prologued planes: nothing is normalised on the
    device, so every output is bit-equal to oracle.propagate itself."""
    name, T = "g24x40", 6
    c = fc.INPUTS[name]
    s = fc.inputs(name)
    p0, conf_b, aff, off_ins = _oracle_prologue(oracle, name, s)
    e = fc.oracle_propagate(oracle, name, s, T=T)
    with _env(env):
        ok, nt, _, _ = _form(c, s["pred_init"].shape[0], T)
        print(f"fwd_elem normalized env={env}: resident {ok}, {nt} quad-owning threads")
        assert (not ok or env == STEPS) if expect == "steps" else (ok and nt == expect[0])
        o = propagate_normalized(cu(p0), cu(s["dep"]), cu(conf_b), cu(aff), cu(off_ins), prop_time=T,
                                 kernel=(c["kh"], c["kw"]), preserve_input=c["preserve"], always_clip=c["clip"])
        torch.cuda.synchronize()
    _lib.check_resident()
    got, pred = host(o["pred_inter_tensor"]), host(o["pred"])
    assert np.array_equal(bits(got), bits(e["pred_inter"])), describe(name, s, got, e["pred_inter"], T)
    assert np.array_equal(bits(pred), bits(e["pred"])), describe(name, s, pred, e["pred"])
    for t in range(T):
        assert o["pred_inter"][t].data_ptr() == o["pred_inter_tensor"][t].data_ptr()


def test_plan_replayed_over_refilled_inputs(oracle, record_metric):
    """One PropagationPlan replayed twice over inputs refilled in place, first with another input
    set's values: the second replay is the reference of what was filled in last."""
    name, other, T = "g24x40", "clip", 6
    c = fc.INPUTS[name]
    s, s2 = fc.inputs(name), fc.inputs(other)
    K = c["kh"] * c["kw"] - 1
    Bt = s["pred_init"].shape[0]
    oa = torch.empty((Bt, 3 * K, c["H"], c["W"]), device=DEV)
    buf = [torch.empty((Bt, 1, c["H"], c["W"]), device=DEV) for _ in range(3)] + [oa[:, 2 * K:], oa[:, :2 * K]]
    gamma = torch.tensor([fc.gamma_of(name)], device=DEV)
    with _env({}):
        assert_form("plan", c, Bt, T, (320, False), {})
        plan = PropagationPlan(*buf, gamma, **call_kw(name, T))
        for src in (s2, s):
            for d, k in zip(buf, ("pred_init", "dep", "conf", "aff", "off")):
                d.copy_(cu(src[k]))
            o = plan.replay()
            torch.cuda.synchronize()
        plan.check()
        check_outputs(oracle, record_metric, "plan", name, s, o, T)
        plan.close()


@pytest.mark.parametrize("T", [3, 5])
def test_fp16_resident_equals_fp16_steps(T):
    """fp16 storage in the 576-thread build: all five outputs bit-equal to the fp16 step launches
    on the same (grid-and-ramp, rounded to fp16) inputs."""
    name = "c48x192"
    c = fc.INPUTS[name]
    s = fc.inputs(name)
    inp = gpu_inputs(name, s, torch.float16)
    Bt = s["pred_init"].shape[0]
    with _env(GRID22):
        assert_form(f"fp16_T{T}", c, Bt, T, (576, True), GRID22, dtype=1)
        a = propagate(*inp, **call_kw(name, T))
    with _env(STEPS):
        assert_form(f"fp16_T{T}_steps", c, Bt, T, "steps", STEPS, dtype=1)
        b = propagate(*inp, **call_kw(name, T))
    torch.cuda.synchronize()
    _lib.check_resident()
    for k in ("pred", "pred_inter_tensor", "offset", "aff", "confidence"):
        assert a[k].dtype == torch.float16 and torch.equal(a[k].view(torch.int16), b[k].view(torch.int16)), k
