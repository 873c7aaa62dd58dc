"""Checks shared by tests/test_gpu_big_offsets.py and tests/test_gpu_unaligned_views.py: existing
per-element bars restated once, for gradients that are computed on other batches than the cases'."""
import numpy as np


def backward_failures(name, got, g64, X, info, note=None):
    """The per-element check of tests/test_gpu_backward_elem.py, unchanged, for gradients `got` of
    _bwd_cases case `name` against the float64 oracle (g64, X, info of _bwd_cases.oracle_bound):
    |got - g64| <= c X + Q with c = min(4 R32, ceiling), and X == 0 => got == 0.  Returns the list of
    failures (empty: pass); note(tensor, ratio, c) is called with every worst ratio."""
    import _bwd_cases as bc
    T = bc.case_of(name)["T"]
    Qb = 2.0 ** -50 * info["mass"].max(0) * T * max(1.0, info["amax"]) ** T
    failures = []
    for t in bc.tensors_of(name):
        cbar = min(4.0 * bc.R32[name][t], bc.ceiling(name, t))
        x = np.asarray(X[t], np.float64)
        Q = float(Qb.max()) if t == "gamma" else np.broadcast_to(Qb.reshape(-1, 1, 1, 1), x.shape).ravel()
        if t == "aff":
            Q = Q + bc.aff_slack(name, info)
        r, zeros_ok, i = bc.ratio(np.asarray(got[t]), g64[t], x, bc.checked_mask(name, t, np.asarray(got[t])), Q)
        if note is not None:
            note(t, r, cbar)
        if not zeros_ok:
            failures.append(f"{t}: an element whose bound is 0 is not exactly 0")
        if not r <= cbar:
            failures.append(f"{t}: worst (err - Q)/X {r:.3e} > c {cbar:.3e} at flat index {i}")
    return failures
