"""GPU: every element of the generic DCN backward (seam 2) against the float64 oracle.

The six geometries of tests/test_gpu_dcn.py in float32, with offsets on the 1/64 grid and the
tap classes of tests/_bwd_cases.py (integer coordinates, -1, H-1, H, the partial-corner bands,
far outside).  For all five gradients and every element

    |got_e - g64_e| <= c * X_e        and        X_e == 0  =>  got_e == 0 exactly

with X the oracle's magnitude pass (oracle.mdcn_backward_bound) and c = min(4 * DCN_R32,
(n + 2) 2^-24), n the longest sum of that gradient (_bwd_cases.dcn_ceiling);
tests/test_oracle_backward.py holds DCN_R32, the float32 oracle's own worst ratio, under it.

Measured worst |got - g64| / X on an MI355X (recorded as bwd_elem/dcn<i>/<tensor>):

    case                            input             offset               mask             weight               bias
    dcn0                 1.9e-07 (0.32 c)   2.0e-07 (0.26 c)   1.7e-07 (0.25 c)   1.3e-08 (0.07 c)   1.0e-08 (0.15 c)
    dcn1                 1.6e-07 (0.24 c)   1.9e-07 (0.24 c)   1.7e-07 (0.24 c)   2.3e-08 (0.07 c)   3.9e-09 (0.09 c)
    dcn2                 1.3e-07 (0.24 c)   2.0e-07 (0.24 c)   1.6e-07 (0.24 c)   2.9e-08 (0.07 c)   5.2e-09 (0.06 c)
    dcn3                 1.4e-07 (0.27 c)   1.7e-07 (0.25 c)   1.5e-07 (0.24 c)   1.6e-08 (0.09 c)   4.0e-09 (0.04 c)
    dcn4                 1.3e-07 (0.18 c)   2.3e-07 (0.30 c)   1.9e-07 (0.27 c)   1.1e-08 (0.03 c)   1.9e-09 (0.08 c)
    dcn5                 2.7e-07 (0.27 c)   2.3e-07 (0.25 c)   1.5e-07 (0.25 c)   2.0e-08 (0.04 c)   6.0e-09 (0.03 c)
"""
import numpy as np
import pytest
import torch

import _bwd_cases as bc
from nlspn_eccv20_amd import dcn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("i", range(6))
def test_dcn_backward_per_element(oracle, record_metric, i):
    case = bc.dcn_cases()[i]
    C, Cout, group, dg, kh, kw, stride, pad, dil = case
    inp, wt, bias, off, mask, go = bc.dcn_inputs(100 + i, *case)
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    x = [cu(a).requires_grad_(True) for a in (inp, off, mask, wt, bias)]
    out = dcn.ModulatedDeformConvFunction.apply(x[0], x[1], x[2], x[3], x[4], stride, pad, dil, group, dg, 64)
    out.backward(cu(go))
    torch.cuda.synchronize()
    g64, X = oracle.mdcn_backward_bound(*(a.astype(np.float64) for a in (inp, wt, off, mask, go)), stride, pad, dil,
                                        group, dg)
    got = dict(zip(("input", "offset", "mask", "weight", "bias"), (t.grad.cpu().numpy() for t in x)))
    failures = []
    for t, want, bound in zip(bc.DCN_TENSORS, g64, X):
        cbar = min(4.0 * bc.DCN_R32[i][t], bc.dcn_ceiling(case, t))
        r, zeros_ok, k = bc.ratio(got[t], want, bound)
        record_metric(f"bwd_elem/dcn{i}/{t}", r)
        print(f"bwd_elem dcn{i} {t}: worst err/X = {r:.3e}, bar c = {cbar:.3e}, ratio/c = {r / cbar:.2f}")
        if not zeros_ok:
            failures.append(f"{t}: an element whose bound is 0 is not exactly 0")
        if not r <= cbar:
            failures.append(f"{t}: worst err/X {r:.3e} > c {cbar:.3e} at {np.unravel_index(k, bound.shape)}")
    assert not failures, "\n".join(failures)
