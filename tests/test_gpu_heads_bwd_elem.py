"""GPU: every element of every output of the head epilogue's backward through the C ABI against
float64 (cases, references and bars: tests/_heads_bwd_cases.py; no bar comes from the kernels
under test, no element is excluded).

Each launch is pinned on its own operands: nlspn_head_backward_pre on the seeded gradients and
saved outputs; the wide data gradients (nlspn_gconv_dgrad, preset NLSPN_GC_DG_S1 at cg = nout + 2
-> 2 C, never run at these shapes before), nlspn_head_dgrad_single and nlspn_head_wgrad on the
DEVICE's gpre, from which their float64 references are computed.  Operands are views into NaN
buffers, outputs and the workspace lie between sentinels.  Also: two calls give the same bits,
a NULL head's outputs are not touched and do not change the other head's bits, and a NaN in
g_off_aff row 0 reaches exactly its 3 x 3 neighbourhood in d_fe1 / d_fd_oa and nothing in
d_fd_id / d_fd_cf.

The 64-bit per-image bases are held by review: no case here (and no row of
tests/test_gpu_big_offsets.py) lies past 2^31 bytes.

Worst measured error / X per kind over the ten cases (MI355X), against the bars c:
    gpre sigmoid row  1.4e-7 of |ref|          (c = 4.8e-7)
    d_fe1, d_fd_oa    2.9e-7, 3.7e-7           (c = 2e-6)
    d_fd_id, d_fd_cf  1.9e-7, 2.5e-7           (c = 7.7e-7)
    dW                1.1e-7 (oa), 8.8e-8 (id), 7.7e-8 (cf)   (c = 2e-6; 3.6e-7 in the one-row case)
    db                5.9e-8                   (c = 2e-6)
"""
import pytest
import torch

import _heads_bwd_cases as hc
from nlspn_eccv20_amd import _lib
from nlspn_eccv20_amd.gru import GC_DG_S1, pack_adjoint_s1

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _pre(c, o, dev_o):
    """The pre launch on a case's operands: (buffer, gpre view)."""
    B, H, W, nout = c["B"], c["H"], c["W"], c["nout"]
    buf, gpre = hc.guarded_out((B, nout + 2, H, W), DEV)
    _lib.call("nlspn_head_backward_pre", gpre.device, dev_o["g_oa"], dev_o["g_pi"], dev_o["g_cf"],
              dev_o["pred_init"] if o["g_pi"] is not None else None, dev_o["conf"] if o["g_cf"] is not None else None, gpre,
              B, H, W, nout, _lib.STREAM)
    torch.cuda.synchronize()
    return buf, gpre


def _stacked(o, C, nout):
    """Wst (R, 2C, 3, 3): the stacked weight with the decoder halves of the id / cf rows zeroed."""
    wst = torch.zeros((nout + 2, 2 * C, 3, 3))
    wst[:nout] = o["w_oa"]
    for k, w in enumerate((o["w_id"], o["w_cf"])):
        if w is not None:
            wst[nout + k, C:] = w[0, C:]
    return wst


def _dgrads(c, o, dev_o, gpre, heads=(True, True)):
    """The wide launch and the one-row launch on gpre: buffers and views by name."""
    B, C, H, W, nout = c["B"], c["C"], c["H"], c["W"], c["nout"]
    out = {k: hc.guarded_out((B, C, H, W), DEV) for k in ("d_fe1", "d_fd_oa")}
    wadj = hc.guarded(pack_adjoint_s1(_stacked(o, C, nout).to(DEV)).cpu(), DEV)
    _lib.call("nlspn_gconv_dgrad", gpre.device, GC_DG_S1, gpre, nout + 2, wadj, None, None, None, out["d_fd_oa"][1],
              out["d_fe1"][1], C, B, H, W, 2 * C, H, W, 0, 1.0, _lib.STREAM)
    for k, w, on in (("d_fd_id", "w_id", heads[0]), ("d_fd_cf", "w_cf", heads[1])):
        if o[w] is not None and on:
            out[k] = hc.guarded_out((B, C, H, W), DEV)
    v = lambda k: out[k][1] if k in out else None  # noqa: E731
    _lib.call("nlspn_head_dgrad_single", gpre.device, gpre, dev_o["w_id"] if v("d_fd_id") is not None else None,
              dev_o["w_cf"] if v("d_fd_cf") is not None else None, v("d_fd_id"), v("d_fd_cf"), B, C, H, W, nout, _lib.STREAM)
    torch.cuda.synchronize()
    return out


def _wgrad(c, o, dev_o, gpre, heads=(True, True)):
    B, C, H, W, nout = c["B"], c["C"], c["H"], c["W"], c["nout"]
    need = _lib.get().nlspn_head_wgrad_workspace_bytes(B, C, H, W, nout)
    assert need == 4 * hc.plan_of(c)["floats"]
    out = {"dw_oa": hc.guarded_out((nout, 2 * C, 3, 3), DEV), "db_oa": hc.guarded_out((nout,), DEV)}
    for name, src, on in (("id", "fd_id", heads[0]), ("cf", "fd_cf", heads[1])):
        if o[src] is not None and on:
            out["dw_" + name] = hc.guarded_out((1, 2 * C, 3, 3), DEV)
            out["db_" + name] = hc.guarded_out((1,), DEV)
    out["ws"] = hc.guarded_out((need // 4,), DEV)  # exactly the queried bytes
    v = lambda k: out[k][1] if k in out else None  # noqa: E731
    _lib.call("nlspn_head_wgrad", gpre.device, gpre, dev_o["fe1"], dev_o["fd_oa"], dev_o["fd_id"] if v("dw_id") is not None else None,
              dev_o["fd_cf"] if v("dw_cf") is not None else None, v("dw_oa"), v("db_oa"), v("dw_id"), v("db_id"), v("dw_cf"),
              v("db_cf"), out["ws"][1], need, B, C, H, W, nout, _lib.STREAM)
    torch.cuda.synchronize()
    return out


def _device_operands(c, o):
    shift = 1 if c.get("unaligned") else 0
    return {k: hc.guarded(v, DEV, shift=shift if k in ("fe1", "fd_oa", "fd_id", "fd_cf") else 0) for k, v in o.items()}


def _intact(out, what):
    for k, (buf, _) in out.items():
        assert hc.guards_intact(buf), f"a store outside {k} ({what})"


@pytest.mark.parametrize("cid", hc.IDS)
def test_every_element_of_every_output(cid, record_metric):
    c, o = hc.BY_ID[cid], hc.operands(cid)
    B, C, H, W, nout = c["B"], c["C"], c["H"], c["W"], c["nout"]
    dev_o = _device_operands(c, o)
    if c.get("unaligned"):
        assert all(dev_o[k].data_ptr() % 16 == 4 for k in ("fe1", "fd_oa", "fd_id", "fd_cf"))
    # ---- gpre
    buf, gpre = _pre(c, o, dev_o)
    assert hc.guards_intact(buf), "a store outside gpre"
    ref = hc.gpre_reference(o["g_oa"], o["g_pi"], o["g_cf"], o["pred_init"], o["conf"], B, H, W, nout)
    got = gpre.cpu().double()
    assert torch.equal(got[:, :nout + 1], ref[:, :nout + 1]), "rows < nout and the ReLU row are bit-equal"
    assert not bool(torch.signbit(gpre[:, nout].cpu()[o["pred_init"][:, 0] <= 0]).any()) if o["g_pi"] is not None else True
    hc.check(f"gpre_sigmoid/{cid}", got[:, nout + 1], ref[:, nout + 1], ref[:, nout + 1].abs(), hc.C_GATES, record=record_metric)
    if o["g_cf"] is None:
        assert not bool(got[:, nout + 1].any())  # zero rows, always R rows
    # ---- the data gradients, from the device's own gpre
    dg = _dgrads(c, o, dev_o, gpre)
    _intact(dg, "data gradients")
    R = hc.dgrad_reference(got, o["w_oa"], o["w_id"], o["w_cf"], C)
    assert set(R) == set(dg)
    for k, (r, X, cc) in R.items():
        hc.check(f"{k}/{cid}", dg[k][1].cpu(), r, X, cc, record=record_metric)
    # ---- the weight and bias gradients
    wg = _wgrad(c, o, dev_o, gpre)
    _intact(wg, "weight gradients / workspace")
    Rw = hc.wgrad_reference(got, o["fe1"], o["fd_oa"], o["fd_id"], o["fd_cf"], hc.plan_of(c))
    assert set(Rw) == set(wg) - {"ws"}
    for k, (r, X, cc) in Rw.items():
        hc.check(f"{k}/{cid}", wg[k][1].cpu(), r, X, cc, record=record_metric)
    # ---- the same bits again
    dg2, wg2 = _dgrads(c, o, dev_o, gpre), _wgrad(c, o, dev_o, gpre)
    assert torch.equal(_pre(c, o, dev_o)[1], gpre)
    for a, b in ((dg, dg2), (wg, wg2)):
        for k in a:
            if k != "ws":
                assert torch.equal(a[k][1], b[k][1]), k


def test_a_null_head_is_skipped_and_changes_no_other_bits():
    """Base case: with the cf pair NULL (then the id pair) the other head's outputs and the
    off_aff rows keep their bits, and nothing is written for the NULL head."""
    c, o = hc.BY_ID[hc.IDS[0]], hc.operands(hc.IDS[0])
    dev_o = _device_operands(c, o)
    _, gpre = _pre(c, o, dev_o)
    dg, wg = _dgrads(c, o, dev_o, gpre), _wgrad(c, o, dev_o, gpre)
    for heads, kept, gone in (((True, False), "id", "cf"), ((False, True), "cf", "id")):
        dg1, wg1 = _dgrads(c, o, dev_o, gpre, heads), _wgrad(c, o, dev_o, gpre, heads)
        _intact(dg1, "data gradients")
        _intact(wg1, "weight gradients / workspace")
        assert f"d_fd_{gone}" not in dg1 and f"dw_{gone}" not in wg1
        for k in (f"d_fd_{kept}",):
            assert torch.equal(dg1[k][1], dg[k][1]), k
        for k in ("dw_oa", "db_oa", f"dw_{kept}", f"db_{kept}"):
            assert torch.equal(wg1[k][1], wg[k][1]), k


def test_a_nan_reaches_exactly_its_neighbourhood():
    """A NaN at one pixel of g_off_aff row 0: in d_fe1 and d_fd_oa exactly the 3 x 3 neighbourhood
    of that pixel in that image (every channel), no element of d_fd_id / d_fd_cf."""
    c = hc.BY_ID[hc.IDS[1]]  # 2 x 64 x 37 x 50
    o = dict(hc.operands(c["id"]))
    b, y, x = 1, 17, 31
    o["g_oa"] = o["g_oa"].clone()
    o["g_oa"][b, 0, y, x] = float("nan")
    dev_o = _device_operands(c, o)
    _, gpre = _pre(c, o, dev_o)
    dg = _dgrads(c, o, dev_o, gpre)
    want = torch.zeros((c["B"], c["C"], c["H"], c["W"]), dtype=torch.bool)
    want[b, :, y - 1:y + 2, x - 1:x + 2] = True
    for k in ("d_fe1", "d_fd_oa"):
        assert torch.equal(torch.isnan(dg[k][1].cpu()), want), k
    for k in ("d_fd_id", "d_fd_cf"):
        assert bool(torch.isfinite(dg[k][1]).all()), k
