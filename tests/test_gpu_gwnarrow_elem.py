"""GPU: the streaming weight gradient of the narrow layers (nlspn_gconv_wgrad_narrow,
csrc/nlspn_gwnarrow.h) per element against float64, through the C ABI.  Cases, operands,
references and bars: tests/_gwnarrow_cases.py (its docstring states the bar; it is the project's
weight-gradient bar with the new plan's count of partial sums, and none of it comes from this
kernel).

Every case asserts, for every element of dW and db,
    finite  and  |got - ref64| <= c * X
on operands that are views into NaN buffers (a read outside an operand poisons an output; one case
starts its views one float past a 16-byte boundary), with outputs and the workspace (exactly the
queried bytes) between sentinel guards.  Two runs of a case give the same bits; a shape the entry
declines gives nlspn_gconv_wgrad's bits; the reference without the last slice's units violates the
bar (the check can fail).

Measured on an MI355X (gwnarrow_elem/<case id> for dW, .../db for db: the worst |got - ref| / X;
informational, the bars do not depend on them), all cases passing on the first run:
    dW  6.8e-8  n3-5-3x7-crop0x7 (6.7e-8 n16-8-1x37-crop1x0-bias-large; 5.1e-9 .. 4.3e-8 elsewhere)
    db  1.8e-8  n3-5-3x7-crop0x7 (0 at 1x1; 2.1e-9 .. 1.7e-8 elsewhere)
against c = 2e-6 (4.2e-7 .. 1.4e-6 where n + P + 2 is small).
"""
import pytest
import torch

import _gconv_bwd_cases as bc
import _gwnarrow_cases as nc
from nlspn_eccv20_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _guarded(t, mis):
    """bc.guarded, the view starting `mis` floats past the buffer's 16-byte aligned GUARD."""
    if not mis:
        return bc.guarded(t, DEV)
    n = t.numel()
    buf = torch.full((n + 2 * bc.GUARD + mis,), float("nan"), device=DEV, dtype=torch.float32)
    v = buf[bc.GUARD + mis:bc.GUARD + mis + n].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 * mis
    return v


def _call(name, c, sd, ld, need):
    Cs, c0 = c["Cs"], c["c0"]
    bw_, dw = bc.guarded_out((Cs, c0, 3, 3), DEV)
    bb, db = bc.guarded_out((c0 if c["bfl"] else Cs,), DEV)
    bws, ws = bc.guarded_out((need // 4,), DEV)   # exactly the queried bytes
    _lib.call(name, sd.device, c["stride"], sd, Cs, ld, c0, None, 0, dw, db, int(c["bfl"]), c["scale"], ws, need,
              c["B"], c["Hs"], c["Ws"], c["Hl"], c["Wl"], _lib.STREAM)
    torch.cuda.synchronize()
    assert bc.guards_intact(bw_) and bc.guards_intact(bb), "a store outside dW / db"
    assert bc.guards_intact(bws), "a store outside the queried workspace"
    return dw.cpu(), db.cpu()


def _run(cid, record=None, perturb=None):
    c = nc.BY_ID[cid]
    s, l = nc.operands(cid)
    Rf = nc.reference(cid, perturb)
    lib = _lib.get()
    assert lib.nlspn_gconv_wgrad_narrow_covers(2, c["Cs"], c["c0"], 0) == 1
    need = lib.nlspn_gconv_wgrad_narrow_workspace_bytes(*nc.shape_of(c))
    assert need == 4 * nc.plan_of(c)["floats"]
    sd, ld = _guarded(s, c["mis"]), _guarded(l, c["mis"])
    dw, db = _call("nlspn_gconv_wgrad_narrow", c, sd, ld, need)
    ww = bc.check(f"wgrad_narrow/{cid}", dw, Rf["dw"], Rf["Xw"], Rf["cw"])
    wb = bc.check(f"dbias_narrow/{cid}", db, Rf["db"], Rf["Xb"], Rf["cb"])
    print(f"gwnarrow_elem/{cid}: dW {ww:.3g}  db {wb:.3g}")
    if record:
        record(f"gwnarrow_elem/{cid}", ww)
        record(f"gwnarrow_elem/{cid}/db", wb)
    return c, sd, ld, need, dw, db


@pytest.mark.parametrize("cid", [c["id"] for c in nc.CASES])
def test_every_element_of_dw_and_db(cid, record_metric):
    c, sd, ld, need, dw, db = _run(cid, record_metric)
    dw2, db2 = _call("nlspn_gconv_wgrad_narrow", c, sd, ld, need)   # a second run: the same bits
    assert torch.equal(dw, dw2) and torch.equal(db, db2)


@pytest.mark.parametrize("shape", [(2, 40, 16, 2, 13, 18, 26, 36), (1, 16, 16, 2, 7, 9, 7, 9), (2, 16, 17, 1, 5, 6, 9, 11)])
def test_a_declined_shape_gives_the_f32_entrys_bits(shape):
    stride, Cs, Cl, B, Hs, Ws, Hl, Wl = shape
    lib = _lib.get()
    assert lib.nlspn_gconv_wgrad_narrow_covers(stride, Cs, Cl, 0) == 0
    need = lib.nlspn_gconv_wgrad_narrow_workspace_bytes(*shape)
    assert need == lib.nlspn_gconv_wgrad_workspace_bytes(*shape) > 0
    gen = torch.Generator().manual_seed(11)
    c = dict(stride=stride, Cs=Cs, c0=Cl, B=B, Hs=Hs, Ws=Ws, Hl=Hl, Wl=Wl, bfl=False, scale=0.5)
    sd = bc.guarded(torch.randn((B, Cs, Hs, Ws), generator=gen), DEV)
    ld = bc.guarded(torch.randn((B, Cl, Hl, Wl), generator=gen), DEV)
    a, b = _call("nlspn_gconv_wgrad_narrow", c, sd, ld, need), _call("nlspn_gconv_wgrad", c, sd, ld, need)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and bool(torch.isfinite(a[0]).all())


def test_the_check_can_fail():
    """The reference with the last slice's units zeroed violates the bar."""
    with pytest.raises(AssertionError, match="elements outside"):
        _run("n16-9-5x65-band-plus-one-crop1", perturb="skip_last_slice")
