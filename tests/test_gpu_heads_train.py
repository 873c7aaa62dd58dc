"""GPU: training through the fused head epilogue (heads.head_epilogue(..., differentiable=True),
heads._HeadFn, NLSPNModel.native_head_train; csrc/nlspn_heads_bwd.h).

 1. Under gradients the differentiable call's outputs are bit-equal to the no_grad call, and all
    ten gradients (four sources, three weights, three biases) are within 1e-4 relative L2 (the
    project's gradient bar) of a float64 CPU autograd of the reference's op sequence in which
    the ReLU is a multiplication by the DEVICE's own pred_init > 0 mask (a rounding-level sign
    disagreement at the kink cannot enter; the pixels whose mask differs from the float64 sign
    are counted and recorded, nothing is excluded).
 2. Frozen parameters: no weight-gradient launch, .grad stays None; sources without grad: no
    data-gradient launch; a frozen id head alone.
 3. precision="bf16x3" with a gradient-requiring differentiable call raises; under no_grad it
    is today's call, bit for bit.  differentiable=False under gradients returns tensors
    without grad_fn.
 4. NLSPNModel (non-GRU and GRU mode) on a small input, forward + loss.backward() with
    native_head_train on and off: the two forwards' pred_init > 0 masks agree everywhere (a
    condition on the seeded input), then pred and every parameter gradient are within 1e-3
    relative L2 of each other (the bar of the section-level comparison of DESIGN 3.8.1: the
    module path does not reproduce itself bit for bit); train_stats proves which path ran, the
    module call counts with the switch off are today's, a replica keeps the modules.
 5. Two native runs give bit-equal gradients wherever the step is reproducible at all: all ten
    gradients of the autograd function on the same incoming gradients, and through the model's
    encoder, decoder and heads (NLSPNModel.heads) under fixed projections of the three outputs
    the six head-parameter gradients and the four gradients handed to the decoder.  A whole
    forward + loss.backward() is NOT bit-reproducible with the switch on or off: the propagation
    backward flushes dL/df with float atomics, so the gradients ENTERING the heads
    already differ between two identical runs.  Measured on MI355X (2 x 50 x 70, T = 3, both
    modes, cudnn.deterministic on): the three head outputs bit-equal, all three incoming
    gradients different, 113 (native) / 112 (modules) of 116 parameter gradients different
    non-GRU, 137 / 137 of 140 in GRU mode; without cudnn.deterministic even pred differs (MIOpen).
"""
import copy
import types

import pytest
import torch
import torch.nn as nn

from nlspn_eccv20_amd import heads
from nlspn_eccv20_amd.model import NLSPNModel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAR, BAR_MODEL = 1e-4, 1e-3
NAMES = ("fe1", "fd_oa", "fd_id", "fd_cf")


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def _setup(B, C, H, W, nout, hid=True, hcf=True, seed=3):
    g = torch.Generator().manual_seed(seed)
    src = {n: torch.randn((B, C, H, W), generator=g) for n in NAMES}
    if not hid:
        src["fd_id"] = None
    if not hcf:
        src["fd_cf"] = None
    torch.manual_seed(seed)
    convs = {"oa": nn.Conv2d(2 * C, nout, 3, 1, 1), "id": nn.Conv2d(2 * C, 1, 3, 1, 1) if hid else None,
             "cf": nn.Conv2d(2 * C, 1, 3, 1, 1) if hcf else None}
    ups = {"oa": torch.randn((B, nout, H, W), generator=g), "id": torch.randn((B, 1, H, W), generator=g),
           "cf": torch.randn((B, 1, H, W), generator=g)}
    return src, convs, ups


def _call(src, convs, differentiable=True, precision="fp32", weights=None):
    return heads.head_epilogue(src["fe1"], src["fd_oa"], convs["oa"], src["fd_id"], convs["id"], src["fd_cf"], convs["cf"],
                               weights=weights, precision=precision, differentiable=differentiable)


def _loss(outs, ups, dev):
    pred, off, conf = outs
    loss = (off * ups["oa"].to(off)).sum()
    if pred is not None:
        loss = loss + (pred * ups["id"].to(pred)).sum()
    if conf is not None:
        loss = loss + (conf * ups["cf"].to(conf)).sum()
    return loss


@pytest.mark.parametrize("shape", [(2, 64, 40, 64, 24, True, True), (1, 16, 13, 40, 48, False, True)])
def test_outputs_are_the_inference_bits_and_gradients_match_float64(shape, record_metric):
    B, C, H, W, nout, hid, hcf = shape
    src, convs, ups = _setup(*shape)
    dsrc = {n: None if t is None else t.to(DEV).requires_grad_(True) for n, t in src.items()}
    dconvs = {k: None if c is None else copy.deepcopy(c).to(DEV) for k, c in convs.items()}
    with torch.no_grad():
        want = _call(dsrc, dconvs)
    before = dict(heads.stats)
    heads.train_stats.update(dict.fromkeys(heads.train_stats, 0))
    outs = _call(dsrc, dconvs)
    assert heads.stats["fp32"] == before["fp32"] + 1 and heads.stats["bf16x3"] == before["bf16x3"]
    for a, b in zip(outs, want):
        assert (a is None and b is None) or (torch.equal(a, b) and a.grad_fn is not None)
    _loss(outs, ups, DEV).backward()
    assert heads.train_stats == {"pre": 1, "dgrad": 1, "dgrad_single": 1, "wgrad": 1}
    # float64 reference: the op sequence with the ReLU as the device's own mask
    rsrc = {n: None if t is None else t.double().requires_grad_(True) for n, t in src.items()}
    rconvs = {k: None if c is None else copy.deepcopy(c).double() for k, c in convs.items()}
    off = rconvs["oa"](torch.cat((rsrc["fd_oa"], rsrc["fe1"]), 1))
    pred = conf = None
    if hid:
        pre = rconvs["id"](torch.cat((rsrc["fd_id"], rsrc["fe1"]), 1))
        mask = (outs[0].detach() > 0).cpu()
        differ = int((mask != (pre.detach() > 0)).sum())
        record_metric(f"heads_train/mask_pixels_differing/{B}x{C}x{H}x{W}", differ)
        print("pixels whose device mask differs from the float64 sign:", differ, "of", mask.numel())
        pred = pre * mask.double()
    if hcf:
        conf = torch.sigmoid(rconvs["cf"](torch.cat((rsrc["fd_cf"], rsrc["fe1"]), 1)))
    _loss((pred, off, conf), {k: v.double() for k, v in ups.items()}, "cpu").backward()
    seen = 0
    for n in NAMES:
        if src[n] is not None:
            e = _rel(dsrc[n].grad, rsrc[n].grad)
            record_metric(f"heads_train/d_{n}/{B}x{C}x{H}x{W}", e)
            assert e <= BAR, (n, e)
            seen += 1
    for k in ("oa", "id", "cf"):
        if convs[k] is not None:
            for pn in ("weight", "bias"):
                e = _rel(getattr(dconvs[k], pn).grad, getattr(rconvs[k], pn).grad)
                record_metric(f"heads_train/d{pn}_{k}/{B}x{C}x{H}x{W}", e)
                assert e <= BAR, (k, pn, e)
                seen += 1
    assert seen == (10 if hid and hcf else 7)


def _fresh(requires=True, freeze=()):
    src, convs, ups = _setup(2, 16, 12, 20, 24)
    dsrc = {n: t.to(DEV).requires_grad_(requires) for n, t in src.items()}
    dconvs = {k: c.to(DEV) for k, c in convs.items()}
    for k in freeze:
        dconvs[k].requires_grad_(False)
    heads.train_stats.update(dict.fromkeys(heads.train_stats, 0))
    return dsrc, dconvs, ups


def test_frozen_parameters_launch_no_wgrad():
    dsrc, dconvs, ups = _fresh(freeze=("oa", "id", "cf"))
    _loss(_call(dsrc, dconvs), ups, DEV).backward()
    assert heads.train_stats == {"pre": 1, "dgrad": 1, "dgrad_single": 1, "wgrad": 0}
    assert all(p.grad is None for c in dconvs.values() for p in c.parameters())
    assert all(t.grad is not None for t in dsrc.values())


def test_sources_without_grad_launch_no_dgrad():
    dsrc, dconvs, ups = _fresh(requires=False)
    _loss(_call(dsrc, dconvs), ups, DEV).backward()
    assert heads.train_stats == {"pre": 1, "dgrad": 0, "dgrad_single": 0, "wgrad": 1}
    assert all(p.grad is not None for c in dconvs.values() for p in c.parameters())


def test_a_frozen_id_head_only():
    dsrc, dconvs, ups = _fresh(freeze=("id",))
    _loss(_call(dsrc, dconvs), ups, DEV).backward()
    assert heads.train_stats == {"pre": 1, "dgrad": 1, "dgrad_single": 1, "wgrad": 1}
    assert dconvs["id"].weight.grad is None and dconvs["id"].bias.grad is None
    full_src, full_convs, _ = _fresh()
    _loss(_call(full_src, full_convs), ups, DEV).backward()
    for k in ("oa", "cf"):  # the other heads' gradients keep their bits
        assert torch.equal(dconvs[k].weight.grad, full_convs[k].weight.grad) and torch.equal(dconvs[k].bias.grad, full_convs[k].bias.grad)
    assert all(torch.equal(dsrc[n].grad, full_src[n].grad) for n in NAMES)


def test_bf16x3_is_inference_only_and_the_default_records_nothing():
    dsrc, dconvs, ups = _fresh()
    with pytest.raises(RuntimeError, match="inference only"):
        _call(dsrc, dconvs, precision="bf16x3")
    with torch.no_grad():
        a, b = _call(dsrc, dconvs, precision="bf16x3"), _call(dsrc, dconvs, differentiable=False, precision="bf16x3")
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    outs = _call(dsrc, dconvs, differentiable=False)  # under gradients, on parameters that require grad: as today
    assert all(o.grad_fn is None and not o.requires_grad for o in outs)
    with torch.no_grad():
        assert all(torch.equal(x, y) for x, y in zip(outs, _call(dsrc, dconvs)))
    assert heads.train_stats == dict.fromkeys(heads.train_stats, 0)


# ------------------------------------------------------------------ the model
B, H, W, T = 2, 50, 70, 3


def _model(gru, seed=0):
    args = types.SimpleNamespace(prop_kernel=3, affinity="TGASS", affinity_gamma=0.5, prop_time=T,
                                 preserve_input=True, always_clip=False, conf_prop=True, offset=True,
                                 network="resnet34", from_scratch=True, zero_init_aff=False, use_GRU=gru,
                                 use_S2D=False, GRU_hidden_dim=128, GRU_input_dim=128, lr=1e-3, max_depth=10.0,
                                 patch_height=H, patch_width=W, model_name="NLSPN")
    torch.manual_seed(seed)
    return NLSPNModel(args).to(DEV).eval()


def _sample(seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    rgb = torch.randn((B, 3, H, W), device=DEV, generator=g)
    depth = torch.rand((B, 1, H, W), device=DEV, generator=g) * 10
    return {"rgb": rgb, "dep": depth * (torch.rand((B, 1, H, W), device=DEV, generator=g) < 0.05)}


def _step(m, sample, native, replica=False):
    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        return _step_det(m, sample, native, replica)
    finally:
        torch.backends.cudnn.deterministic = det


def _step_det(m, sample, native, replica):
    """(Under cudnn.deterministic: MIOpen's default choice makes even the encoder's FORWARD differ
    between two identical calls here, and a ReLU deep in the network that flips between the two
    runs compared would enter the comparison as the head's error.)"""
    m.native_head_train = native
    calls = {"id": 0, "oa": 0, "cf": 0}
    hooks = [mod.register_forward_hook(lambda *a, k=k: calls.__setitem__(k, calls[k] + 1))
             for k, mod in (("id", m.id_dec0), ("oa", m.off_aff_dec0), ("cf", m.cf_dec0))]
    heads.train_stats.update(dict.fromkeys(heads.train_stats, 0))
    m.zero_grad(set_to_none=True)
    if replica:
        m._is_replica = True
    pred_init = m.heads(sample)[0].detach()
    heads.train_stats.update(dict.fromkeys(heads.train_stats, 0))
    for k in calls:
        calls[k] = 0
    out = m(sample)
    g = torch.Generator(device=DEV).manual_seed(21)
    (out["pred"] * torch.randn(out["pred"].shape, device=DEV, generator=g)).sum().backward()
    for h in hooks:
        h.remove()
    if replica:
        del m._is_replica
    grads = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
    return dict(pred=out["pred"].detach().clone(), mask=pred_init > 0, grads=grads, stats=dict(heads.train_stats), calls=calls)


@pytest.mark.parametrize("gru", [False, True])
def test_model_trains_through_the_native_heads(gru, record_metric):
    m, sample = _model(gru), _sample(4)
    assert m.native_head_train is False
    with pytest.raises(ValueError):
        m.native_head_train = 1
    on, off, off2 = _step(m, sample, True), _step(m, sample, False), _step(m, sample, False)
    floor = max(_rel(off2["grads"][n], g) for n, g in off["grads"].items())
    record_metric(f"heads_train/model/{'gru' if gru else 'plain'}/modules_vs_modules_worst_rel_l2", floor)
    print("the module path against itself, worst parameter-gradient rel L2:", floor)
    assert torch.equal(on["mask"], off["mask"]), "the seeded input puts a pre-activation at the kink: name another seed"
    assert on["stats"] == {"pre": 1, "dgrad": 1, "dgrad_single": 1, "wgrad": 1} and on["calls"] == {"id": 0, "oa": 0, "cf": 0}
    assert off["stats"] == dict.fromkeys(heads.train_stats, 0) and off["calls"] == {"id": 1, "oa": 1, "cf": 1}
    e = _rel(on["pred"], off["pred"])
    assert e <= BAR_MODEL, e
    assert set(on["grads"]) == set(off["grads"]) and any(n.startswith("id_dec0") for n in on["grads"])
    worst = 0.0
    for n, g in off["grads"].items():
        e = _rel(on["grads"][n], g)
        worst = max(worst, e)
        assert e <= BAR_MODEL, (n, e)
    record_metric(f"heads_train/model/{'gru' if gru else 'plain'}/worst_rel_l2", worst)
    print("model", "gru" if gru else "plain", "worst parameter-gradient rel L2 native vs modules:", worst)
    rep = _step(m, sample, True, replica=True)  # a DataParallel replica keeps the modules
    assert rep["stats"] == dict.fromkeys(heads.train_stats, 0) and rep["calls"] == {"id": 1, "oa": 1, "cf": 1}


def test_two_native_runs_of_the_function_give_the_same_bits():
    runs = []
    for _ in range(2):
        dsrc, dconvs, ups = _fresh()
        _loss(_call(dsrc, dconvs), ups, DEV).backward()
        runs.append([t.grad for t in dsrc.values()] + [p.grad for c in dconvs.values() for p in c.parameters()])
    assert len(runs[0]) == 10 and all(torch.equal(a, b) for a, b in zip(*runs))


def _heads_step(m, sample):
    """Encoder, decoder and heads under fixed projections of the three outputs (no propagation,
    whose backward is not reproducible: module docstring): the head-parameter gradients and the
    gradients handed to the decoder."""
    cap = []
    dec = type(m)._decoder

    def capture(sample):
        outs = dec(m, sample)
        for t in outs:
            t.retain_grad()
        cap.append(outs)
        return outs
    m._decoder = capture
    try:
        m.zero_grad(set_to_none=True)
        outs = m.heads(sample)
    finally:
        del m._decoder
    g = torch.Generator(device=DEV).manual_seed(22)
    sum((o * torch.randn(o.shape, device=DEV, generator=g)).sum() for o in outs).backward()
    grads = {n: p.grad.clone() for n, p in m.named_parameters() if "_dec0." in n}
    grads.update({f"decoder{i}": t.grad.clone() for i, t in enumerate(cap[0])})
    return grads


@pytest.mark.parametrize("gru", [False, True])
def test_two_native_runs_through_the_model_give_the_same_bits(gru):
    m, sample = _model(gru), _sample(4)
    m.native_head_train = True
    heads.train_stats.update(dict.fromkeys(heads.train_stats, 0))
    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True  # (MIOpen's encoder / decoder forward: else the sources differ already)
    try:
        a, b = _heads_step(m, sample), _heads_step(m, sample)
    finally:
        torch.backends.cudnn.deterministic = det
    assert heads.train_stats == {"pre": 2, "dgrad": 2, "dgrad_single": 2, "wgrad": 2}
    assert len(a) == 10 and all(torch.equal(a[k], b[k]) for k in a), [k for k in a if not torch.equal(a[k], b[k])]
