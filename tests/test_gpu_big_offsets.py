"""GPU: every entry below on tensors whose last items start beyond 2^31 bytes (S1), 2^32 bytes (S2)
and 2^31 elements (S3) from the tensor's base: what a kernel does with a batch index.

The per-element tests pin every kernel on small tensors; none of them has an item that starts past
2^31 bytes, so a missing (long long) in ``b * HW``, a ``t * N`` plane index or a partial index held
in 32 bits would pass them all and return wrong depths for the later images of a large batch.
Here one operand per row is made that large (tests/_big_cases.py: the table, the periodic and the
sparse batch, and why a wrapped access cannot hide; tests/test_big_cases_cpu.py checks the table).

  * Periodic rows: the whole-batch output is the compact batch's output, tiled, BIT FOR BIT
    (_big_cases.first_mismatch, in slabs on the device).  The compact batch is what the
    per-element tests tie to float64 (_bwd_cases "big_compact", the head and S2D _case helpers).
  * Sparse row (propagation backward): zero items add exactly nothing, so every gradient of the
    non-zero items meets the existing per-element bar min(4 R32, ceiling) of
    tests/test_gpu_backward_elem.py against the float64 oracle of those items alone, dL/dgamma
    (whose partials per tile are indexed by batch) included, and every per-image gradient of a
    zero item is exactly 0.

Why bit-equality may be asked of the periodic rows: in none of these kernels does the summation
order of an image's result depend on B.
  * prop_step_kernel (nlspn_step.h): one workgroup per tile of one image; a pixel's taps are added
    in tap index order.  The resident kernel (nlspn_resident.h) cuts an image into parts by B, but
    runs the same per-pixel IEEE sequence: every form is pinned bit-equal to the oracle's loop
    (tests/test_gpu_forward_elem.py), so the compact batch (resident path) and the large one
    (step launches above 64 image groups) agree bit for bit.
  * affnorm_kernel / affnorm_bwd_kernel's dL/daff: per pixel, K terms in index order.  (The
    stand-alone normalisation's dL/dgamma is one sum over the batch in a B-dependent partition and
    is not asserted here; the section's dL/dgamma is, by the sparse row.)
  * heads_kernel / headsx3_kernel: one workgroup per 8 x 32 tile of one image, channel chunks and
    taps in a fixed order.  s2d_pyramid_kernel: per pixel.

The resident kernel's plan holds at most 64 image groups of one part per CU, so the step kernels
serve the rows above 16384 images whatever NLSPN_RESIDENT says; prop_res_s1 and prop_res_k17_s2 are
sized for the resident kernel (asserted through nlspn_resident_config) and run both ways.

  * The GRU-mode layers and their data gradients: see the comment above their tests (the reference
    is the large batch's own first period, tied to the compact batch by the bar of
    tests/test_gpu_gru.py, because nlspn_gconv picks 32-pixel tiles for small batches).
  * mdcn_forward_kernel: one thread's serial loop per output element.

Sparse rows besides the propagation backward: the three weight-gradient entries of the GRU-mode
layers in the conv role, the transposed-conv role (bias from the large tensor) and, for the f32 and
split-bf16 entries, the ConvGRU's stride-1 two-source shape (dW, db; bars of
tests/test_gpu_gconv_bwd_elem.py, tests/test_gpu_gwgrad16.py and tests/_gwnarrow_cases.py), and the
generic DCN's backward (bars of tests/test_gpu_dcn_elem.py).

The ConvGRU cell under gradients runs entry by entry through the raw C ABI, as _GruFn.backward
calls them (autograd's cell keeps a dozen state-sized tensors, above the 48 GiB cap at S2): the gate
derivatives stage 1 and 2, the two NLSPN_GC_DG_S1 data-gradient calls with two outputs (the second
adding in place) and the stride-1 weight gradient.  The training forward nlspn_gconv_gru_train is
nlspn_gconv's GRU1 / GRU2 launch with two more stores (r, q) and is held at size only through that
launch (gru_cell_fp32_s2).  The stand-alone normalisation's dL/dgamma is not asserted at size (no
existing bar for that sum).  The size guards are held by tests/test_capi_guards_cpu.py.

Memory: a test computes its peak from the table (<= 48 GiB), skips only when
torch.cuda.mem_get_info() shows less (recording big/<row>/ran = 0), asserts that the allocator's
peak stayed below the computed one and frees everything.

Rows: B, the tiers crossed, the allocator's peak in GiB and the wall seconds of the row (allocation,
fill, both runs and the comparison) measured in one run of the whole suite on an MI355X; every row
ran (big/<row>/ran = 1), the file takes under 20 s in all.  "/steps": with NLSPN_RESIDENT=0.

    row                          B      tiers     peak GiB  seconds
    prop_f32_s2                  58257  S1,S2     10.1      0.02
    prop_f32_s2/steps            58257  S1,S2     10.1      0.01
    prop_f32_s3                 116511  S1,S2,S3  19.9      0.86
    prop_f32_s3/steps           116511  S1,S2,S3  19.9      0.80
    prop_f16_s3                 116511  S1,S2,S3  10.1      0.02
    prop_f16_k17_s2              58257  S1,S2,S3   9.2      0.02
    prop_inter_s2 (T = 48)       29128  S1,S2      8.9      1.31
    prop_res_s1                   7284  S1         5.2      0.02
    prop_res_s1/steps             7284  S1         5.2      0.01
    prop_res_k17_s2              14566  S1,S2      9.2      0.02
    prop_res_k17_s2/steps        14566  S1,S2      9.2      0.01
    c4_global_batch                 32  -          -        0.02
    prop_bwd_s2                  58257  S1,S2     16.7      0.03
    affnorm_f32_s2              174765  S1,S2      8.8      1.77
    affnorm_f32_s3              349528  S1,S2,S3  17.3      0.01
    affnorm_f16_s3              349528  S1,S2,S3   8.8      0.01
    affnorm_bwd_s2              174765  S1,S2     12.8      1.15
    heads_fp32_s3               174765  S1,S2,S3  21.3      0.04
    heads_x3_s2                  87384  S1,S2     10.8      0.01
    heads_pro_fp32_s2            87384  S1,S2     12.0      1.44
    heads_pro_x3_s2              87384  S1,S2     12.0      0.02
    s2d_s2                       82244  S1,S2      4.5      0.02
    gru_enc_{fp32,fp16,bf16x3}   29130  S1,S2     12.9 8.9 13.0   0.08 0.03 0.03
    gru_cell_{fp32,fp16,bf16x3} 131075  S1,S2     24.1 24.1 32.1  2.22 0.14 1.68
    gru_dec_{fp32,fp16,bf16x3}   29130  S1,S2      9.8 10.7 14.7  0.09 0.04 0.06
    gru_dgrad_conv_s2            16387  S1,S2     14.1      1.96
    gru_dgrad_convt_s2           16387  S1,S2     16.1      0.04
    gwgrad_fp32_s2               16387  S1,S2      6.1      0.03
    gwgrad_bf16x3_s2              8195  S1,S2      5.1      0.03
    gwgrad_narrow_s2             16387  S1,S2      5.0      0.03
    gwgrad_{fp32,bf16x3,narrow}_t_s2  as the three rows above   0.03 0.02 0.03
    gwgrad_s1_{fp32,bf16x3}_s2  131075  S1,S2     12.0      0.13 0.19
    gates1_s2 / gates2_s2       131075  S1,S2     28.3 32.3 0.18 0.02
    gru_dgrad_cell_q_s2         131075  S1,S2     12.3      1.03
    gru_dgrad_cell_zr_s2         65539  S1,S2      8.3      0.11
    dcn_fwd_s2                 134963  S1,S2      7.2      0.02
    dcn_bwd_s2 (two placements) 134963  S1,S2     13.9      0.28 0.24

(The times above one second include a first kernel load or the model's construction.)
No defect was found: every row passed on its first run, with no kernel or host change.
"""
import os
import time

import numpy as np
import pytest
import torch

import _big_cases as big
import _big_checks as chk
import _bwd_cases as bc
from nlspn_eccv20_amd import _lib, affinity_normalization, propagate
from nlspn_eccv20_amd.heads import HeadWeights, head_epilogue, head_epilogue_prologue
from nlspn_eccv20_amd.propagation import _affnorm_backward
from nlspn_eccv20_amd.s2d import s2d_front
from nlspn_eccv20_amd.synthetic import rmse

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DT = {"f32": torch.float32, "f16": torch.float16}


class _Row:
    """A row's run: the memory gate, big/<row>/ran and big/<row>/seconds, and the clean-up."""

    def __init__(self, name, record_metric, tag=""):
        self.row, self.rec, self.key = big.ROW[name], record_metric, f"big/{name}{tag}"

    def __enter__(self):
        torch.cuda.empty_cache()
        need = big.peak_bytes(self.row)
        assert need <= big.MEM_CAP
        free = torch.cuda.mem_get_info(0)[0]
        if free < need:
            self.rec(self.key + "/ran", 0)
            pytest.skip(f"{free / big.GIB:.1f} GiB free, the row needs {need / big.GIB:.1f}")
        torch.cuda.reset_peak_memory_stats(0)
        self.t0 = time.perf_counter()
        return self.row

    def __exit__(self, et, ev, tb):
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated(0)
        torch.cuda.empty_cache()
        if et is None:
            assert peak <= big.peak_bytes(self.row), (peak / big.GIB, big.peak_bytes(self.row) / big.GIB)
            self.rec(self.key + "/ran", 1)
            self.rec(self.key + "/seconds", time.perf_counter() - self.t0)
            self.rec(self.key + "/peak_gib", peak / big.GIB)


class _env:
    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        self.old = os.environ.get(self.name)
        if self.value is not None:
            os.environ[self.name] = self.value

    def __exit__(self, *a):
        if self.value is not None:
            if self.old is None:
                os.environ.pop(self.name, None)
            else:
                os.environ[self.name] = self.old


def _dev(x, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV, dtype)


def _periodic(compact, B):
    """compact (k, ...) on the device -> (B, ...) with item b = compact[b mod k]."""
    return big.fill_periodic(torch.empty((B,) + tuple(compact.shape[1:]), dtype=compact.dtype, device=DEV), compact)


def _assert_tiled(name, out, compact_out):
    bad = big.first_mismatch(out, compact_out)
    assert bad is None, f"{name}: item {bad} of {out.shape[0]} differs from compact item {bad % compact_out.shape[0]}"


# ------------------------------------------------------------------ the propagation section
_PROP_CASE = {}


def _prop_compact(r):
    """The compact batch of a propagation row (numpy float32, k items, the last all zeros) and its
    _bwd_cases-style case: "big_compact" itself at its geometry, its like at another."""
    key = (r["H"], r["W"], r["kh"], r["kw"])
    if key not in _PROP_CASE:
        c = bc.CASES["big_compact"]
        if key != (c["H"], c["W"], c["kh"], c["kw"]):
            c = bc._case(r["k"] - 1, r["H"], r["W"], 3, kh=r["kh"], kw=r["kw"], seed=1000 + r["H"] + r["W"] + r["kw"])
        imgs = [bc._image(c, b, c["retry"].get(b, 0)) for b in range(r["k"] - 1)]
        s = {n: np.stack([im[n] for im in imgs] + [np.zeros_like(imgs[0][n])], 0) for n in ("pred_init", "dep", "conf")}
        s["off_aff"] = np.stack([np.concatenate([im["off"], im["aff"]], 0) for im in imgs]
                                + [np.zeros((3 * r["K"], r["H"], r["W"]), np.float32)], 0)
        _PROP_CASE[key] = (c, s)
    return _PROP_CASE[key]


def _propagate(r, pi, dep, conf, oa, gamma):
    K = r["K"]
    with torch.no_grad():
        return propagate(pi, dep, conf, oa[:, 2 * K:], oa[:, :2 * K], gamma, prop_time=r["T"], kernel=(r["kh"], r["kw"]))


def _resident(r):
    ok = _lib.get().nlspn_resident_config(0 if r["dtype"] == "f32" else 1, r["B"], r["H"], r["W"], r["kh"], r["kw"], r["T"],
                                          1, None, None, None)
    return bool(ok)


PROP_RUNS = [("prop_f32_s2", None), ("prop_f32_s2", "0"), ("prop_f32_s3", None), ("prop_f32_s3", "0"),
             ("prop_f16_s3", None), ("prop_f16_k17_s2", None), ("prop_inter_s2", None),
             ("prop_res_s1", None), ("prop_res_s1", "0"), ("prop_res_k17_s2", None), ("prop_res_k17_s2", "0")]


@pytest.mark.parametrize("name,resident_env", PROP_RUNS, ids=[n + ("" if e is None else "-steps") for n, e in PROP_RUNS])
def test_propagate_periodic(oracle, record_metric, name, resident_env):
    with _Row(name, record_metric, "" if resident_env is None else "/steps") as r, _env("NLSPN_RESIDENT", resident_env):
        c, s = _prop_compact(r)
        dt, B = DT[r["dtype"]], r["B"]
        gamma = torch.tensor([bc._gamma("TGASS", r["K"])], device=DEV)
        cin = {n: _dev(s[n], dt) for n in ("pred_init", "dep", "conf", "off_aff")}
        co = _propagate(r, cin["pred_init"], cin["dep"], cin["conf"], cin["off_aff"], gamma)
        if r["dtype"] == "f32" and r["T"] == 3:  # the compact batch itself, against the oracle (smoke's bar)
            K = r["K"]
            e = oracle.propagate(s["pred_init"], s["dep"], s["conf"], s["off_aff"][:, 2 * K:], s["off_aff"][:, :2 * K],
                                 float(gamma.item()), kh=r["kh"], kw=r["kw"], prop_time=r["T"])
            assert rmse(co["pred"].cpu().numpy(), e["pred"]) <= 1e-4
        if r.get("resident"):
            assert _resident(r) == (resident_env is None), "the row is sized for the resident kernel"
        bi = {n: _periodic(cin[n], B) for n in cin}
        assert bi[{"pred_inter_plane": "off_aff"}.get(r["tensor"], r["tensor"])].numel() * r["es"] > 1 << 31
        o = _propagate(r, bi["pred_init"], bi["dep"], bi["conf"], bi["off_aff"], gamma)
        torch.cuda.synchronize()
        _lib.check_resident(torch.device(DEV))
        if r["tensor"] == "pred_inter_plane":
            assert o["pred_inter_tensor"].numel() * r["es"] > 1 << 32
        for n in ("pred", "aff", "offset", "confidence"):
            _assert_tiled(n, o[n], co[n])
        for t in range(r["T"]):
            _assert_tiled(f"pred_inter[{t}]", o["pred_inter_tensor"][t], co["pred_inter_tensor"][t])
        del o, bi, co, cin


def test_c4_global_batch(record_metric):
    """C4 (KITTI 240 x 1216, global batch 32, T = 18): one call on the whole batch
    against propagate on its eight chunks of 4, the C3 shape that is held against the oracle at full
    size.  Bit for bit, every output."""
    c = big.C4
    B, H, W, K, T = c["B"], c["H"], c["W"], c["K"], c["T"]
    t0 = time.perf_counter()
    g = torch.Generator(device=DEV).manual_seed(32)
    r = lambda *sh: torch.rand(sh, device=DEV, generator=g)  # noqa: E731
    pi, conf = r(B, 1, H, W) * 10, r(B, 1, H, W)
    dep = r(B, 1, H, W) * 10 * (r(B, 1, H, W) < 0.05)
    oa = torch.randn((B, 3 * K, H, W), device=DEV, generator=g)
    oa[:, :2 * K] *= 2.0
    gamma = torch.tensor([4.0], device=DEV)
    run = lambda s: propagate(pi[s], dep[s], conf[s], oa[s, 2 * K:], oa[s, :2 * K], gamma, prop_time=T)  # noqa: E731
    with torch.no_grad():
        whole = run(slice(0, B))
        for b0 in range(0, B, c["chunk"]):
            part = run(slice(b0, b0 + c["chunk"]))
            for n in ("pred", "aff", "offset", "confidence"):
                assert torch.equal(whole[n][b0:b0 + c["chunk"]].view(torch.int32), part[n].view(torch.int32)), (n, b0)
            assert torch.equal(whole["pred_inter_tensor"][:, b0:b0 + c["chunk"]].view(torch.int32),
                               part["pred_inter_tensor"].view(torch.int32)), b0
    torch.cuda.synchronize()
    _lib.check_resident(torch.device(DEV))
    assert torch.isfinite(whole["pred"]).all()
    del whole, part, pi, conf, dep, oa
    torch.cuda.empty_cache()
    record_metric("big/c4_global_batch/ran", 1)
    record_metric("big/c4_global_batch/seconds", time.perf_counter() - t0)


# ------------------------------------------------------------------ the propagation backward, sparse batch
def test_propagate_backward_sparse(oracle, record_metric):
    name = "big_compact"
    with _Row("prop_bwd_s2", record_metric) as r:
        c = bc.CASES[name]
        K, T, B, H, W = r["K"], r["T"], r["B"], r["H"], r["W"]
        oracle.set_threads(16)
        s = bc.grid_inputs(name)
        g64, X, info = bc.oracle_bound(oracle, name, s)
        items = big.sparse_items(r)
        assert len(items) == c["B"]
        z = lambda *sh: torch.zeros(sh, device=DEV)  # noqa: E731
        put = lambda t, dense: big.scatter_sparse(t, items, _dev(dense))  # noqa: E731
        oa = put(z(B, 3 * K, H, W), np.concatenate([s["off"], s["aff"]], 1)).requires_grad_(True)
        pi = put(z(B, 1, H, W), s["pred_init"]).requires_grad_(True)
        cf = put(z(B, 1, H, W), s["conf"]).requires_grad_(True)
        dep = put(z(B, 1, H, W), s["dep"])
        gp = put(z(B, 1, H, W), s["grad_pred"])
        gi = z(T, B, 1, H, W)
        for t in range(T):
            put(gi[t], s["grad_inter"][t])
        assert oa.numel() * 4 > 1 << 32
        gamma = torch.tensor([bc.gamma_of(name)], device=DEV, requires_grad=True)
        o = propagate(pi, dep, cf, oa[:, 2 * K:], oa[:, :2 * K], gamma, prop_time=T)
        torch.autograd.backward([o["pred"], o["pred_inter_tensor"]], [gp, gi])
        torch.cuda.synchronize()
        for n, t in (("off_aff", oa.grad), ("pred_init", pi.grad), ("confidence", cf.grad)):
            assert not big.nonzero_outside(t, items), f"dL/d{n}: a zero item has a non-zero gradient"
        ga = oa.grad[items].cpu().numpy()
        got = {"pred_init": pi.grad[items].cpu().numpy(), "aff": ga[:, 2 * K:], "offset": ga[:, :2 * K],
               "confidence": cf.grad[items].cpu().numpy(), "gamma": np.float32(gamma.grad.item())}
        del o, oa, pi, cf, dep, gp, gi
        def note(t, ratio, cbar):
            record_metric(f"big/prop_bwd_s2/{t}", ratio)
            print(f"big prop_bwd_s2 {t}: worst (err - Q)/X = {ratio:.3e}, bar c = {cbar:.3e}")

        failures = chk.backward_failures(name, got, g64, X, info, note)  # the bar of tests/test_gpu_backward_elem.py
        assert not failures, "\n".join(failures) + f" (sparse items {items})"


# ------------------------------------------------------------------ the stand-alone affinity normalisation
def _aff_compact(r):
    return _prop_compact(r)[1]["off_aff"][:, 2 * r["K"]:]


@pytest.mark.parametrize("name", ["affnorm_f32_s2", "affnorm_f32_s3", "affnorm_f16_s3"])
def test_affinity_normalization_periodic(oracle, record_metric, name):
    with _Row(name, record_metric) as r:
        a = _aff_compact(r)
        gamma = torch.tensor([4.0], device=DEV)
        ca = _dev(a, DT[r["dtype"]])
        co = affinity_normalization(ca, gamma, "TGASS")
        if r["dtype"] == "f32":  # the compact batch against float64: the bar of tests/_fwd_cases.py
            import _fwd_cases as fc
            a64 = oracle.affinity_normalization(a.astype(np.float64), "TGASS", 4.0)
            ref = r["K"] // 2
            X = np.abs(a64)  # |a_k| for the K taps, 1 + sum |a_k| for the reference tap
            X[:, ref] = 1.0 + np.delete(X, ref, 1).sum(1)
            err = np.abs(co.double().cpu().numpy() - a64)
            cbar = np.full((1, r["K"] + 1, 1, 1), min(4.0 * fc.A32["TGASS"][r["K"]][0], fc.aff_ceiling(r["K"])))
            cbar[0, ref] = min(4.0 * fc.A32["TGASS"][r["K"]][1], fc.aff_ceiling(r["K"]))
            assert (err <= cbar * X).all()
        x = _periodic(ca, r["B"])
        assert x.numel() * r["es"] > 1 << 32
        out = affinity_normalization(x, gamma, "TGASS")
        _assert_tiled("aff", out, co)
        del out, x


def test_affinity_normalization_backward_periodic(record_metric):
    with _Row("affnorm_bwd_s2", record_metric) as r:
        a = _aff_compact(r)
        k = a.shape[0]
        gamma = torch.tensor([4.0], device=DEV)
        go = np.random.default_rng(77).standard_normal((k, r["K"] + 1, r["H"], r["W"])).astype(np.float32)
        go[k - 1] = 0
        ca, cg = _dev(a), _dev(go)
        cr = _affnorm_backward(ca, gamma, cg, "TGASS")[0]
        assert torch.isfinite(cr).all() and not cr[k - 1].any() and cr[0].any()
        x, g = _periodic(ca, r["B"]), _periodic(cg, r["B"])
        assert x.numel() * 4 > 1 << 32
        gr = _affnorm_backward(x, gamma, g, "TGASS")[0]
        _assert_tiled("dL/daff", gr, cr)
        del gr, x, g


# ------------------------------------------------------------------ the head epilogue
def _head_case(r, prologue):
    """C = 16, nout = 24, k = 3 compact items (the last zero); one tensor is all four sources."""
    if prologue:
        from test_gpu_heads_prologue import _case
        oa, idc, cfc, src, dep = _case(r["k"], r["C"], r["H"], r["W"], seed=5)
    else:
        from test_gpu_heads import _case
        (oa, idc, cfc, src), dep = _case(r["k"], r["C"], r["H"], r["W"], 24, seed=5), None
    x = src[0].clone()
    x[r["k"] - 1] = 0
    if dep is not None:
        dep[r["k"] - 1] = 0
    return oa, idc, cfc, x, dep


@pytest.mark.parametrize("name,precision", [("heads_fp32_s3", "fp32"), ("heads_x3_s2", "bf16x3")])
def test_head_epilogue_periodic(record_metric, name, precision):
    with _Row(name, record_metric) as r:
        oa, idc, cfc, x, _ = _head_case(r, False)
        hw = HeadWeights()
        with torch.no_grad():
            cp, co, cc = head_epilogue(x, x, oa, x, idc, x, cfc, weights=hw, precision=precision)
            X = _periodic(x, r["B"])
            assert X.numel() * 4 > 1 << 32
            p, o, c = head_epilogue(X, X, oa, X, idc, X, cfc, weights=hw, precision=precision)
        assert torch.isfinite(co).all() and co[0].any()
        for n, a, b in (("pred_init", p, cp), ("off_aff", o, co), ("confidence", c, cc)):
            _assert_tiled(n, a, b)
        del p, o, c, X


@pytest.mark.parametrize("name,precision", [("heads_pro_fp32_s2", "fp32"), ("heads_pro_x3_s2", "bf16x3")])
def test_head_epilogue_prologue_periodic(record_metric, name, precision):
    with _Row(name, record_metric) as r:
        oa, idc, cfc, x, dep = _head_case(r, True)
        hw = HeadWeights()
        gamma = torch.tensor([4.0], device=DEV)
        with torch.no_grad():
            ch = head_epilogue_prologue(x, x, oa, x, idc, dep, gamma, "TGASS", x, cfc, True, False, weights=hw,
                                        precision=precision)
            X, D = _periodic(x, r["B"]), _periodic(dep, r["B"])
            assert X.numel() * 4 > 1 << 32
            h = head_epilogue_prologue(X, X, oa, X, idc, D, gamma, "TGASS", X, cfc, True, False, weights=hw,
                                       precision=precision)
        assert torch.isfinite(ch["aff"]).all() and ch["offset"][0].any()
        for n in ("pred_init", "offset", "aff", "confidence", "p0"):
            _assert_tiled(n, h[n], ch[n])
        del h, X, D


# ------------------------------------------------------------------ the S2D front
def test_s2d_front_periodic(oracle, record_metric):
    from test_gpu_s2d import _case
    with _Row("s2d_s2", record_metric) as r:
        dep, w1, b1, w2, b2 = _case(r["k"], r["H"], r["W"], 0.05, seed=11)
        dep[r["k"] - 1] = 0
        ref_out, _ = oracle.s2d_front(*(a.numpy() for a in (dep, w1, b1, w2, b2)))
        cd, w1, b1, w2, b2 = (a.to(DEV) for a in (dep, w1, b1, w2, b2))
        with torch.no_grad():
            co = s2d_front(cd, w1, b1, w2, b2)
            np.testing.assert_allclose(co.cpu().numpy(), ref_out, rtol=1e-5, atol=1e-5)  # the bar of tests/test_gpu_s2d.py
            D = _periodic(cd, r["B"])
            out = s2d_front(D, w1, b1, w2, b2)
        assert out.numel() * 4 > 1 << 32
        _assert_tiled("out", out, co)
        del out, D


# ------------------------------------------------------------------ the GRU-mode layers at inference
# The reference of these rows is the large batch's own first period (items 0 .. k - 1, at offsets every
# small test covers), tiled bit for bit; that first period is tied to the compact batch's output by the
# bar of tests/test_gpu_gru.py (relative L2 <= 1e-5).  Not bit-equality there: nlspn_gconv switches a
# small batch to 32-pixel tiles (NLSPN_GC_S2_N32 / NLSPN_GC_GRU2_N32, a choice that depends on B), which
# is another build of the same sums.  Within one launch every image runs the same build.
_GRU = {}


def _gru_model():
    if "m" not in _GRU:
        from test_gpu_gru import _model
        _GRU["m"] = _model(64, 64, seed=5)
    return _GRU["m"]


def _rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def _gru_api(gc, m, precision):
    """(P, encode_dep, encode_aff, gru, decode_aff) of a precision; states are tuples in the matrix-core modes."""
    if precision == "fp32":
        P = gc.pack(m)
        return (P, lambda x: (gc.encode_dep(P, x, m.args.max_depth),), lambda a: (gc.encode_aff(P, a),),
                lambda h, x: (gc.gru(P, h[0], x[0]),), lambda h, g: gc.decode_aff(P, h[0], (64, 64), gamma=g, kind="TGASS"))
    P, enc_d, enc_a, cell, dec = ((gc.pack16(m), gc.encode_dep16, gc.encode_aff16, gc.gru16, gc.decode_aff16)
                                  if precision == "fp16" else
                                  (gc.pack_x3(m), gc.encode_dep_x3, gc.encode_aff_x3, gc.gru_x3, gc.decode_aff_x3))
    return (P, lambda x: (enc_d(P, x, m.args.max_depth),), lambda a: tuple(enc_a(P, a)), lambda h, x: tuple(cell(P, h, x[0])),
            lambda h, g: dec(P, h, (64, 64), gamma=g, kind="TGASS"))


def _gru_compact(k, seed=21):
    g = torch.Generator(device=DEV).manual_seed(seed)
    new_pred = torch.rand((k, 1, 64, 64), device=DEV, generator=g) * 10
    aff = torch.rand((k, 9, 64, 64), device=DEV, generator=g) - 0.3
    new_pred[k - 1] = 0
    aff[k - 1] = 0
    return new_pred, aff


def _assert_own_period(name, out, compact_out):
    k = compact_out.shape[0]
    r = _rel(out[:k], compact_out)
    assert r <= 1e-5, f"{name}: the first period against the compact batch, relative L2 {r:.3g}"
    _assert_tiled(name, out, out[:k].clone())


GRU_ROWS = [(f"gru_{what}_{p}_s2", what, p) for what in ("enc", "cell", "dec") for p in ("fp32", "fp16", "bf16x3")]


@pytest.mark.parametrize("name,what,precision", GRU_ROWS, ids=[r[0] for r in GRU_ROWS])
def test_gru_mode_layers_periodic(record_metric, name, what, precision):
    from nlspn_eccv20_amd.gru import GruConvs
    with _Row(name, record_metric) as r, torch.no_grad():
        m, gc, B = _gru_model(), GruConvs(), r["B"]
        P, enc_d, enc_a, cell, dec = _gru_api(gc, m, precision)
        gamma = torch.tensor([4.0], device=DEV)
        new_pred, aff = _gru_compact(r["k"])
        cx, ch = enc_d(new_pred), enc_a(aff)
        if what == "enc":
            A = _periodic(aff, B)
            assert A.numel() * 4 > 1 << 32
            for i, (o, c) in enumerate(zip(enc_a(A), ch)):
                _assert_own_period(f"encode_aff[{i}]", o, c)
        elif what == "cell":
            chn = cell(ch, cx)
            Hs, Xs = tuple(_periodic(t, B) for t in ch), tuple(_periodic(t, B) for t in cx)
            assert Hs[0].numel() * 4 > 1 << 32
            for i, (o, c) in enumerate(zip(cell(Hs, Xs), chn)):
                _assert_own_period(f"gru[{i}]", o, c)
        else:
            co = dec(ch, gamma)
            out = dec(tuple(_periodic(t, B) for t in ch), gamma)
            assert out.numel() * 4 > 1 << 32 and tuple(out.shape[1:]) == (9, 64, 64)
            _assert_own_period("decode_aff", out, co)


# ------------------------------------------------------------------ the GRU-mode layers under gradients (native f32)
@pytest.mark.parametrize("name", ["gru_dgrad_conv_s2", "gru_dgrad_convt_s2"])
def test_gru_mode_data_gradient_periodic(record_metric, name):
    """dL/dx of one layer through GruConvs.layer and autograd (the data-gradient launch and the
    activation derivative), periodic batch: the reference as for the forward rows above."""
    import torch.nn as nn
    from nlspn_eccv20_amd.gru import ACT_RELU, GruConvs
    with _Row(name, record_metric) as r:
        torch.manual_seed(13)
        tr = name == "gru_dgrad_convt_s2"
        conv = (nn.ConvTranspose2d(32, 16, 3, 2, 1, 1) if tr else nn.Conv2d(16, 32, 3, 2, 1)).to(DEV)
        gc, k, B = GruConvs(), r["k"], r["B"]
        g = torch.Generator(device=DEV).manual_seed(17)
        cx = torch.randn((k, 32, 32, 32) if tr else (k, 16, 64, 64), device=DEV, generator=g)
        cg = torch.randn((k, 16, 64, 64) if tr else (k, 32, 32, 32), device=DEV, generator=g)
        cx[k - 1] = 0
        cg[k - 1] = 0

        def grad_x(x, go):
            x = x.requires_grad_(True)
            y = gc.layer(conv, x, ACT_RELU)
            y.backward(go)
            return y.detach(), x.grad

        cy, cdx = grad_x(cx, cg)
        x2 = cx.detach().clone().requires_grad_(True)  # the module's own autograd on the compact batch: the bar of tests/test_gpu_gru.py
        torch.relu(conv(x2)).backward(cg)
        assert _rel(cdx, x2.grad) <= 1e-5
        X, G = _periodic(cx.detach(), B), _periodic(cg, B)
        y, dx = grad_x(X, G)
        assert max(X.numel(), y.numel()) * 4 > 1 << 32
        _assert_own_period("y", y, cy)
        _assert_own_period("dL/dx", dx, cdx)
        del X, G, y, dx
        conv.zero_grad(set_to_none=True)


# (row, entry, c of dW; None: C_BAR of tests/test_gpu_gwgrad16.py).  "_t_": the transposed-conv role;
# "gwgrad_s1_": the ConvGRU's stride-1 weight gradient with two sources (l0 = r*h or h, l1 = x).
GW_ROWS = [(n.format(t), e, c) for t in ("", "_t") for n, e, c in (
    ("gwgrad_fp32{}_s2", "nlspn_gconv_wgrad", 2e-6), ("gwgrad_bf16x3{}_s2", "nlspn_gconv_wgrad_bf16x3", None),
    ("gwgrad_narrow{}_s2", "nlspn_gconv_wgrad_narrow", 2e-6))] + [
    ("gwgrad_s1_fp32_s2", "nlspn_gconv_wgrad", 2e-6), ("gwgrad_s1_bf16x3_s2", "nlspn_gconv_wgrad_bf16x3", None)]


@pytest.mark.parametrize("name,entry,cbar", GW_ROWS, ids=[r[0] for r in GW_ROWS])
def test_gconv_wgrad_sparse(record_metric, name, entry, cbar):
    """dW and db of the weight-gradient entries on the sparse batch, per element against float64 on
    the non-zero items: |got - ref| <= c sum |s| |l| with the entry's existing c -- 2e-6 (the cap of
    min(2e-6, (n + slices + 2) 2^-24), which binds from 32 terms on) for the f32 and the narrow entry,
    C_BAR of tests/test_gpu_gwgrad16.py for the split-bf16 one; db <= 2e-6 sum |g|.
    Stride 2: s (B, Cs, 32, 32), l (B, Cl, 64, 64); the conv role (s the output gradient, db from s)
    and the transposed-conv role (s the input, l the signed output gradient, db from l).
    Stride 1: the ConvGRU's shape, s (B, 128, 8, 8) and l = [l0; l1] of 128 channels each."""
    from _gconv_bwd_cases import wgrad_reference
    if cbar is None:
        from test_gpu_gwgrad16 import C_BAR as cbar
    with _Row(name, record_metric) as r:
        s1 = "_s1_" in name
        bfl = bool(r.get("bfl"))
        stride, B = (1, r["B"]) if s1 else (2, r["B"])
        Cs, c0, c1 = (128, 128, 128) if s1 else (r["Cs"], r["Cl"], 0)
        (Hs, Ws), (Hl, Wl) = ((8, 8), (8, 8)) if s1 else ((32, 32), (64, 64))
        items = big.sparse_items(r)
        gen = torch.Generator().manual_seed(23)
        s = torch.randn((len(items), Cs, Hs, Ws), generator=gen)
        l = torch.randn((len(items), c0 + c1, Hl, Wl), generator=gen)
        if not bfl:
            l = torch.relu(l)
        ref, mag = wgrad_reference(stride, s, l)
        put = lambda t: big.scatter_sparse(torch.zeros((B,) + tuple(t.shape[1:]), device=DEV), items, t.contiguous().to(DEV))  # noqa: E731
        S, L0 = put(s), put(l[:, :c0])
        L1 = put(l[:, c0:]) if c1 else None
        assert L0.numel() * 4 > 1 << 32
        need = getattr(_lib.get(), entry + "_workspace_bytes")(stride, Cs, c0 + c1, B, Hs, Ws, Hl, Wl)
        assert need > 0
        ws = torch.empty((need + 3) // 4, device=DEV)
        dw = torch.full((Cs, c0 + c1, 3, 3), float("nan"), device=DEV)
        db = torch.full((c0 if bfl else Cs,), float("nan"), device=DEV)
        _lib.call(entry, torch.device(DEV), stride, S, Cs, L0, c0, L1, c1, dw, db, int(bfl), 1.0, ws, ws.numel() * 4, B,
                  Hs, Ws, Hl, Wl, _lib.STREAM)
        torch.cuda.synchronize()
        dw, db = dw.cpu().double(), db.cpu().double()
        assert torch.isfinite(dw).all() and torch.isfinite(db).all() and float(mag.min()) > 0
        g = (l if bfl else s).double()
        rw = float(((dw - ref).abs() / mag).max())
        rb = float(((db - g.sum((0, 2, 3))).abs() / g.abs().sum((0, 2, 3))).max())
        record_metric(f"big/{name}/dw_ratio", rw)
        record_metric(f"big/{name}/db_ratio", rb)
        print(f"big {name}: dW worst |err| / sum |s||l| = {rw:.3e} (bar {cbar:.3e}), db {rb:.3e} (bar 2e-6)")
        assert rw <= cbar and rb <= 2e-6, (rw, cbar, rb)
        del S, L0, L1, ws


# ------------------------------------------------------------------ the ConvGRU cell under gradients, entry by entry
@pytest.mark.parametrize("stage", [1, 2])
def test_gate_derivatives_periodic(record_metric, stage):
    """nlspn_gconv_gru_gates_backward as _GruFn.backward calls it, on the periodic batch: stage 1 writes
    du_q and the du_z half of the NaN-filled (B, 2 hc, H, W) tensor, stage 2 the du_r half and dh.  The
    kernel is elementwise: the tiled compact output is the reference, bit for bit (the NaN half
    included), and the compact output meets C_GATES of tests/test_gpu_gconv_bwd_elem.py against float64."""
    import _gconv_bwd_cases as gb
    with _Row(f"gates{stage}_s2", record_metric) as r:
        cid = gb.BIG_GATES["id"]
        o = gb.gate_operands(cid)
        B, k, hc = r["B"], r["k"], 128
        want = gb.gate_formulas(cid, torch.float64, stage=stage)
        names = ("dhn", "z", "q", "h") if stage == 1 else ("dhn", "z", "r", "h", "drh")
        c = {n: o[n].to(DEV) for n in names}

        def run(d, n):
            nan = lambda *sh: torch.full(sh, float("nan"), device=DEV)  # noqa: E731
            duzr = nan(n, 2 * hc, 8, 8)
            if stage == 1:
                out = {"duq": nan(n, hc, 8, 8), "duzr": duzr}
                args = (d["dhn"], d["z"], None, d["q"], d["h"], None, out["duq"], duzr, None)
            else:
                out = {"duzr": duzr, "dh": nan(n, hc, 8, 8)}
                args = (d["dhn"], d["z"], d["r"], None, d["h"], d["drh"], None, duzr, out["dh"])
            _lib.call("nlspn_gconv_gru_gates_backward", torch.device(DEV), stage, *args, gb.ACT_NONE, n, hc, 8, 8, _lib.STREAM)
            return out

        co = run(c, k)
        torch.cuda.synchronize()
        half = co["duzr"][:, :hc] if stage == 1 else co["duzr"][:, hc:]
        other = co["duzr"][:, hc:] if stage == 1 else co["duzr"][:, :hc]
        assert bool(torch.isnan(other).all())  # only its own half is written
        got = {"duq": co["duq"], "duz": half} if stage == 1 else {"dur": half, "dh": co["dh"]}
        for n, (ref, X) in want.items():
            gb.check(f"big/gates{stage}/{n}", got[n].cpu(), ref, X, gb.C_GATES)
        big_in = {n: _periodic(t, B) for n, t in c.items()}
        assert big_in["h"].numel() * 4 > 1 << 32
        out = run(big_in, B)
        for n in out:
            _assert_tiled(n, out[n], co[n])
        del out, big_in


@pytest.mark.parametrize("which", ["q", "zr"])
def test_cell_data_gradient_periodic(record_metric, which):
    """The ConvGRU's two data-gradient calls (NLSPN_GC_DG_S1, two outputs): convq's adjoint into
    d(rh) and dx, then [convz; convr]'s added into dh and dx IN PLACE.  The first period of the large
    batch meets the per-element bar of tests/test_gpu_gconv_bwd_elem.py against float64 (c = min(2e-6,
    (n + 4) 2^-24) times the sum of the absolute terms), and the whole batch is that period tiled, bit
    for bit: one launch runs one build, and a workgroup sums one image's tile in a fixed order."""
    import _gconv_bwd_cases as gb
    from test_gpu_gconv_bwd_elem import _pack
    with _Row(f"gru_dgrad_cell_{which}_s2", record_metric) as r:
        c = gb.BIG_DG_Q if which == "q" else gb.BIG_DG_ZR
        o, R = gb.dgrad_operands(c["id"]), gb.dgrad_reference(c["id"])
        B, k, split, cout = r["B"], r["k"], c["split"], c["cout"]
        assert c["cg"] == r["cg"] and c["add"] == r["add"] and c["B"] == k
        wpk = _pack(c, o["w"])
        G = _periodic(o["g"].to(DEV), B)
        if c["add"] == "alias":   # the outputs hold the addends
            dx0 = _periodic(o["add"][:, :split].contiguous().to(DEV), B)
            dx1 = _periodic(o["add"][:, split:].contiguous().to(DEV), B)
            a0, a1 = dx0, dx1
        else:
            dx0, dx1 = (torch.full((B, n, 8, 8), float("nan"), device=DEV) for n in (split, cout - split))
            a0 = a1 = None
        assert max(G.numel(), dx0.numel()) * 4 > 1 << 32
        _lib.call("nlspn_gconv_dgrad", torch.device(DEV), c["preset"], G, c["cg"], wpk, None, a0, a1, dx0, dx1, split, B, 8, 8,
                  cout, 8, 8, c["act"], c["scale"], _lib.STREAM)
        torch.cuda.synchronize()
        first = torch.cat([dx0[:k], dx1[:k]], 1).cpu()
        gb.check(f"big/dgrad_cell_{which}", first, R["ref"], R["X"], R["c"], R["e"])
        _assert_tiled("dx0", dx0, dx0[:k].clone())
        _assert_tiled("dx1", dx1, dx1[:k].clone())
        del G, dx0, dx1


# ------------------------------------------------------------------ the generic DCN (f32, groups)
def _dcn_inputs():
    case = bc.dcn_cases()[big.DCN_CASE]
    return case, bc.dcn_inputs(100 + big.DCN_CASE, *case)  # the B = 2 inputs tests/test_gpu_dcn_elem.py checks per element


def test_dcn_forward_periodic(oracle, record_metric):
    """mdcn_forward_kernel sums one output element's taps and channels in a serial loop of its own
    thread: the order cannot depend on B, so the tiled compact output is the reference, bit for bit."""
    from nlspn_eccv20_amd import dcn
    from test_gpu_dcn import rel
    with _Row("dcn_fwd_s2", record_metric) as r:
        case, (inp, wt, bias, off, mask, _) = _dcn_inputs()
        C, Cout, group, dg, kh, kw, stride, pad, dil = case
        z = lambda a: np.concatenate([a, np.zeros_like(a[:1])], 0)  # noqa: E731  (k = 3: the two images and a zero item)
        ci, co_, cm = _dev(z(inp)), _dev(z(off)), _dev(z(mask))
        w, b = _dev(wt), _dev(bias)
        run = lambda i, o, m: dcn.modulated_deform_conv_forward(i, w, b, o, m, kh, kw, *stride, *pad, *dil, group, dg, 64)  # noqa: E731
        cout = run(ci, co_, cm)
        exp = oracle.mdcn_forward(*(x.astype(np.float64) for x in (inp, wt, bias, off, mask)), stride, pad, dil, group, dg)
        assert rel(cout[:2].cpu().numpy(), exp) <= 1e-5  # the bar of tests/test_gpu_dcn.py
        O = _periodic(co_, r["B"])
        assert O.numel() * 4 > 1 << 32
        out = run(_periodic(ci, r["B"]), O, _periodic(cm, r["B"]))
        _assert_tiled("out", out, cout)
        del out, O


@pytest.mark.parametrize("pair", ["ends", "boundaries"])
def test_dcn_backward_sparse(oracle, record_metric, pair):
    """Every gradient of the DCN backward on the sparse batch, per element against the float64 oracle
    of the two non-zero images with the bars of tests/test_gpu_dcn_elem.py (min(4 DCN_R32, ceiling),
    the very inputs those bars were measured on); the images sit at items 0 and B - 1 ("ends") or at
    the first items beyond 2^31 and 2^32 bytes ("boundaries").  grad_weight and grad_bias are sums
    over the batch; every per-image gradient of a zero item is exactly 0."""
    from nlspn_eccv20_amd import dcn
    with _Row("dcn_bwd_s2", record_metric, "/" + pair) as r:
        case, (inp, wt, bias, off, mask, go) = _dcn_inputs()
        C, Cout, group, dg, kh, kw, stride, pad, dil = case
        B, s = r["B"], big.sparse_items(r)
        items = [s[0], s[-1]] if pair == "ends" else s[1:3]
        assert len(s) == 4 and (pair == "ends" or big.start_offsets(r, items[0])[0] > 1 << 31)
        put = lambda a: big.scatter_sparse(torch.zeros((B,) + a.shape[1:], device=DEV), items, _dev(a))  # noqa: E731
        I, O, M, G = put(inp), put(off), put(mask), put(go)
        assert O.numel() * 4 > 1 << 32
        gi, goff, gm, gw, gb = dcn.modulated_deform_conv_backward(I, _dev(wt), _dev(bias), O, M, G, kh, kw, *stride, *pad, *dil,
                                                                  group, dg, 64)
        torch.cuda.synchronize()
        for n, t in (("input", gi), ("offset", goff), ("mask", gm)):
            assert not big.nonzero_outside(t, items), f"grad_{n}: a zero item has a non-zero gradient"
        got = {"input": gi[items].cpu().numpy(), "offset": goff[items].cpu().numpy(), "mask": gm[items].cpu().numpy(),
               "weight": gw.cpu().numpy(), "bias": gb.cpu().numpy()}
        del I, O, M, G, gi, goff, gm
        g64, X = oracle.mdcn_backward_bound(*(a.astype(np.float64) for a in (inp, wt, off, mask, go)), stride, pad, dil,
                                            group, dg)
        failures = []
        for t, want, bound in zip(bc.DCN_TENSORS, g64, X):
            cbar = min(4.0 * bc.DCN_R32[big.DCN_CASE][t], bc.dcn_ceiling(case, t))
            ratio, zeros_ok, k = bc.ratio(got[t], want, bound)
            record_metric(f"big/dcn_bwd_s2/{pair}/{t}", ratio)
            print(f"big dcn_bwd_s2 {pair} {t}: worst err/X = {ratio:.3e}, bar c = {cbar:.3e}")
            if not zeros_ok:
                failures.append(f"{t}: an element whose bound is 0 is not exactly 0")
            if not ratio <= cbar:
                failures.append(f"{t}: worst err/X {ratio:.3e} > c {cbar:.3e} at {np.unravel_index(k, bound.shape)}")
        assert not failures, "\n".join(failures) + f" (items {items})"
