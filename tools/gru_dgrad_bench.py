#!/usr/bin/env python
"""The split-bf16 data gradients (nlspn_gconv_x3_dgrad, csrc/nlspn_gconv_x3.h) against the f32
entry (nlspn_gconv_dgrad) of the same library, in one process, the variants alternating.

(a) Per call: every data-gradient kind of the GRU-mode section at the training benchmark's shapes
    (NYU 228x304, B=8, hidden 128) through the C ABI on the same operands: the ConvGRU's two
    adjoints, the adjoints of the 2hc -> hc and 16 -> 2hc encoder convs and of the hc -> 2hc and
    2hc -> 16 decoder layers (the last two measured last, as the smallest).  The new entry's time
    includes what that kind needs around it in a chain: the nlspn_gconv_x3_split launch where its
    gradient enters in f32, and the split copy of its output where the next data gradient reads
    it.  Every round times each variant once (device events around `--calls` calls); reported:
    mean, min, max and range of the per-round means and whether the ranges are apart.
(b) The gate stages' outputs: the two nlspn_gconv_x3_split launches of a ConvGRU backward, timed
    alone (what fusing the split stores into the gate kernel could save at most).
(c) The whole training step of DESIGN.md 3.8.1 (propagate_heads forward + backward, T=18) on top
    of gru_wgrad_precision = "bf16x3" + gru_wgrad_narrow = True: native with
    gru_dgrad_precision = "bf16x3", native without it, modules (MIOpen defaults), modules_tuned
    (channels_last + algorithm search), as tools/gru_wgrad_bench.py times them.
(d) The relative L2 of every parameter gradient of that step against the all-"fp32" native step.

Writes JSON (default profiles/gru_dgrad_x3_bench.json).  No GPU: an error.
"""
import argparse
import copy
import json
import os
import sys

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from gru_wgrad_bench import build, summary  # noqa: E402
from nlspn_eccv20_amd import _lib  # noqa: E402
from nlspn_eccv20_amd import gru as G  # noqa: E402


def kinds(a):
    half = lambda n: (n - 1) // 2 + 1  # noqa: E731
    H4, W4, H8, W8 = half(half(a.H)), half(half(a.W)), half(half(half(a.H))), half(half(half(a.W)))
    hc = a.hidden
    # name, forward module (None: the stride-1 adjoint), cg, cout, (Hg, Wg), (Ho, Wo), split, act, add,
    # the gradient enters in f32 (a split launch), the next data gradient reads the split copy
    return [("GRU convq adjoint", None, hc, 2 * hc, (H8, W8), (H8, W8), hc, G.ACT_NONE, False, True, False),
            ("GRU [convz; convr] adjoint", None, 2 * hc, 2 * hc, (H8, W8), (H8, W8), hc, G.ACT_NONE, True, True, False),
            ("adjoint of conv 2hc->hc at 1/8", nn.Conv2d(2 * hc, hc, 3, 2, 1), hc, 2 * hc, (H8, W8), (H4, W4), 2 * hc,
             G.ACT_RELU, False, True, True),
            ("adjoint of convT hc->2hc from 1/8", nn.ConvTranspose2d(hc, 2 * hc, 3, 2, 1, 1), 2 * hc, hc, (2 * H8, 2 * W8),
             (H8, W8), hc, G.ACT_NONE, False, a.all_kinds is False, False),
            ("adjoint of conv 16->2hc at 1/4", nn.Conv2d(16, 2 * hc, 3, 2, 1), 2 * hc, 16, (H4, W4), (2 * H4, 2 * W4), 16,
             G.ACT_RELU, False, False, False),
            ("adjoint of convT 2hc->16 from 1/4", nn.ConvTranspose2d(2 * hc, 16, 3, 2, 1, 1), 16, 2 * hc, (4 * H8, 4 * W8),
             (2 * H8, 2 * W8), 2 * hc, G.ACT_RELU, False, True, True)]


def timed(run, rounds, calls):
    times = {m: [] for m in run}
    for _ in range(rounds):
        for mode, call in run.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                call()
            e1.record()
            e1.synchronize()
            times[mode].append(e0.elapsed_time(e1) / calls)
    return {m: summary(t) for m, t in times.items()}


def bench_calls(a, dev):
    lib = _lib.get()
    gen = torch.Generator(device=dev).manual_seed(2)
    out = []
    for name, mod, cg, cout, (Hg, Wg), (Ho, Wo), split, act, add, enters, hands_on in kinds(a):
        B = a.B
        g = torch.randn((B, cg, Hg, Wg), device=dev, generator=gen)
        if mod is None:
            w = torch.randn((cg, cout, 3, 3), device=dev, generator=gen) / (4.0 * cg) ** 0.5
            f32, x3 = (G.GC_DG_S1, G.pack_adjoint_s1(w)), (G.GCX3_DG_S1, G.pack_adjoint_s1_x3(w))
        else:
            mod = mod.to(dev)
            f32, x3 = G.pack_adjoint(mod), G.pack_adjoint_x3(mod)
        ysave = torch.relu(torch.randn((B, cout, Ho, Wo), device=dev, generator=gen)) if act != G.ACT_NONE else None
        adds = [torch.randn((B, c, Ho, Wo), device=dev, generator=gen) if add else None for c in (split, cout - split)]
        outs = {m: [torch.empty((B, c, Ho, Wo), device=dev) if c else None for c in (split, cout - split)] for m in ("fp32", "bf16x3")}
        gs = G._MX3.empty(B, cg, Hg, Wg, dev)
        dxs = G._MX3.empty(B, cout, Ho, Wo, dev) if hands_on else None
        covered = bool(lib.nlspn_gconv_x3_dgrad_covers(x3[0], cg, cout, Hg, Wg, Ho, Wo))
        _lib.call("nlspn_gconv_x3_split", dev, g, gs, B, cg, Hg, Wg, _lib.STREAM)

        def run_f32():
            d0, d1 = outs["fp32"]
            _lib.call("nlspn_gconv_dgrad", dev, f32[0], g, cg, f32[1], ysave, adds[0], adds[1], d0, d1, split, B, Hg, Wg, cout,
                      Ho, Wo, act, 1.0, _lib.STREAM)

        def run_x3():
            d0, d1 = outs["bf16x3"]
            if enters:
                _lib.call("nlspn_gconv_x3_split", dev, g, gs, B, cg, Hg, Wg, _lib.STREAM)
            _lib.call("nlspn_gconv_x3_dgrad", dev, x3[0], gs, cg, x3[1], ysave, adds[0], adds[1], d0, d1, split, dxs, B, Hg, Wg,
                      cout, Ho, Wo, act, 1.0, _lib.STREAM)

        row = {"kind": name, "cg": cg, "cout": cout, "gradient": [Hg, Wg], "output": [Ho, Wo], "covered": covered,
               "split_launch_included": enters, "split_copy_written": hands_on, "flops": 2 * 9 * cg * cout * B * Ho * Wo
               if mod is None or isinstance(mod, nn.ConvTranspose2d) else 2 * 9 * cg * cout * B * Hg * Wg}
        if not covered:   # (the kind stays on the f32 entry: nothing to compare)
            out.append(row)
            print(f"{name:36s} not covered: nlspn_gconv_dgrad's", flush=True)
            continue
        run = {"fp32": run_f32, "bf16x3": run_x3}
        for call in run.values():
            for _ in range(3):
                call()
        torch.cuda.synchronize()
        ref = torch.cat([t for t in outs["fp32"] if t is not None], 1)
        got = torch.cat([t for t in outs["bf16x3"] if t is not None], 1)
        row["rel_l2_vs_fp32"] = float((got.double() - ref.double()).norm() / ref.double().norm())
        row.update(timed(run, a.rounds, a.calls))
        row["speedup"] = row["fp32"]["ms_mean"] / row["bf16x3"]["ms_mean"]
        # faster by more than the round-to-round range of either entry
        row["bf16x3_faster_beyond_range"] = row["fp32"]["ms_min"] > row["bf16x3"]["ms_max"]
        out.append(row)
        print(f"{name:36s} fp32 {row['fp32']['ms_mean']:.4f} ms [{row['fp32']['ms_min']:.4f} .. {row['fp32']['ms_max']:.4f}]  "
              f"bf16x3 {row['bf16x3']['ms_mean']:.4f} ms [{row['bf16x3']['ms_min']:.4f} .. {row['bf16x3']['ms_max']:.4f}]  "
              f"x{row['speedup']:.2f}  apart {row['bf16x3_faster_beyond_range']}", flush=True)
    return out


def bench_gate_splits(a, dev):
    half = lambda n: (n - 1) // 2 + 1  # noqa: E731
    H8, W8, hc, B = half(half(half(a.H))), half(half(half(a.W))), a.hidden, a.B
    duq, duzr = torch.randn((B, hc, H8, W8), device=dev), torch.randn((B, 2 * hc, H8, W8), device=dev)
    sq, szr = G._MX3.empty(B, hc, H8, W8, dev), G._MX3.empty(B, 2 * hc, H8, W8, dev)

    def both():
        _lib.call("nlspn_gconv_x3_split", dev, duq, sq, B, hc, H8, W8, _lib.STREAM)
        _lib.call("nlspn_gconv_x3_split", dev, duzr, szr, B, 2 * hc, H8, W8, _lib.STREAM)
    for _ in range(3):
        both()
    torch.cuda.synchronize()
    r = timed({"two_split_launches": both}, a.rounds, a.calls)["two_split_launches"]
    r["bytes"] = B * 3 * hc * H8 * W8 * 8  # 4 read + 4 written per element
    print(f"gate stages' two split launches {r['ms_mean']:.4f} ms [{r['ms_min']:.4f} .. {r['ms_max']:.4f}]", flush=True)
    return r


def bench_step(a, dev):
    m = build(a, dev)
    tuned = copy.deepcopy(m).gru_channels_last()
    g = torch.Generator(device=dev).manual_seed(1)
    pred_init = torch.rand((a.B, 1, a.H, a.W), device=dev, generator=g) * 10
    dep = pred_init * (torch.rand((a.B, 1, a.H, a.W), device=dev, generator=g) < 0.02)
    off_aff = torch.randn((a.B, 24, a.H, a.W), device=dev, generator=g)
    conf = torch.rand((a.B, 1, a.H, a.W), device=dev, generator=g)
    proj = torch.randn((a.B, 1, a.H, a.W), device=dev, generator=g)

    def step(model, native, bench, dgrad, wgrad="bf16x3", narrow=True):
        model.native_gru, model.native_gru_train = native, native
        model.gru_wgrad_precision, model.gru_wgrad_narrow, model.gru_dgrad_precision = wgrad, narrow, dgrad
        torch.backends.cudnn.benchmark = bench
        ins = [t.clone().requires_grad_(True) for t in (pred_init, off_aff, conf)]
        for p in model.parameters():
            p.grad = None
        o = model.propagate_heads(*ins, dep)
        (o["pred"] * proj).sum().backward()

    variants = {"native_dgrad_bf16x3": (m, True, False, "bf16x3"), "native_dgrad_fp32": (m, True, False, "fp32"),
                "modules": (m, False, False, "fp32"), "modules_tuned": (tuned, False, True, "fp32")}
    for v in variants.values():
        for _ in range(a.warmup):
            step(*v)
    torch.cuda.synchronize()
    res = timed({n: (lambda v=v: step(*v)) for n, v in variants.items()}, a.rounds, a.steps)
    stats, grads = {}, {}
    subs = ("encode_dep", "encode_aff", "GRU", "decode_aff")
    for name, v in (("native_dgrad_bf16x3", variants["native_dgrad_bf16x3"]), ("native_dgrad_fp32", variants["native_dgrad_fp32"]),
                    ("native_all_fp32", (m, True, False, "fp32", "fp32", False))):
        m._gru_convs.reset_stats()
        step(*v)
        stats[name] = dict(m._gru_convs.stats)
        grads[name] = {f"{s}.{n}": p.grad.detach().double().clone() for s in subs for n, p in getattr(m, s).named_parameters()}
    torch.cuda.synchronize()
    ref = grads["native_all_fp32"]
    acc = {name: {k: float((gr[k] - ref[k]).norm() / ref[k].norm()) for k in ref}
           for name, gr in grads.items() if name != "native_all_fp32"}
    for n, r in res.items():
        print(f"{n:20s} {r['ms_mean']:.3f} ms [{r['ms_min']:.3f} .. {r['ms_max']:.3f}]", flush=True)
    x3 = res["native_dgrad_bf16x3"]
    print("largest parameter-gradient rel L2 vs the all-fp32 native step:", {n: max(e.values()) for n, e in acc.items()}, flush=True)
    return {"workload": {"B": a.B, "H": a.H, "W": a.W, "T": a.T, "hidden": a.hidden,
                         "what": "propagate_heads forward + backward, GRU mode; native variants with "
                                 "gru_wgrad_precision = bf16x3 and gru_wgrad_narrow = True"},
            "steps_per_block": a.steps, "variants": res, "native_stats_per_step": stats,
            "param_grad_rel_l2_vs_all_fp32_native": acc,
            "dgrad_bf16x3_beats_dgrad_fp32_beyond_range": res["native_dgrad_fp32"]["ms_min"] > x3["ms_max"],
            "dgrad_bf16x3_beats_modules_tuned_beyond_range": res["modules_tuned"]["ms_min"] > x3["ms_max"]}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--H", type=int, default=228)
    ap.add_argument("--W", type=int, default=304)
    ap.add_argument("--T", type=int, default=18)
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=10, help="alternations of the variants")
    ap.add_argument("--calls", type=int, default=20, help="(a), (b): calls per timed block")
    ap.add_argument("--steps", type=int, default=2, help="(c): forward + backward passes per timed block")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--part", choices=["all", "calls", "step"], default="all")
    ap.add_argument("--all-kinds", action="store_true",
                    help="(a): the chain as it is when nlspn_gconv_x3_dgrad_covers accepts the 2hc -> 16 decoder layer's "
                         "adjoint too (the library of profiles/gru_dgrad_x3_bench_all_kinds.json): the hc -> 2hc "
                         "layer's adjoint then reads the split copy and needs no split launch")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gru_dgrad_x3_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gru_dgrad_bench: no GPU present (this tool measures the HIP kernels; there is no fallback)")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "library": _lib.LIB_PATH.replace(ROOT, ".")}
    if a.part in ("all", "calls"):
        res["calls"] = {"calls_per_block": a.calls, "rows": bench_calls(a, dev)}
        res["gate_stage_splits"] = bench_gate_splits(a, dev)
    if a.part in ("all", "step"):
        res["step"] = bench_step(a, dev)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
