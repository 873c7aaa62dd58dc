#!/usr/bin/env python
"""The split-bf16 weight gradient (nlspn_gconv_wgrad_bf16x3, csrc/nlspn_gwgrad16.h) against the
f32 kernel (nlspn_gconv_wgrad) of the same library, in one process, the variants alternating.

(a) Per layer: both entry points through the C ABI on the weight-gradient shapes of the
    training benchmark (NYU 228x304, B=8, hidden 128): 16->256 at 57x76, 256->128 at 29x38, the
    ConvGRU's [h, x] -> [z, r] and -> q at 29x38, and the transposed 128->256 and 256->16.  Every
    round times each entry once (device events around `--calls` calls: kernel, slab reduce and
    bias gradient); reported: mean, min, max and range of the per-round means, TF/s of the
    layer's 2 * 9 * Cs * Cl * B * Hs * Ws FLOPs, and the largest |bf16x3 - f32| / max |f32|.
(b) The whole training step of DESIGN.md 3.8.1 (propagate_heads forward + backward, T=18):
    native fp32, native bf16x3, modules (MIOpen defaults), modules_tuned (channels_last +
    algorithm search), as tools/gru_train_bench.py times them.

Writes JSON (default profiles/gru_wgrad_x3_bench.json).  No GPU: an error.
"""
import argparse
import copy
import json
import os
import statistics
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nlspn_eccv20_amd import NLSPNModel, _lib  # noqa: E402

ENTRIES = {"fp32": "nlspn_gconv_wgrad", "bf16x3": "nlspn_gconv_wgrad_bf16x3"}


def layers(a):
    half = lambda n: (n - 1) // 2 + 1  # noqa: E731
    H4, W4, H8, W8 = half(half(a.H)), half(half(a.W)), half(half(half(a.H))), half(half(half(a.W)))
    hc = a.hidden
    # name, stride, Cs, c0, c1, (Hs, Ws), (Hl, Wl), bias_from_large
    return [("conv 16->256 at 1/4", 2, 2 * hc, 16, 0, (H4, W4), (2 * H4, 2 * W4), False),
            ("conv 256->128 at 1/8", 2, hc, 2 * hc, 0, (H8, W8), (H4, W4), False),
            ("GRU [h,x]->[z,r]", 1, 2 * hc, hc, hc, (H8, W8), (H8, W8), False),
            ("GRU [rh,x]->q", 1, hc, hc, hc, (H8, W8), (H8, W8), False),
            ("convT 128->256 from 1/8", 2, hc, 2 * hc, 0, (H8, W8), (2 * H8, 2 * W8), True),
            ("convT 256->16 from 1/4", 2, 2 * hc, 16, 0, (2 * H8, 2 * W8), (4 * H8, 4 * W8), True)]


def summary(t):
    return {"ms_mean": statistics.mean(t), "ms_median": statistics.median(t), "ms_min": min(t), "ms_max": max(t),
            "range_ms": max(t) - min(t), "ms_rounds": t}


def bench_layers(a, dev):
    lib = _lib.get()
    g = torch.Generator(device=dev).manual_seed(2)
    out = []
    for name, S, Cs, c0, c1, (Hs, Ws), (Hl, Wl), bfl in layers(a):
        s = torch.randn((a.B, Cs, Hs, Ws), device=dev, generator=g)
        l0 = torch.relu(torch.randn((a.B, c0, Hl, Wl), device=dev, generator=g))
        l1 = torch.relu(torch.randn((a.B, c1, Hl, Wl), device=dev, generator=g)) if c1 else None
        run, dws = {}, {}
        for mode, entry in ENTRIES.items():
            need = getattr(lib, entry + "_workspace_bytes")(S, Cs, c0 + c1, a.B, Hs, Ws, Hl, Wl)
            ws = torch.empty((need + 3) // 4, device=dev)
            dw = torch.empty((Cs, c0 + c1, 3, 3), device=dev)
            db = torch.empty(c0 if bfl else Cs, device=dev)

            def call(entry=entry, ws=ws, dw=dw, db=db):
                _lib.call(entry, dev, S, s, Cs, l0, c0, l1, c1, dw, db, int(bfl), 1.0, ws, ws.numel() * 4, a.B, Hs, Ws,
                          Hl, Wl, _lib.STREAM)
            run[mode], dws[mode] = call, dw
            for _ in range(3):
                call()
        torch.cuda.synchronize()
        times = {m: [] for m in run}
        for _ in range(a.rounds):
            for mode, call in run.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.calls):
                    call()
                e1.record()
                e1.synchronize()
                times[mode].append(e0.elapsed_time(e1) / a.calls)
        flops = 2 * 9 * Cs * (c0 + c1) * a.B * Hs * Ws
        row = {"layer": name, "stride": S, "Cs": Cs, "Cl": c0 + c1, "small": [Hs, Ws], "large": [Hl, Wl], "flops": flops,
               "workspace_bytes": {m: getattr(lib, e + "_workspace_bytes")(S, Cs, c0 + c1, a.B, Hs, Ws, Hl, Wl)
                                   for m, e in ENTRIES.items()},
               "max_abs_diff_over_max_abs": float((dws["bf16x3"] - dws["fp32"]).abs().max() / dws["fp32"].abs().max())}
        for mode, t in times.items():
            row[mode] = summary(t)
            row[mode]["tflops"] = flops / (row[mode]["ms_mean"] * 1e-3) / 1e12
        row["speedup"] = row["fp32"]["ms_mean"] / row["bf16x3"]["ms_mean"]
        # faster by more than the round-to-round range of either entry
        row["bf16x3_faster_beyond_range"] = row["fp32"]["ms_min"] > row["bf16x3"]["ms_max"]
        out.append(row)
        print(f"{name:26s} fp32 {row['fp32']['ms_mean']:.4f} ms [{row['fp32']['range_ms']:.4f}]  bf16x3 "
              f"{row['bf16x3']['ms_mean']:.4f} ms [{row['bf16x3']['range_ms']:.4f}]  x{row['speedup']:.2f}", flush=True)
    return out


def build(a, dev):
    args = types.SimpleNamespace(prop_kernel=3, affinity="TGASS", affinity_gamma=0.5, prop_time=a.T,
                                 preserve_input=True, always_clip=False, conf_prop=True, offset=True,
                                 network="resnet34", from_scratch=True, zero_init_aff=False, use_GRU=True,
                                 use_S2D=False, GRU_hidden_dim=a.hidden, GRU_input_dim=a.hidden, lr=1e-3,
                                 max_depth=10.0, patch_height=a.H, patch_width=a.W, model_name="NLSPN")
    torch.manual_seed(0)
    m = NLSPNModel(args).to(dev).eval()
    with torch.no_grad():
        for mod in (m.encode_dep, m.encode_aff, m.GRU, m.decode_aff):
            for p in mod.parameters():
                p.add_(0.02 * torch.randn_like(p))
    return m


def bench_step(a, dev):
    m = build(a, dev)
    tuned = copy.deepcopy(m).gru_channels_last()
    g = torch.Generator(device=dev).manual_seed(1)
    pred_init = torch.rand((a.B, 1, a.H, a.W), device=dev, generator=g) * 10
    dep = pred_init * (torch.rand((a.B, 1, a.H, a.W), device=dev, generator=g) < 0.02)
    off_aff = torch.randn((a.B, 24, a.H, a.W), device=dev, generator=g)
    conf = torch.rand((a.B, 1, a.H, a.W), device=dev, generator=g)
    proj = torch.randn((a.B, 1, a.H, a.W), device=dev, generator=g)

    def step(model, native, bench, precision):
        model.native_gru, model.native_gru_train = native, native
        model.gru_wgrad_precision = precision
        torch.backends.cudnn.benchmark = bench
        ins = [t.clone().requires_grad_(True) for t in (pred_init, off_aff, conf)]
        for p in model.parameters():
            p.grad = None
        o = model.propagate_heads(*ins, dep)
        (o["pred"] * proj).sum().backward()

    variants = {"native_fp32": (m, True, False, "fp32"), "native_bf16x3": (m, True, False, "bf16x3"),
                "modules": (m, False, False, "fp32"), "modules_tuned": (tuned, False, True, "fp32")}
    for v in variants.values():
        for _ in range(a.warmup):
            step(*v)
    torch.cuda.synchronize()
    times = {n: [] for n in variants}
    for _ in range(a.rounds):
        for name, v in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                step(*v)
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) / a.steps)
    res = {n: summary(t) for n, t in times.items()}
    stats = {}
    for name in ("native_fp32", "native_bf16x3"):
        m._gru_convs.reset_stats()
        step(*variants[name])
        stats[name] = dict(m._gru_convs.stats)
    torch.cuda.synchronize()
    for n, r in res.items():
        print(f"{n:14s} {r['ms_mean']:.3f} ms [{r['range_ms']:.3f}]", flush=True)
    return {"workload": {"B": a.B, "H": a.H, "W": a.W, "T": a.T, "hidden": a.hidden,
                         "what": "propagate_heads forward + backward, GRU mode"},
            "steps_per_block": a.steps, "variants": res, "native_stats_per_step": stats,
            "bf16x3_beats_fp32_beyond_range": res["native_fp32"]["ms_min"] > res["native_bf16x3"]["ms_max"],
            "bf16x3_beats_modules_tuned_beyond_range": res["modules_tuned"]["ms_min"] > res["native_bf16x3"]["ms_max"]}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--H", type=int, default=228)
    ap.add_argument("--W", type=int, default=304)
    ap.add_argument("--T", type=int, default=18)
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=10, help="alternations of the variants")
    ap.add_argument("--calls", type=int, default=20, help="(a): calls per timed block")
    ap.add_argument("--steps", type=int, default=2, help="(b): forward + backward passes per timed block")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--part", choices=["all", "layers", "step"], default="all")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gru_wgrad_x3_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gru_wgrad_bench: no GPU present (this tool measures the HIP kernels; there is no fallback)")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "library": _lib.LIB_PATH.replace(ROOT, ".")}
    if a.part in ("all", "layers"):
        res["layers"] = {"calls_per_block": a.calls, "what": "kernel + slab reduce + bias gradient per call", "rows": bench_layers(a, dev)}
    if a.part in ("all", "step"):
        res["step"] = bench_step(a, dev)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
