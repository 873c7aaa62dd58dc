#!/usr/bin/env python
"""The streaming weight gradient of the narrow layers (nlspn_gconv_wgrad_narrow,
csrc/nlspn_gwnarrow.h) against the f32 kernel (nlspn_gconv_wgrad) of the same library, in one
process, the variants alternating.

(a) Per layer: both entry points through the C ABI on the three narrow weight-gradient shapes
    of the training benchmark (NYU 228x304, B=8): encode_dep's first conv 1 -> 16 and
    encode_aff's 9 -> 16 (s = dY at 1/2, l = x), decode_aff's last transposed conv 16 -> 8 (s = x
    at 1/2, l = dY, bias gradient from the large side).  Every round times each entry once
    (device events around `--calls` calls: every launch of the call); reported: mean, min, max
    and range of the per-round means, GB/s on the compulsory bytes (both operands read once),
    the largest |narrow - f32| / max |f32| of dW and db, and whether the narrow entry's slowest
    round is below the f32 entry's fastest (the rule by which a shape stays covered).
(b) The whole training step of DESIGN.md 3.8.1 (propagate_heads forward + backward, T=18):
    native bf16x3, native bf16x3 with gru_wgrad_narrow, modules (MIOpen defaults), modules_tuned
    (channels_last + algorithm search), as tools/gru_wgrad_bench.py times them.

Writes JSON (default profiles/gru_wgrad_narrow_bench.json).  No GPU: an error.
"""
import argparse
import copy
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from nlspn_eccv20_amd import _lib  # noqa: E402
from gru_wgrad_bench import build, summary  # noqa: E402

ENTRIES = {"fp32": "nlspn_gconv_wgrad", "narrow": "nlspn_gconv_wgrad_narrow"}


def layers(a):
    half = lambda n: (n - 1) // 2 + 1  # noqa: E731
    H2, W2 = half(a.H), half(a.W)
    # name, Cs, Cl, (Hs, Ws), (Hl, Wl), bias_from_large
    return [("encode_dep conv 1->16", 16, 1, (H2, W2), (a.H, a.W), False),
            ("encode_aff conv 9->16", 16, 9, (H2, W2), (a.H, a.W), False),
            ("decode_aff convT 16->8", 16, 8, (H2, W2), (a.H, a.W), True)]


def bench_layers(a, dev):
    lib = _lib.get()
    g = torch.Generator(device=dev).manual_seed(2)
    out = []
    for name, Cs, Cl, (Hs, Ws), (Hl, Wl), bfl in layers(a):
        s = torch.randn((a.B, Cs, Hs, Ws), device=dev, generator=g)
        l0 = torch.randn((a.B, Cl, Hl, Wl), device=dev, generator=g)
        run, outs = {}, {}
        for mode, entry in ENTRIES.items():
            need = getattr(lib, entry + "_workspace_bytes")(2, Cs, Cl, a.B, Hs, Ws, Hl, Wl)
            ws = torch.empty((need + 3) // 4, device=dev)
            dw = torch.empty((Cs, Cl, 3, 3), device=dev)
            db = torch.empty(Cl if bfl else Cs, device=dev)

            def call(entry=entry, ws=ws, dw=dw, db=db):
                _lib.call(entry, dev, 2, s, Cs, l0, Cl, None, 0, dw, db, int(bfl), 1.0, ws, ws.numel() * 4, a.B, Hs, Ws,
                          Hl, Wl, _lib.STREAM)
            run[mode], outs[mode] = call, (dw, db)
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
        nbytes = 4 * a.B * (Cs * Hs * Ws + Cl * Hl * Wl)
        row = {"layer": name, "Cs": Cs, "Cl": Cl, "small": [Hs, Ws], "large": [Hl, Wl], "bias_from_large": bfl,
               "compulsory_bytes": nbytes, "covered": bool(lib.nlspn_gconv_wgrad_narrow_covers(2, Cs, Cl, 0)),
               "workspace_bytes": {m: getattr(lib, e + "_workspace_bytes")(2, Cs, Cl, a.B, Hs, Ws, Hl, Wl) for m, e in ENTRIES.items()},
               "dw_max_abs_diff_over_max_abs": float((outs["narrow"][0] - outs["fp32"][0]).abs().max() / outs["fp32"][0].abs().max()),
               "db_max_abs_diff_over_max_abs": float((outs["narrow"][1] - outs["fp32"][1]).abs().max() / outs["fp32"][1].abs().max())}
        for mode, t in times.items():
            row[mode] = summary(t)
            row[mode]["gbytes_per_s"] = nbytes / (row[mode]["ms_mean"] * 1e-3) / 1e9
        row["speedup"] = row["fp32"]["ms_mean"] / row["narrow"]["ms_mean"]
        # the rule of keeping: the narrow entry's slowest round below the f32 entry's fastest
        row["narrow_max_below_fp32_min"] = row["narrow"]["ms_max"] < row["fp32"]["ms_min"]
        out.append(row)
        print(f"{name:24s} fp32 {row['fp32']['ms_mean']:.4f} ms [{row['fp32']['ms_min']:.4f}, {row['fp32']['ms_max']:.4f}]  narrow "
              f"{row['narrow']['ms_mean']:.4f} ms [{row['narrow']['ms_min']:.4f}, {row['narrow']['ms_max']:.4f}]  x{row['speedup']:.2f}  "
              f"{row['narrow']['gbytes_per_s']:.0f} GB/s", flush=True)
    return out


def bench_step(a, dev):
    m = build(a, dev)
    tuned = copy.deepcopy(m).gru_channels_last()
    g = torch.Generator(device=dev).manual_seed(1)
    pred_init = torch.rand((a.B, 1, a.H, a.W), device=dev, generator=g) * 10
    dep = pred_init * (torch.rand((a.B, 1, a.H, a.W), device=dev, generator=g) < 0.02)
    off_aff = torch.randn((a.B, 24, a.H, a.W), device=dev, generator=g)
    conf = torch.rand((a.B, 1, a.H, a.W), device=dev, generator=g)
    proj = torch.randn((a.B, 1, a.H, a.W), device=dev, generator=g)

    def step(model, native, bench, precision, narrow):
        model.native_gru, model.native_gru_train = native, native
        model.gru_wgrad_precision = precision
        model.gru_wgrad_narrow = narrow
        torch.backends.cudnn.benchmark = bench
        ins = [t.clone().requires_grad_(True) for t in (pred_init, off_aff, conf)]
        for p in model.parameters():
            p.grad = None
        o = model.propagate_heads(*ins, dep)
        (o["pred"] * proj).sum().backward()

    variants = {"native_bf16x3": (m, True, False, "bf16x3", False), "native_bf16x3_narrow": (m, True, False, "bf16x3", True),
                "modules": (m, False, False, "fp32", False), "modules_tuned": (tuned, False, True, "fp32", False)}
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
    for name in ("native_bf16x3", "native_bf16x3_narrow"):
        m._gru_convs.reset_stats()
        step(*variants[name])
        stats[name] = dict(m._gru_convs.stats)
    torch.cuda.synchronize()
    for n, r in res.items():
        print(f"{n:22s} {r['ms_mean']:.3f} ms [{r['ms_min']:.3f}, {r['ms_max']:.3f}]", flush=True)
    return {"workload": {"B": a.B, "H": a.H, "W": a.W, "T": a.T, "hidden": a.hidden,
                         "what": "propagate_heads forward + backward, GRU mode"},
            "steps_per_block": a.steps, "variants": res, "native_stats_per_step": stats,
            "narrow_beats_bf16x3_beyond_range": res["native_bf16x3"]["ms_min"] > res["native_bf16x3_narrow"]["ms_max"],
            "narrow_beats_modules_tuned_beyond_range": res["modules_tuned"]["ms_min"] > res["native_bf16x3_narrow"]["ms_max"],
            "modules_tuned_beats_narrow_beyond_range": res["native_bf16x3_narrow"]["ms_min"] > res["modules_tuned"]["ms_max"]}


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gru_wgrad_narrow_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gru_wgrad_narrow_bench: no GPU present (this tool measures the HIP kernels; there is no fallback)")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "library": _lib.LIB_PATH.replace(ROOT, ".")}
    if a.part in ("all", "layers"):
        res["layers"] = {"calls_per_block": a.calls, "what": "every launch of a call (kernel, reduce, bias gradient)",
                         "rows": bench_layers(a, dev)}
    if a.part in ("all", "step"):
        res["step"] = bench_step(a, dev)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
