#!/usr/bin/env python
"""The fused head epilogue on the bf16 matrix cores with split operands
(precision = "bf16x3", csrc/nlspn_heads_x3.h) against the f32 kernel and against torch.cat +
MIOpen, on the same weights and inputs, in the same process, the variants alternating.

Workloads: NYU 228x304 B=8 and KITTI 240x1216 B=4 (C = 64, 3x3 / K = 8 with offsets and the
confidence head, T = 18).  Variants:
    fp32              heads.head_epilogue (the f32 kernel: the yardstick)
    bf16x3            heads.head_epilogue(precision="bf16x3")
    torch_cat_miopen  the three nn.Conv2d on torch.cat inputs, ReLU / sigmoid (the reference's ops)
    fp32_section      head_epilogue_prologue + propagate_normalized (T iterations), f32 heads
    bf16x3_section    the same with precision="bf16x3"
A round times `--steps` calls of each variant in turn (device events).  Reported: the per-round
means, their mean and their range over the rounds; and `pred` RMSE / largest difference of the
bf16x3 section against the fp32 section.  bf16x3 counts as a gain at a workload if its mean is
below fp32's by more than the two ranges together.  Writes JSON under profiles/.  No GPU: an error.

A kernel trace comes from a separate run (no counters), never mixed with the timing run.  Each
GPU step under its own time limit, chained:
    timeout -k 10 300 python tools/head_x3_bench.py && \\
    timeout -k 10 300 rocprofv3 --kernel-trace --stats -d DIR -o hx3 --output-format csv -- \\
        python tools/head_x3_bench.py --workload nyu --rounds 1 --no-write
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nlspn_eccv20_amd import heads as HD  # noqa: E402
from nlspn_eccv20_amd import propagate_normalized  # noqa: E402

WORKLOADS = {"nyu": (8, 228, 304), "kitti": (4, 240, 1216)}


def run_workload(a, name, dev):
    B, H, W = WORKLOADS[name]
    C, T = a.C, a.T
    torch.manual_seed(0)
    oa = nn.Conv2d(2 * C, 24, 3, padding=1).to(dev)
    idc = nn.Conv2d(2 * C, 1, 3, padding=1).to(dev)
    cfc = nn.Conv2d(2 * C, 1, 3, padding=1).to(dev)
    with torch.no_grad():
        oa.weight.mul_(3.0)  # offsets of a few pixels, affinities of either sign
        idc.bias.add_(2.0)
    g = torch.Generator(device=dev).manual_seed(1)
    fe1, fd_oa, fd_id, fd_cf = (torch.rand((B, C, H, W), device=dev, generator=g) for _ in range(4))
    dep = torch.rand((B, 1, H, W), device=dev, generator=g) * 10
    dep = dep * (torch.rand((B, 1, H, W), device=dev, generator=g) < 0.05)
    gamma = torch.tensor([4.0], device=dev)
    hw = HD.HeadWeights()

    def epi(precision):
        return lambda: HD.head_epilogue(fe1, fd_oa, oa, fd_id, idc, fd_cf, cfc, weights=hw, precision=precision)

    def section(precision):
        def f():
            h = HD.head_epilogue_prologue(fe1, fd_oa, oa, fd_id, idc, dep, gamma, "TGASS", fd_cf, cfc, True, False,
                                          weights=hw, precision=precision)
            return propagate_normalized(h["p0"], dep, h["confidence"], h["aff"], h["offset"], T, (3, 3), True, False)
        return f

    def miopen():
        return (torch.relu(idc(torch.cat((fd_id, fe1), 1))), oa(torch.cat((fd_oa, fe1), 1)),
                torch.sigmoid(cfc(torch.cat((fd_cf, fe1), 1))))

    variants = {"fp32": epi("fp32"), "bf16x3": epi("bf16x3"), "torch_cat_miopen": miopen,
                "fp32_section": section("fp32"), "bf16x3_section": section("bf16x3")}
    times = {n: [] for n in variants}
    with torch.no_grad():
        for f in variants.values():  # warm-up: packs, MIOpen's choice, the resident plan
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for n, f in variants.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.steps):
                    f()
                e1.record()
                e1.synchronize()
                times[n].append(e0.elapsed_time(e1) / a.steps)
        ref = variants["fp32_section"]()["pred"].double()
        d = variants["bf16x3_section"]()["pred"].double() - ref
        p32, px3 = variants["fp32"](), variants["bf16x3"]()
        torch.cuda.synchronize()
    res = {"shape": {"B": B, "C": C, "H": H, "W": W, "nout": 24, "T": T}, "variants": {}}
    for n, t in times.items():
        res["variants"][n] = {"ms_mean": statistics.mean(t), "ms_median": statistics.median(t), "ms_min": min(t),
                              "ms_max": max(t), "spread_ms": max(t) - min(t), "ms_rounds": t}
    res["pred_bf16x3_vs_fp32_T%d" % T] = {"rmse": float(d.pow(2).mean().sqrt()), "max_abs": float(d.abs().max())}
    res["off_aff_bf16x3_vs_fp32_max_abs"] = float((px3[1] - p32[1]).abs().max())
    for pair in (("fp32", "bf16x3"), ("fp32_section", "bf16x3_section")):
        f, x = (res["variants"][k] for k in pair)
        by, ranges = f["ms_mean"] - x["ms_mean"], f["spread_ms"] + x["spread_ms"]
        res["%s_vs_%s" % (pair[1], pair[0])] = {"faster_by_ms": by, "ranges_combined_ms": ranges, "gain": by > ranges}
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", choices=["all", *WORKLOADS], default="all")
    ap.add_argument("--C", type=int, default=64)
    ap.add_argument("--T", type=int, default=18)
    ap.add_argument("--steps", type=int, default=20, help="calls per timed block")
    ap.add_argument("--rounds", type=int, default=10, help="alternations of the variants")
    ap.add_argument("--no-write", action="store_true", help="do not write --out (the profiler run)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "head_x3_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("head_x3_bench: no GPU present (this tool measures the HIP kernels; there is no fallback)")
    dev = torch.device("cuda:0")
    names = list(WORKLOADS) if a.workload == "all" else [a.workload]
    res = {"device": torch.cuda.get_device_name(0), "calls_per_block": a.steps, "rounds": a.rounds,
           "launches": None, "workloads": {}}
    for k in HD.stats:
        HD.stats[k] = 0
    for n in names:
        res["workloads"][n] = run_workload(a, n, dev)
    res["launches"] = dict(HD.stats)
    if not a.no_write:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps({n: {"ms_mean": {v: round(x["ms_mean"], 4) for v, x in w["variants"].items()},
                          "spread_ms": {v: round(x["spread_ms"], 4) for v, x in w["variants"].items()},
                          **{k: v for k, v in w.items() if k not in ("variants", "shape")}}
                      for n, w in res["workloads"].items()}))


if __name__ == "__main__":
    main()
