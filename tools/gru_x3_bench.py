#!/usr/bin/env python
"""The GRU-mode propagation section at inference (NLSPNModel.propagate_heads, graph-replayed
through SectionGraph) with the GRU convolutions on the bf16 matrix cores with split operands
(gru_precision = "bf16x3", csrc/nlspn_gconv_x3.h) against the f32 HIP path, the f16 matrix
cores and the tuned torch modules, on the same weights, in the same process, the variants
alternating.

Workload: NYU 228x304, B=8, T=18, hidden 128.  Variants:
    fp32            native_gru, gru_precision = "fp32" (the default path)
    bf16x3          native_gru, gru_precision = "bf16x3"
    fp16            native_gru, gru_precision = "fp16"
    modules_tuned   native_gru = False, gru_channels_last() + cudnn.benchmark (a second model
                    with the same weights)
Every variant is captured once into its own hipGraph; a round times `--steps` replays of each
variant in turn (device events).  Reported: the per-round means, their mean and their range
over the rounds, and `pred` RMSE / largest difference of each mode against the "fp32" section.
Writes JSON under profiles/.  No GPU: an error.

The per-kernel table of the bf16x3 run comes from a separate kernel-trace run (no counters),
never mixed with the timing run.  Each GPU step under its own time limit, chained:
    timeout -k 10 300 python tools/gru_x3_bench.py && \\
    timeout -k 10 300 rocprofv3 --kernel-trace --stats -d DIR -o x3 --output-format csv -- \\
        python tools/gru_x3_bench.py --variant bf16x3 --rounds 1 --no-write && \\
    python tools/gru_x3_bench.py --merge-trace DIR/.../x3_kernel_trace.csv
(--merge-trace measures nothing and needs no GPU: it folds that run's dispatches, grouped by
kernel, into the existing result file.)
"""
import argparse
import copy
import csv
import json
import os
import statistics
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nlspn_eccv20_amd import NLSPNModel, SectionGraph  # noqa: E402


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


def merge_trace(a):
    with open(a.out) as f:
        res = json.load(f)
    groups, total = {}, 0
    with open(a.merge_trace) as f:
        for r in csv.DictReader(f):
            d = int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
            total += d
            name = r["Kernel_Name"].replace("void nlspn::", "").replace("nlspn::", "").split("(")[0]
            groups.setdefault((name, int(r["Grid_Size_X"])), []).append(d)
    rows = [{"kernel": k, "grid_threads": g, "calls": len(d), "mean_us": statistics.mean(d) / 1e3, "total_ms": sum(d) / 1e6,
             "share": sum(d) / total} for (k, g), d in sorted(groups.items(), key=lambda kv: -sum(kv[1]))]
    res["kernel_trace_bf16x3"] = {"what": "one separate rocprofv3 --kernel-trace --stats run of --variant bf16x3 (warm-up, capture "
                                        "and replays together: shares, not section times); dispatches grouped by kernel and grid",
                                "total_ms": total / 1e6, "groups": rows[:a.top]}
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(f"merged {min(len(rows), a.top)} of {len(rows)} kernel groups into {a.out}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--H", type=int, default=228)
    ap.add_argument("--W", type=int, default=304)
    ap.add_argument("--T", type=int, default=18)
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--steps", type=int, default=10, help="graph replays per timed block")
    ap.add_argument("--rounds", type=int, default=10, help="alternations of the variants")
    ap.add_argument("--variant", choices=["all", "fp32", "bf16x3", "fp16", "modules_tuned"], default="all")
    ap.add_argument("--merge-trace", help="kernel trace CSV of a profiler run of --variant bf16x3: fold it into --out")
    ap.add_argument("--top", type=int, default=24, help="kernel groups kept by --merge-trace")
    ap.add_argument("--no-write", action="store_true", help="do not write --out (the profiler run)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gru_x3_bench.json"))
    a = ap.parse_args()
    if a.merge_trace:
        return merge_trace(a)
    if not torch.cuda.is_available():
        sys.exit("gru_x3_bench: no GPU present (this tool measures the HIP kernels; there is no fallback)")
    dev = torch.device("cuda:0")
    m32 = build(a, dev)
    m16, mx3 = copy.deepcopy(m32), copy.deepcopy(m32)
    m16.gru_precision, mx3.gru_precision = "fp16", "bf16x3"
    tuned = copy.deepcopy(m32).gru_channels_last()
    tuned.native_gru = False
    g = torch.Generator(device=dev).manual_seed(1)
    pred_init = torch.rand((a.B, 1, a.H, a.W), device=dev, generator=g) * 10
    dep = pred_init * (torch.rand((a.B, 1, a.H, a.W), device=dev, generator=g) < 0.02)
    off_aff = torch.randn((a.B, 24, a.H, a.W), device=dev, generator=g)
    conf = torch.rand((a.B, 1, a.H, a.W), device=dev, generator=g)

    models = {"fp32": m32, "bf16x3": mx3, "fp16": m16, "modules_tuned": tuned}
    if a.variant != "all":
        models = {a.variant: models[a.variant]}
    graphs, stats = {}, {}
    for name, model in models.items():
        torch.backends.cudnn.benchmark = name == "modules_tuned"
        model._gru_convs.reset_stats()
        graphs[name] = SectionGraph(model, pred_init, off_aff, conf, dep)   # (2 warm-up runs + the capture)
        stats[name] = {k: v // 3 for k, v in model._gru_convs.stats.items()}
        graphs[name].replay()
    torch.cuda.synchronize()
    times = {n: [] for n in graphs}
    for _ in range(a.rounds):
        for name, sg in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                sg.replay()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) / a.steps)
    res = {"workload": {"B": a.B, "H": a.H, "W": a.W, "T": a.T, "hidden": a.hidden,
                        "what": "propagate_heads at inference, GRU mode, one hipGraph replay per section"},
           "device": torch.cuda.get_device_name(0), "replays_per_block": a.steps, "rounds": a.rounds,
           "launches_per_section": stats, "variants": {}}
    for name, t in times.items():
        res["variants"][name] = {"ms_mean": statistics.mean(t), "ms_median": statistics.median(t), "ms_min": min(t),
                                 "ms_max": max(t), "spread_ms": max(t) - min(t), "ms_rounds": t}
    if "fp32" in graphs:
        ref = graphs["fp32"].replay()["pred"].double().clone()
        res["pred_vs_fp32"] = {}
        for name in graphs:
            if name != "fp32":
                d = graphs[name].replay()["pred"].double() - ref
                res["pred_vs_fp32"][name] = {"rmse": float(d.pow(2).mean().sqrt()), "max_abs": float(d.abs().max())}
        torch.cuda.synchronize()
    if "fp32" in times and "bf16x3" in times:
        f, x = res["variants"]["fp32"], res["variants"]["bf16x3"]
        res["bf16x3_faster_than_fp32_by_ms"] = f["ms_mean"] - x["ms_mean"]
        res["ranges_combined_ms"] = f["spread_ms"] + x["spread_ms"]
    if not a.no_write:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps({"variants": {n: {"ms_mean": round(x["ms_mean"], 3), "spread_ms": round(x["spread_ms"], 3)}
                                   for n, x in res["variants"].items()},
                      "launches_per_section": stats, "pred_vs_fp32": res.get("pred_vs_fp32")}))


if __name__ == "__main__":
    main()
