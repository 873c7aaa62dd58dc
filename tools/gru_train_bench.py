#!/usr/bin/env python
"""Forward + backward of the GRU-mode propagation section (NLSPNModel.propagate_heads under
gradients): the native HIP path (gru.py, csrc/nlspn_gconv_bwd.h) against the torch-module
path, on the same model, in the same process, the variants alternating.

Workload: NYU 228x304, B=8, T=18, hidden 128.  Variants:
    native          native_gru_train = True
    modules         native_gru = False, MIOpen defaults
    modules_tuned   native_gru = False, gru_channels_last() + cudnn.benchmark (a second
                    model with the same weights)
Every round times each variant once (device events around `--steps` forward + backward
passes, at least `--min-seconds` of work per variant over all rounds); the spread is the
run-to-run range of the per-round means.  Writes JSON under profiles/.  No GPU: an error.

Per-layer weight / data gradient kernel times come from a separate kernel-trace run
(rocprofv3 --kernel-trace --stats) of this tool with --variant native --rounds 1:
`--merge-trace TRACE.csv --out BENCH.json` (no measuring, no GPU needed) folds that run's
dispatches, grouped by kernel and grid, into an existing result file, the weight-gradient
groups labelled with their layers and TF/s against the 157.3 TF/s f32-MFMA peak.
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
from nlspn_eccv20_amd import NLSPNModel  # noqa: E402

PEAK_TFLOPS = 157.3


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


def wgrad_layers(a):
    """{grid threads: (layers, FLOPs per call)} of the weight-gradient launches (the planner of
    nlspn_gwgrad_plan.h gw_plan: tiling by channel counts, K slices for ~512 workgroups)."""
    half = lambda n: (n - 1) // 2 + 1  # noqa: E731
    H2, W2, H4, W4, H8, W8 = half(a.H), half(a.W), half(half(a.H)), half(half(a.W)), (a.H + 7) // 8, (a.W + 7) // 8
    hc, K = a.hidden, 8
    layers = [("encode_dep.0", 2, 16, 1, H2, W2), ("encode_aff.0", 2, 16, K + 1, H2, W2),
              ("encode_dep.1 / encode_aff.1", 2, 2 * hc, 16, H4, W4), ("encode_dep.2 / encode_aff.2 / decode_aff.0", 2, hc, 2 * hc, H8, W8),
              ("GRU convz+convr", 1, 2 * hc, 2 * hc, H8, W8), ("GRU convq", 1, hc, 2 * hc, H8, W8),
              ("decode_aff.1", 2, 2 * hc, 16, 2 * H8, 2 * W8), ("decode_aff.2", 2, 16, K, 4 * H8, 4 * W8)]
    out = {}
    for name, S, Cs, Cl, Hs, Ws in layers:
        mt, nt, nthr = (64, 32, 256) if S == 1 or Cl > 16 else (128, 16, 256) if Cs > 16 else (16, 16, 64)
        tiles = -(-Cs // mt) * -(-Cl // nt)
        units = a.B * Hs * -(-Ws // 64)
        nsl = max(1, min(units, -(-512 // tiles)))
        nsl = -(-units // -(-units // nsl))
        grid = tiles * nsl * nthr
        prev = out.get((S, mt, grid))
        out[(S, mt, grid)] = (name if prev is None else prev[0] + " / " + name, 2 * 9 * Cs * Cl * a.B * Hs * Ws)
    return out


def merge_trace(a):
    with open(a.out) as f:
        res = json.load(f)
    groups = {}
    with open(a.merge_trace) as f:
        for r in csv.DictReader(f):
            name = r["Kernel_Name"]
            if not any(k in name for k in ("gwgrad", "gbias", "ggates", "gconv_kernel", "gsmall")):
                continue
            key = (name, int(r["Grid_Size_X"]), int(r["Workgroup_Size_X"]))
            groups.setdefault(key, []).append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    wl = wgrad_layers(a)
    rows = []
    for (name, grid, block), d in sorted(groups.items(), key=lambda kv: -sum(kv[1])):
        row = {"kernel": name.replace("void nlspn::", "").replace("nlspn::", "").split("(")[0], "grid_threads": grid,
               "block": block, "calls": len(d), "mean_us": statistics.mean(d) / 1e3, "total_ms": sum(d) / 1e6}
        if "gwgrad_kernel<" in name:
            S, mt = int(name.split("<")[1].split(",")[0]), {(2, 2): 64, (2, 4): 128, (1, 1): 16}[
                tuple(int(v) for v in name.split("<")[1].split(">")[0].split(",")[1:3])]
            hit = wl.get((S, mt, grid))
            if hit:
                row["layers"], row["flops"] = hit
                row["tflops"] = hit[1] / (row["mean_us"] * 1e-6) / 1e12
                row["of_peak"] = row["tflops"] / PEAK_TFLOPS
        rows.append(row)
    res["kernel_trace"] = {"what": "one separate rocprofv3 --kernel-trace --stats run of --variant native (its warm-up, "
                                   "timed and counting steps together); dispatches grouped by kernel and grid",
                           "peak_tflops_f32_mfma": PEAK_TFLOPS, "groups": rows}
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(f"merged {len(rows)} kernel groups into {a.out}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--H", type=int, default=228)
    ap.add_argument("--W", type=int, default=304)
    ap.add_argument("--T", type=int, default=18)
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--steps", type=int, default=3, help="forward + backward passes per timed block")
    ap.add_argument("--rounds", type=int, default=5, help="alternations of the variants (at least)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--min-seconds", type=float, default=1.0, help="timed work per variant at least")
    ap.add_argument("--variant", choices=["all", "native", "modules", "modules_tuned"], default="all")
    ap.add_argument("--merge-trace", help="kernel trace CSV of a profiler run of --variant native: fold it into --out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gru_train_bench.json"))
    a = ap.parse_args()
    if a.merge_trace:
        return merge_trace(a)
    if not torch.cuda.is_available():
        sys.exit("gru_train_bench: no GPU present (this tool measures the HIP kernels; there is no fallback)")
    dev = torch.device("cuda:0")
    m = build(a, dev)
    tuned = copy.deepcopy(m).gru_channels_last()
    g = torch.Generator(device=dev).manual_seed(1)
    pred_init = torch.rand((a.B, 1, a.H, a.W), device=dev, generator=g) * 10
    dep = pred_init * (torch.rand((a.B, 1, a.H, a.W), device=dev, generator=g) < 0.02)
    off_aff = torch.randn((a.B, 24, a.H, a.W), device=dev, generator=g)
    conf = torch.rand((a.B, 1, a.H, a.W), device=dev, generator=g)
    proj = torch.randn((a.B, 1, a.H, a.W), device=dev, generator=g)

    def step(model, native, bench):
        model.native_gru, model.native_gru_train = native, native
        torch.backends.cudnn.benchmark = bench
        ins = [t.clone().requires_grad_(True) for t in (pred_init, off_aff, conf)]
        for p in model.parameters():
            p.grad = None
        o = model.propagate_heads(*ins, dep)
        (o["pred"] * proj).sum().backward()

    variants = {"native": (m, True, False), "modules": (m, False, False), "modules_tuned": (tuned, False, True)}
    if a.variant != "all":
        variants = {a.variant: variants[a.variant]}
    for name, v in variants.items():
        for _ in range(a.warmup):
            step(*v)
    torch.cuda.synchronize()
    times = {n: [] for n in variants}
    rounds = 0
    while rounds < a.rounds or any(sum(t) * a.steps < a.min_seconds * 1e3 for t in times.values()):
        for name, v in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                step(*v)
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) / a.steps)
        rounds += 1
    res = {"workload": {"B": a.B, "H": a.H, "W": a.W, "T": a.T, "hidden": a.hidden,
                        "what": "propagate_heads forward + backward, GRU mode"},
           "device": torch.cuda.get_device_name(0), "steps_per_block": a.steps, "rounds": rounds,
           "native_stats_per_step": None, "variants": {}}
    for name, t in times.items():
        res["variants"][name] = {"ms_mean": statistics.mean(t), "ms_median": statistics.median(t), "ms_min": min(t),
                                 "ms_max": max(t), "spread_ms": max(t) - min(t), "ms_rounds": t}
    if "native" in variants:
        m._gru_convs.reset_stats()
        step(*variants["native"])
        res["native_stats_per_step"] = dict(m._gru_convs.stats)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: (v if k != "variants" else {n: {"ms_mean": round(x["ms_mean"], 3),
                                                          "spread_ms": round(x["spread_ms"], 3)}
                                                      for n, x in v.items()}) for k, v in res.items()
                      if k in ("variants", "native_stats_per_step", "rounds")}))


if __name__ == "__main__":
    main()
