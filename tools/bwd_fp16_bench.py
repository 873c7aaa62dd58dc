#!/usr/bin/env python
"""Forward + backward of the propagation section (propagate() under autograd) in float32 and
in float16 storage, on the same values, in one process, the two alternating.

Workloads (synthetic inputs of synth(), gradients on pred and every pred_inter):
    c2       NYU 228x304, B = 8, 3x3 (K = 8), T = 18: the resident two-pass backward
    c3       KITTI 240x1216, B = 4, 3x3, T = 18: the two-pass step launches
    c5geom   BASELINE.md C5's geometry, 228x304, B = 16, 1x17 (K = 16), T = 36: the one-pass
             form (float16 is C5's storage; float32 there for comparison only)
Variants per workload: step_f32 / step_f16 (forward + backward), fwd_f32 / fwd_f16 (the forward
alone under no_grad, so the backward's share can be read off).  A round times `--steps` calls of
each variant in turn (device events).  Reported: the per-round means, their mean and their range
over the rounds, and the peak allocated bytes of one step above what is live before it.
Writes JSON under profiles/.  No GPU: an error.

One GPU step under its own time limit:
    timeout -k 10 400 python tools/bwd_fp16_bench.py
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nlspn_eccv20_amd import propagate  # noqa: E402
from nlspn_eccv20_amd.synthetic import synth  # noqa: E402

# name -> (B, H, W, kh, kw, T)
WORKLOADS = {"c2": (8, 228, 304, 3, 3, 18), "c3": (4, 240, 1216, 3, 3, 18), "c5geom": (16, 228, 304, 1, 17, 36)}
DTYPES = {"f32": torch.float32, "f16": torch.float16}


def _time_rounds(variants, rounds, steps, warm=2):
    for f in variants.values():
        for _ in range(warm):
            f()
    torch.cuda.synchronize()
    times = {n: [] for n in variants}
    for _ in range(rounds):
        for n, f in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                f()
            e1.record()
            e1.synchronize()
            times[n].append(e0.elapsed_time(e1) / steps)
    return {n: {"ms_mean": statistics.mean(t), "ms_median": statistics.median(t), "ms_min": min(t), "ms_max": max(t),
                "spread_ms": max(t) - min(t), "ms_rounds": t} for n, t in times.items()}


def run_workload(a, name, dev):
    B, H, W, kh, kw, T = WORKLOADS[name]
    K = kh * kw - 1
    s = synth(B, H, W, K, seed=1)
    rng = np.random.default_rng(2)
    up = {"gp": rng.standard_normal((B, 1, H, W)).astype(np.float32),
          "gi": rng.standard_normal((T, B, 1, H, W)).astype(np.float32)}
    gamma = torch.tensor([0.5 * K], device=dev, requires_grad=True)
    variants, steps_of = {}, {}
    for tag, dt in DTYPES.items():
        t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev).to(dt)  # noqa: E731
        oa = t(s["off_aff"]).requires_grad_(True)
        pi, cf, dep = t(s["pred_init"]).requires_grad_(True), t(s["conf"]).requires_grad_(True), t(s["dep"])
        gp, gi = t(up["gp"]), t(up["gi"])
        leaves = [oa, pi, cf, gamma]

        def forward(oa=oa, pi=pi, cf=cf, dep=dep):
            return propagate(pi, dep, cf, oa[:, 2 * K:], oa[:, :2 * K], gamma, prop_time=T, affinity="TGASS",
                             kernel=(kh, kw))

        def step(forward=forward, leaves=leaves, gp=gp, gi=gi):
            for x in leaves:
                x.grad = None
            o = forward()
            torch.autograd.backward((o["pred"], o["pred_inter_tensor"]), (gp, gi))

        def fwd(forward=forward):
            with torch.no_grad():
                forward()

        variants["step_" + tag], variants["fwd_" + tag] = step, fwd
        steps_of[tag] = (step, leaves)
    res = {"shape": {"B": B, "H": H, "W": W, "kh": kh, "kw": kw, "T": T}}
    res["time"] = _time_rounds(variants, a.rounds, a.steps)
    tm = res["time"]
    res["backward_ms"] = {tag: tm["step_" + tag]["ms_mean"] - tm["fwd_" + tag]["ms_mean"] for tag in DTYPES}
    by = tm["step_f32"]["ms_mean"] - tm["step_f16"]["ms_mean"]
    ranges = tm["step_f32"]["spread_ms"] + tm["step_f16"]["spread_ms"]
    res["f16_vs_f32_step"] = {"faster_by_ms": by, "ranges_combined_ms": ranges, "gain": by > ranges, "slower": -by > ranges}
    res["peak_step_bytes"] = {}
    for tag, (step, leaves) in steps_of.items():
        for x in leaves:
            x.grad = None
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        step()
        torch.cuda.synchronize()
        res["peak_step_bytes"][tag] = torch.cuda.max_memory_allocated(dev) - base
        for x in leaves:
            x.grad = None
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", choices=["all", *WORKLOADS], default="all")
    ap.add_argument("--steps", type=int, default=5, help="calls per timed block")
    ap.add_argument("--rounds", type=int, default=10, help="alternations of the variants")
    ap.add_argument("--no-write", action="store_true", help="do not write --out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bwd_fp16_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bwd_fp16_bench: no GPU present (this tool measures the HIP kernels; there is no fallback)")
    dev = torch.device("cuda:0")
    names = list(WORKLOADS) if a.workload == "all" else [a.workload]
    res = {"device": torch.cuda.get_device_name(0), "calls_per_block": a.steps, "rounds": a.rounds, "workloads": {}}
    for n in names:
        res["workloads"][n] = run_workload(a, n, dev)
        torch.cuda.empty_cache()
    if not a.no_write:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    short = lambda blk: {v: [round(x["ms_mean"], 4), round(x["spread_ms"], 4)] for v, x in blk.items()}  # noqa: E731
    print(json.dumps({n: {"time": short(w["time"]), "backward_ms": w["backward_ms"], "f16_vs_f32_step": w["f16_vs_f32_step"],
                          "peak_step_bytes": w["peak_step_bytes"]} for n, w in res["workloads"].items()}))


if __name__ == "__main__":
    main()
