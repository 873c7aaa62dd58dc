#!/usr/bin/env python
"""Training through the fused head epilogue (heads.head_epilogue(..., differentiable=True),
csrc/nlspn_heads_bwd.h) against the torch modules, and its weight-gradient entry against the
GRU-mode entries, on the same weights and inputs, in one process, the variants alternating.

Workloads: NYU 228x304 B=8 and KITTI 240x1216 B=4 (C = 64, nout = 24, both one-row heads).
 1. step: forward + backward of the heads given decoder outputs that require grad
        native              the HIP forward and backward
        modules             the three nn.Conv2d on torch.cat inputs, ReLU / sigmoid, MIOpen defaults
        modules_cl_search   the same in channels_last with MIOpen's algorithm search
 2. wgrad: nlspn_head_wgrad against nlspn_gconv_wgrad and nlspn_gconv_wgrad_bf16x3 (stride 1,
    s = gpre, l0 = fd_oa, l1 = fe1; each with its own bias gradient) on the same operands.  The
    new kernel counts as a gain if its mean is below the f32 entry's by more than the two ranges
    together.
 3. pieces: the backward's calls one by one (pre, dgrad, dgrad_single, wgrad; the reduce
    launches inside wgrad show in the kernel trace).
 4. memory: peak allocated bytes of one step above the inputs, native against modules.
A round times `--steps` calls of each variant in turn (device events).  Reported: the per-round
means, their mean and their range over the rounds.  Writes JSON under profiles/.  No GPU: an error.

A kernel trace comes from a separate run (no counters), never mixed with the timing run.  Each
GPU step under its own time limit, chained:
    timeout -k 10 400 python tools/head_train_bench.py && \\
    timeout -k 10 300 rocprofv3 --kernel-trace --stats -d DIR -o htb --output-format csv -- \\
        python tools/head_train_bench.py --workload nyu --rounds 1 --no-write
"""
import argparse
import copy
import json
import os
import statistics
import sys

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nlspn_eccv20_amd import _lib  # noqa: E402
from nlspn_eccv20_amd import heads as HD  # noqa: E402
from nlspn_eccv20_amd.gru import GC_DG_S1  # noqa: E402

WORKLOADS = {"nyu": (8, 228, 304), "kitti": (4, 240, 1216)}
NOUT = 24


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
    B, H, W = WORKLOADS[name]
    C = a.C
    torch.manual_seed(0)
    convs = [nn.Conv2d(2 * C, n, 3, padding=1).to(dev) for n in (NOUT, 1, 1)]
    convs_cl = [copy.deepcopy(c).to(memory_format=torch.channels_last) for c in convs]
    g = torch.Generator(device=dev).manual_seed(1)
    srcs = [torch.randn((B, C, H, W), device=dev, generator=g).requires_grad_(True) for _ in range(4)]
    ups = [torch.randn((B, n, H, W), device=dev, generator=g) for n in (1, NOUT, 1)]
    hw = HD.HeadWeights()
    fe1, fd_oa, fd_id, fd_cf = srcs

    def zero():
        for t in srcs:
            t.grad = None
        for c in convs + convs_cl:
            c.zero_grad(set_to_none=True)

    def native():
        zero()
        outs = HD.head_epilogue(fe1, fd_oa, convs[0], fd_id, convs[1], fd_cf, convs[2], weights=hw, differentiable=True)
        torch.autograd.backward(outs, ups)

    def modules(cs, cl=False):
        def f():
            zero()
            torch.backends.cudnn.benchmark = cl
            cat = lambda t: torch.cat((t, fe1), 1).contiguous(memory_format=torch.channels_last) if cl else torch.cat((t, fe1), 1)  # noqa: E731
            outs = (torch.relu(cs[1](cat(fd_id))), cs[0](cat(fd_oa)), torch.sigmoid(cs[2](cat(fd_cf))))
            torch.autograd.backward(outs, ups)
            torch.backends.cudnn.benchmark = False
        return f

    res = {"shape": {"B": B, "C": C, "H": H, "W": W, "nout": NOUT}}
    step = {"native": native, "modules": modules(convs), "modules_cl_search": modules(convs_cl, True)}
    res["step"] = _time_rounds(step, a.rounds, a.steps)

    # ---- the entries on the same operands
    with torch.no_grad():
        R = NOUT + 2
        gpre = torch.randn((B, R, H, W), device=dev, generator=g)
        pred, conf = torch.relu(ups[0]), torch.sigmoid(ups[2])
        lib = _lib.get()
        e = lambda *s: torch.empty(s, device=dev)  # noqa: E731
        dw_oa, db_oa, dw_id, db_id, dw_cf, db_cf = e(NOUT, 2 * C, 3, 3), e(NOUT), e(1, 2 * C, 3, 3), e(1), e(1, 2 * C, 3, 3), e(1)
        dw, db = e(R, 2 * C, 3, 3), e(R)
        need = {n: getattr(lib, n + "_workspace_bytes")(1, R, 2 * C, B, H, W, H, W) for n in ("nlspn_gconv_wgrad", "nlspn_gconv_wgrad_bf16x3")}
        need["nlspn_head_wgrad"] = lib.nlspn_head_wgrad_workspace_bytes(B, C, H, W, NOUT)
        ws = e((max(need.values()) + 3) // 4)
        S = [t.detach() for t in srcs]
        wadj = hw.adjoint(*convs)
        d = [torch.empty_like(S[0]) for _ in range(4)]

        def head_wgrad():
            _lib.call("nlspn_head_wgrad", dev, gpre, S[0], S[1], S[2], S[3], dw_oa, db_oa, dw_id, db_id, dw_cf, db_cf, ws,
                      ws.numel() * 4, B, C, H, W, NOUT, _lib.STREAM)

        def gconv_wgrad(entry):
            return lambda: _lib.call(entry, dev, 1, gpre, R, S[1], C, S[0], C, dw, db, 0, 1.0, ws, ws.numel() * 4, B, H, W, H, W,
                                     _lib.STREAM)

        wg = {"head_wgrad": head_wgrad, "gconv_wgrad": gconv_wgrad("nlspn_gconv_wgrad"),
              "gconv_wgrad_bf16x3": gconv_wgrad("nlspn_gconv_wgrad_bf16x3")}
        res["wgrad"] = _time_rounds(wg, a.rounds, a.steps)
        new, old = res["wgrad"]["head_wgrad"], res["wgrad"]["gconv_wgrad"]
        by, ranges = old["ms_mean"] - new["ms_mean"], old["spread_ms"] + new["spread_ms"]
        res["head_wgrad_vs_gconv_wgrad"] = {"faster_by_ms": by, "ranges_combined_ms": ranges, "gain": by > ranges}
        head_wgrad()
        gconv_wgrad("nlspn_gconv_wgrad")()
        res["dw_oa_max_abs_diff_vs_gconv_wgrad"] = float((dw_oa - dw[:NOUT]).abs().max())
        pieces = {
            "pre": lambda: _lib.call("nlspn_head_backward_pre", dev, ups[1], ups[0], ups[2], pred, conf, gpre, B, H, W, NOUT,
                                     _lib.STREAM),
            "dgrad": lambda: _lib.call("nlspn_gconv_dgrad", dev, GC_DG_S1, gpre, R, wadj, None, None, None, d[1], d[0], C, B, H, W,
                                       2 * C, H, W, 0, 1.0, _lib.STREAM),
            "dgrad_single": lambda: _lib.call("nlspn_head_dgrad_single", dev, gpre, convs[1].weight, convs[2].weight, d[2], d[3],
                                              B, C, H, W, NOUT, _lib.STREAM),
            "wgrad": head_wgrad,
        }
        res["pieces"] = _time_rounds(pieces, a.rounds, a.steps)
        del ws, d, dw, gpre

    # ---- peak allocated memory of one step above what is live before it
    res["peak_step_bytes"] = {}
    for n in ("native", "modules"):
        zero()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        step[n]()
        torch.cuda.synchronize()
        res["peak_step_bytes"][n] = torch.cuda.max_memory_allocated(dev) - base
    zero()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", choices=["all", *WORKLOADS], default="all")
    ap.add_argument("--C", type=int, default=64)
    ap.add_argument("--steps", type=int, default=5, help="calls per timed block")
    ap.add_argument("--rounds", type=int, default=10, help="alternations of the variants")
    ap.add_argument("--no-write", action="store_true", help="do not write --out (the profiler run)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "head_train_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("head_train_bench: no GPU present (this tool measures the HIP kernels; there is no fallback)")
    dev = torch.device("cuda:0")
    names = list(WORKLOADS) if a.workload == "all" else [a.workload]
    res = {"device": torch.cuda.get_device_name(0), "calls_per_block": a.steps, "rounds": a.rounds, "workloads": {}}
    for n in names:
        res["workloads"][n] = run_workload(a, n, dev)
        torch.cuda.empty_cache()
    res["launches"] = dict(HD.train_stats)
    if not a.no_write:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    short = lambda blk: {v: [round(x["ms_mean"], 4), round(x["spread_ms"], 4)] for v, x in blk.items()}  # noqa: E731
    print(json.dumps({n: {"step": short(w["step"]), "wgrad": short(w["wgrad"]), "pieces": short(w["pieces"]),
                          "head_wgrad_vs_gconv_wgrad": w["head_wgrad_vs_gconv_wgrad"], "peak_step_bytes": w["peak_step_bytes"],
                          "dw_oa_max_abs_diff_vs_gconv_wgrad": w["dw_oa_max_abs_diff_vs_gconv_wgrad"]}
                      for n, w in res["workloads"].items()}))


if __name__ == "__main__":
    main()
