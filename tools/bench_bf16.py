#!/usr/bin/env python
"""Same-box timing of the fp32 and the bf16 PNASimpleLayer forward (inference) on the bench graph, and the kernel means of the
bf16 kernels (k_gather_bf16*, k_posttrans_bf16) from a separate rocprofv3 kernel-trace run.

    python tools/bench_bf16.py [--shapes C3,C5] [--steps 20] [--warmup 5] [--out profiles/bf16_layer.json] [--no-trace]

Shapes (pna_amd/synth.py::powerlaw_graph, seed 1234): C3 = V 1 M, E 10 M, F 75; C5 = V 2 M, E 20 M, F 128; out_dim = F, the four
standard aggregators, three scalers, BatchNorm, residual.  Features are stored at a pitch of round8(F) elements for both dtypes
(the layout the bench line uses).  Method: HIP events around `steps` forwards after `warmup` ones, gc disabled
around the timed steps.  The kernel means come from a child process run under `rocprofv3 --kernel-trace --stats` (no counters in
the same run).  Bytes moved are ALGORITHMIC (what each kernel must read and write at least); the roofline fraction is against
8 TB/s of HBM.
"""
import argparse
import copy
import csv
import gc
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12
SHAPES = {"C3": (1_000_000, 10_000_000, 75), "C5": (2_000_000, 20_000_000, 128)}
AGGS, SCALERS = "mean max min std", "identity amplification attenuation"


def setup(shape, dev):
    from pna_amd.dgl.pna_layer import PNASimpleLayer
    from pna_amd.graph import Graph
    from pna_amd.synth import powerlaw_graph
    V, E, F = SHAPES[shape]
    src, dst = powerlaw_graph(V, E, seed=1234, device=dev)
    g = Graph(src, dst, V)
    avg_log = torch.log(g.in_degrees().double() + 1).mean().float()
    torch.manual_seed(0)
    layer = PNASimpleLayer(F, F, AGGS, SCALERS, {"log": avg_log}, 0.0, True, True).to(dev).eval()
    P = (F + 7) // 8 * 8
    h32 = torch.zeros(V, P, device=dev)[:, :F]
    h32.copy_(torch.randn(V, F, device=dev))
    h16 = torch.zeros(V, P, device=dev, dtype=torch.bfloat16)[:, :F]
    h16.copy_(h32)
    return g, layer, copy.deepcopy(layer).to(torch.bfloat16), h32, h16


def time_forward(layer, g, h, steps, warmup):
    with torch.no_grad():
        for _ in range(warmup):
            layer(g, h)
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        gc.disable()
        try:
            t0.record()
            for _ in range(steps):
                layer(g, h)
            t1.record()
            torch.cuda.synchronize()
        finally:
            gc.enable()
    return t0.elapsed_time(t1) / steps


def algorithmic_bytes(shape):
    """(gather bytes, contraction bytes) each bf16 kernel must move at least: CSR + 16-byte row pieces of every gathered row + the
    bf16 aggregate written; the aggregate read + the scalers + the residual read + the output written (the weight stays in cache)."""
    V, E, F = SHAPES[shape]
    Fb = (F + 7) // 8 * 8
    A, S = len(AGGS.split()), len(SCALERS.split())
    agg = V * A * Fb * 2
    gather = 4 * (V + 1) + 4 * E + E * Fb * 2 + agg
    post = agg + V * 4 * (S - 1) + 2 * V * F * 2
    return gather, post


def child(shape, steps):
    dev = torch.device("cuda:0")
    g, _, layer16, _, h16 = setup(shape, dev)
    time_forward(layer16, g, h16, steps, 2)


def trace(shape, steps):
    """Kernel means (us) of the bf16 kernels from a rocprofv3 kernel trace of a child process."""
    if shutil.which("rocprofv3") is None:
        return {"error": "rocprofv3 not found"}
    d = tempfile.mkdtemp(prefix="bf16_trace_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "bf16", "--",
           sys.executable, os.path.abspath(__file__), "--child", shape, "--steps", str(steps)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    files = glob.glob(os.path.join(d, "**", "bf16_kernel_stats.csv"), recursive=True)
    if r.returncode != 0 or not files:
        return {"error": f"rocprofv3 rc={r.returncode}", "tail": r.stderr[-400:]}
    out = {}
    for row in csv.DictReader(open(files[0])):
        name = row.get("Name", "")
        for key in ("k_gather_bf16_seg", "k_gather_bf16_fin", "k_gather_bf16", "k_posttrans_bf16"):
            if key in name:
                ent = out.setdefault(key, {"calls": 0, "total_ns": 0.0})
                ent["calls"] += int(row["Calls"])
                ent["total_ns"] += float(row["TotalDurationNs"])
                break
    shutil.rmtree(d, ignore_errors=True)
    return {k: {"calls": v["calls"], "mean_us": v["total_ns"] / v["calls"] / 1e3} for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="C3,C5")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bf16_layer.json"))
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    if args.child:
        child(args.child, args.steps)
        return
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(dev), "method": "HIP events, warm-up, gc disabled; kernel means from rocprofv3 --kernel-trace --stats",
           "hbm_peak_Bps": HBM_PEAK, "shapes": {}}
    for shape in args.shapes.split(","):
        g, l32, l16, h32, h16 = setup(shape, dev)
        ms32 = time_forward(l32, g, h32, args.steps, args.warmup)
        ms16 = time_forward(l16, g, h16, args.steps, args.warmup)
        gb, pb = algorithmic_bytes(shape)
        ent = {"V_E_F": SHAPES[shape], "fp32_ms_per_step": ms32, "bf16_ms_per_step": ms16, "bf16_over_fp32": ms16 / ms32,
               "bytes": {"k_gather_bf16": gb, "k_posttrans_bf16": pb}}
        del g, l32, l16, h32, h16
        torch.cuda.empty_cache()
        if not args.no_trace:
            k = trace(shape, args.steps)
            ent["kernels"] = k
            if "k_gather_bf16" in k:
                seg_us = sum(k[n]["mean_us"] for n in ("k_gather_bf16", "k_gather_bf16_seg", "k_gather_bf16_fin") if n in k)
                ent["roofline_fraction"] = {"k_gather_bf16 (+ heavy segments)": gb / (seg_us * 1e-6) / HBM_PEAK}
                if "k_posttrans_bf16" in k:
                    ent["roofline_fraction"]["k_posttrans_bf16"] = pb / (k["k_posttrans_bf16"]["mean_us"] * 1e-6) / HBM_PEAK
        res["shapes"][shape] = ent
        print(json.dumps({shape: ent}), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
