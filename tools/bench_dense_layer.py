#!/usr/bin/env python
"""The dense-adjacency PNALayer (pna_amd.pytorch.pna.layer.PNALayer: the multitask GNN's convolution) on the one-call route
(autograd.DenseLayerFn: pna_dense_layer_fwd_f32 / _bwd_f32; knob PNA_AMD_DENSE_LAYER_ROWS covering B N) against the route it would replace
(knob 0: sparsify + two aggregate calls + posttrans per tower + the mixing Linear, and autograd's backward of each), in ONE process on one
box:

  * first_BxN: the multitask first layer (in 2 -> 16, 4 towers, Fi = 2, divide_input=False);
  * mid_BxN:   the mid layer (16 -> 16, 4 towers, Fi = 4, divide_input=True);
  * gnn_BxN:   the GNN's inner loop x = gru(x, conv(x, adj)) for N / 2 iterations from public pieces (PNALayer, layers.GRU), the first
               iteration through the first layer, with PNA_AMD_GRU_ROWS on for BOTH routes;
  at (B, N) = (16, 15), (64, 25), (16, 97); aggregators mean max min std, scalers identity amplification attenuation (BASELINE configs[0]).

Each piece is forward + backward (the input's and every parameter's gradient); every step is timed once (host clock around the step and a
device synchronisation); the two routes alternate step by step, so drift hits both; the outputs of the two routes are compared at the timed
size.  Launches per step come from a fresh child process of this tool's own under `rocprofv3 --kernel-trace --stats` (no counters in that
run), one pair of children per traced workload and route.

    python tools/bench_dense_layer.py            # writes profiles/dense_layer.json
"""
import argparse
import csv
import gc
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_small_train import timed  # noqa: E402
from pna_amd import functional as PF, layers  # noqa: E402
from pna_amd.pytorch.pna.layer import PNALayer  # noqa: E402

AGG, SCA = "mean max min std".split(), "identity amplification attenuation".split()
SHAPES = ((16, 15), (64, 25), (16, 97))
WORKLOADS = tuple(f"{kind}_{B}x{N}" for kind in ("first", "mid", "gnn") for B, N in SHAPES)
TRACED = ("mid_16x15", "mid_16x97", "gnn_16x15")
KNOB_ON = 1 << 30


def _graphs(B, N, gen):
    """Symmetric random graphs at ~4 neighbours per node over a ring (every node has an edge), as the benchmark's generators give."""
    up = torch.triu((torch.rand(B, N, N, generator=gen) < 4.0 / N).float(), 1)
    idx = torch.arange(N)
    up[:, idx, (idx + 1) % N] = 1.0
    adj = ((up + up.transpose(1, 2)) > 0).float()
    adj[:, idx, idx] = 0.0
    return adj


def setup(workload, dev):
    """-> (step function returning the output, B, N)."""
    kind, shape = workload.split("_")
    B, N = (int(v) for v in shape.split("x"))
    torch.manual_seed(0)
    gen = torch.Generator().manual_seed(1)
    adj = _graphs(B, N, gen).to(dev)
    deg = adj.sum(-1)
    avg_d = {"log": torch.log(deg + 1).mean(), "lin": deg.mean()}                     # 0-dim device scalars
    conv = dict(aggregators=AGG, scalers=SCA, avg_d=avg_d, towers=4, self_loop=False, pretrans_layers=1, posttrans_layers=1, device=dev)
    first = PNALayer(2, 16, divide_input=False, **conv).to(dev).train()
    mid = PNALayer(16, 16, divide_input=True, **conv).to(dev).train()
    for lay in (first, mid):                                                          # (the default gain 1 / in_size leaves the outputs tiny)
        for p in lay.parameters():
            if p.dim() == 2:
                torch.nn.init.xavier_uniform_(p)
    if kind in ("first", "mid"):
        lay = first if kind == "first" else mid
        x = torch.randn(B, N, 2 if kind == "first" else 16, device=dev).requires_grad_(True)
        R = torch.randn(B, N, 16, device=dev)

        def step():
            lay.zero_grad(set_to_none=True)
            x.grad = None
            out = lay(x, adj)
            (out * R).sum().backward()
            return out.detach()
        return step, B, N
    gru = layers.GRU(16, 16, dev)
    x0 = torch.randn(B, N, 2, device=dev).requires_grad_(True)
    R = torch.randn(B, N, 16, device=dev)
    PF.GRU_ROWS = KNOB_ON                                                             # the GRU's one-call route, for both layer routes

    def step():
        first.zero_grad(set_to_none=True)
        mid.zero_grad(set_to_none=True)
        gru.zero_grad(set_to_none=True)
        x0.grad = None
        x = x0
        for it in range(N // 2):                                                      # models/pytorch/gnn_framework.py:93-95
            x = gru(x, (first if it == 0 else mid)(x, adj))
        (x * R).sum().backward()
        return x.detach()
    return step, B, N


def measure(workload, dev, steps, warmup):
    step, B, N = setup(workload, dev)
    knobs = {"parent_route": 0, "one_call_route": KNOB_ON}
    times = {k: [] for k in knobs}
    outs = {}
    gc.disable()
    try:
        for i in range(warmup + steps):
            for name, knob in knobs.items():                    # the routes alternate step by step
                PF.DENSE_LAYER_ROWS = knob
                out = [None]
                t = timed(lambda: out.__setitem__(0, step()))
                outs[name] = out[0]
                if i >= warmup:
                    times[name].append(t)
    finally:
        gc.enable()
        PF.DENSE_LAYER_ROWS = 0
        PF.GRU_ROWS = 0
    ent = {"B": B, "N": N, "rows": B * N}
    for name, ts in times.items():
        ent[name] = {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "steps": len(ts)}
    ent["one_call_over_parent"] = ent["one_call_route"]["median_ms"] / ent["parent_route"]["median_ms"]
    ent["routes_max_abs_diff"] = float((outs["one_call_route"] - outs["parent_route"]).abs().max())
    ent["output_max_abs"] = float(outs["parent_route"].abs().max())
    return ent


def child(workload, knob, steps):
    dev = torch.device("cuda:0")
    step, _, _ = setup(workload, dev)
    PF.DENSE_LAYER_ROWS = KNOB_ON if knob else 0
    for _ in range(steps):
        step()
    torch.cuda.synchronize()


def _trace_rows(workload, knob, steps):
    d = tempfile.mkdtemp(prefix="dense_trace_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "dense", "--",
           sys.executable, os.path.abspath(__file__), "--child", workload, "--knob", str(knob), "--steps", str(steps)]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        files = glob.glob(os.path.join(d, "**", "dense_kernel_stats.csv"), recursive=True)
        if r.returncode != 0 or not files:
            raise RuntimeError(f"rocprofv3 rc={r.returncode}: {r.stderr[-400:]}")
        return {row["Name"]: (int(row["Calls"]), float(row["TotalDurationNs"])) for row in csv.DictReader(open(files[0]))}
    finally:
        shutil.rmtree(d, ignore_errors=True)


def trace(workload, knob, short=2, long=8):
    """Launches per step and the per-kernel split of the device time: the difference between the kernel statistics of a child that runs
    `long` steps and one that runs `short` (what the set-up launches cancels out of)."""
    if shutil.which("rocprofv3") is None:
        return {"error": "rocprofv3 not found"}
    try:
        a, b = _trace_rows(workload, knob, short), _trace_rows(workload, knob, long)
    except (RuntimeError, subprocess.TimeoutExpired) as ex:
        return {"error": str(ex)}
    n = long - short
    rows = [(k, (b[k][0] - a.get(k, (0, 0.0))[0]) / n, (b[k][1] - a.get(k, (0, 0.0))[1]) / n / 1e3) for k in b]
    rows = [r for r in rows if r[1] > 0]
    top = sorted(rows, key=lambda x: -x[2])[:8]
    return {"steps": n, "launches_per_step": sum(r[1] for r in rows), "kernel_us_per_step": sum(r[2] for r in rows),
            "top_kernels": [{"name": k[:80], "calls_per_step": c, "us_per_step": t} for k, c, t in top]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    ap.add_argument("--traced", default=",".join(TRACED))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_layer.json"))
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--child", default=None)
    ap.add_argument("--knob", type=int, default=0)
    args = ap.parse_args()
    if args.child:
        child(args.child, args.knob, args.steps)
        return
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(dev),
           "method": "one process; wall clock per step (forward + backward) with a device synchronisation, every step timed once, the routes "
                     f"alternating; {args.steps} steps after {args.warmup} warm-up steps; launches from rocprofv3 --kernel-trace --stats of a "
                     "child process (traced workloads only)",
           "workloads": {}}
    traced = set(args.traced.split(",")) if not args.no_trace else set()
    for w in args.workloads.split(","):
        ent = measure(w, dev, args.steps, args.warmup)
        if w in traced:
            ent["trace"] = {"parent_route": trace(w, 0), "one_call_route": trace(w, 1)}
            if any("error" in v for v in ent["trace"].values()):                       # a child that failed: start no further one
                traced = set()
        res["workloads"][w] = ent
        print(w, json.dumps({k: v for k, v in ent.items() if k != "trace"}), flush=True)
        if "trace" in ent:
            print(w, "launches per step:", {k: v.get("launches_per_step", v.get("error")) for k, v in ent["trace"].items()}, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
