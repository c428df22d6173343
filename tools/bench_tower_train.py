#!/usr/bin/env python
"""PNALayer training on ZINC-shaped molecule batches: the one-call route (autograd.TowerLayerSmallTrainFn, pna_tower_train_fwd_f32 /
_bwd_f32; knob PNA_AMD_SMALL_TOWER_TRAIN_ROWS = V) against the generic route it would replace (knob 0: torch.stack of the weights, the
projection GEMMs, AggregateFn, per tower PosttransFn / graph norm / BatchNorm, cat / Linear / LeakyReLU), in ONE process on one box:

  * a ZINC first layer (75 -> 75, 5 towers over the whole input, residual) and a ZINC last layer (75 -> 70, 5 towers over slices, no
    residual), forward + backward, on a synthetic 128-molecule batch (~3 k nodes / ~6.4 k edges) and on a 2 048-molecule batch;
  * a whole ZINC `pna_amd.nets.PNANet` training step (L = 4, hidden 75, out 70, 5 towers, edge_feat False, Adam:
    realworld_benchmark/README.md:61) on both batches.

Every step is timed once (host clock around the step and a device synchronisation: the layer is host- and launch-bound, so wall time per
step IS the figure); the two routes alternate step by step, so drift hits both.  20 steps after 5 warm-up steps; median, min and max are
kept.  Launches per step and the per-kernel split of both routes come from a child process run under `rocprofv3 --kernel-trace --stats`
(no counters in that run), one child per route and workload.

    python tools/bench_tower_train.py            # writes profiles/tower_train.json
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
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pna_amd import Graph, functional as PF  # noqa: E402
from pna_amd.dgl.pna_layer import PNALayer  # noqa: E402
from pna_amd.synth import molecule_batch  # noqa: E402

AGG, SCA = "mean max min std", "identity amplification attenuation"
WORKLOADS = ("first_128", "last_128", "net_128", "first_2048", "last_2048", "net_2048")


def setup(workload, dev):
    """-> (step function, V, E, graphs)."""
    kind, graphs = workload.split("_")
    graphs = int(graphs)
    src, dst, sizes = molecule_batch(graphs, seed=41)
    V, E = sum(sizes), src.numel()
    g = Graph(src, dst, V, sizes).to(dev)
    avg = {"log": torch.log(g.in_degrees().double() + 1).mean().float().cpu()}
    snorm = torch.cat([torch.full((n, 1), n ** -0.5) for n in sizes]).to(dev)
    torch.manual_seed(0)
    if kind in ("first", "last"):
        out_dim, div = (75, False) if kind == "first" else (70, True)
        layer = PNALayer(75, out_dim, AGG, SCA, avg, 0.0, True, True, towers=5, pretrans_layers=1, posttrans_layers=1, divide_input=div,
                         residual=True, edge_features=False).to(dev).train()
        h = torch.randn(V, 75, device=dev).requires_grad_(True)
        R = torch.randn(V, out_dim, device=dev)

        def step():
            h.grad = None
            layer.zero_grad(set_to_none=True)
            (layer(g, h, None, snorm) * R).sum().backward()
    else:
        from pna_amd.nets import PNANet
        net = PNANet(dict(hidden_dim=75, out_dim=70, L=4, readout="sum", edge_feat=False, gru=False, in_feat_dropout=0.0, dropout=0.0,
                          graph_norm=True, batch_norm=True, residual=True, aggregators=AGG, scalers=SCA, avg_d=avg, towers=5, edge_dim=0,
                          pretrans_layers=1, posttrans_layers=1, divide_input_first=False, divide_input_last=True, num_atom_type=28,
                          num_bond_type=4, device=dev)).to(dev).train()
        gen = torch.Generator().manual_seed(0)
        atoms = torch.randint(0, 28, (V,), generator=gen).to(dev)
        targets = torch.randn(len(sizes), 1, generator=gen).to(dev)
        opt = torch.optim.Adam(net.parameters(), lr=1e-3)

        def step():
            opt.zero_grad()
            net.loss(net(g, atoms, None, snorm), targets).backward()
            opt.step()
    return step, V, E, graphs


def timed(step):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def measure(workload, dev, steps, warmup, setup=None, knob_name="SMALL_TOWER_TRAIN_ROWS"):
    """setup / knob_name: another tool's workloads and the knob of its route (tools/bench_tower_edge_train.py)."""
    step, V, E, graphs = (setup or globals()["setup"])(workload, dev)
    knobs = {"parent_route": 0, "one_call_route": V}
    times = {k: [] for k in knobs}
    gc.disable()
    try:
        for i in range(warmup + steps):
            for name, knob in knobs.items():                    # the routes alternate step by step
                setattr(PF, knob_name, knob)
                t = timed(step)
                if i >= warmup:
                    times[name].append(t)
    finally:
        gc.enable()
        setattr(PF, knob_name, 0)
    ent = {"graphs": graphs, "V": V, "E": E}
    for name, ts in times.items():
        ent[name] = {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "steps": len(ts)}
    ent["one_call_over_parent"] = ent["one_call_route"]["median_ms"] / ent["parent_route"]["median_ms"]
    return ent


def child(workload, knob, steps, setup=None, knob_name="SMALL_TOWER_TRAIN_ROWS"):
    dev = torch.device("cuda:0")
    step, V, _, _ = (setup or globals()["setup"])(workload, dev)
    setattr(PF, knob_name, V if knob else 0)
    for _ in range(steps):
        step()
    torch.cuda.synchronize()


def _trace_rows(workload, knob, steps, script):
    d = tempfile.mkdtemp(prefix="tower_train_trace_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "st", "--",
           sys.executable, os.path.abspath(script), "--child", workload, "--knob", str(knob), "--steps", str(steps)]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        files = glob.glob(os.path.join(d, "**", "st_kernel_stats.csv"), recursive=True)
        if r.returncode != 0 or not files:
            raise RuntimeError(f"rocprofv3 rc={r.returncode}: {r.stderr[-400:]}")
        return {row["Name"]: (int(row["Calls"]), float(row["TotalDurationNs"])) for row in csv.DictReader(open(files[0]))}
    finally:
        shutil.rmtree(d, ignore_errors=True)


def trace(workload, knob, short=3, long=13, script=__file__):
    """Launches per step and the per-kernel split of the device time: the difference between the rocprofv3 kernel statistics of a child
    that runs `long` steps and one that runs `short` (what the set-up launches -- graph build, initialisation -- cancels out of)."""
    if shutil.which("rocprofv3") is None:
        return {"error": "rocprofv3 not found"}
    try:
        a, b = _trace_rows(workload, knob, short, script), _trace_rows(workload, knob, long, script)
    except (RuntimeError, subprocess.TimeoutExpired) as ex:
        return {"error": str(ex)}
    n = long - short
    rows = [(k, (b[k][0] - a.get(k, (0, 0.0))[0]) / n, (b[k][1] - a.get(k, (0, 0.0))[1]) / n / 1e3) for k in b]
    rows = [r for r in rows if r[1] > 0]
    top = sorted(rows, key=lambda x: -x[2])[:10]
    return {"steps": n, "launches_per_step": sum(r[1] for r in rows), "kernel_us_per_step": sum(r[2] for r in rows),
            "top_kernels": [{"name": k[:80], "calls_per_step": c, "us_per_step": t} for k, c, t in top]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tower_train.json"))
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--child", default=None)
    ap.add_argument("--knob", type=int, default=0)
    args = ap.parse_args()
    if args.child:
        child(args.child, args.knob, args.steps)
        return
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(dev),
           "method": "one process; wall clock per step with a device synchronisation, every step timed once, the routes alternating; "
                     f"{args.steps} steps after {args.warmup} warm-up steps; launches from rocprofv3 --kernel-trace --stats of a child process",
           "workloads": {}}
    for w in args.workloads.split(","):
        ent = measure(w, dev, args.steps, args.warmup)
        if not args.no_trace:
            ent["trace"] = {"parent_route": trace(w, 0), "one_call_route": trace(w, 1)}
        res["workloads"][w] = ent
        print(w, json.dumps({k: v for k, v in ent.items() if k != "trace"}), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
