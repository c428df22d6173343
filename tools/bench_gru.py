#!/usr/bin/env python
"""The GRU update between two message-passing steps on the one-call route (autograd.GruCellFn: pna_gru_cell_fwd_f32 / _bwd_f32; knob
PNA_AMD_GRU_ROWS covering the rows) against the route it would replace (knob 0: nn.GRU over a length-1 sequence, the vendor RNN
library), in ONE process on one box:

  * multitask_h16: layers.GRU(16, 16) on one batch of the c1_train_trace golden (B x N rows), the FIRST call's 2-column x;
  * zinc_h75 / zinc_h110: nets.GRU on the rows of a 128-graph ZINC-shaped batch at hidden 75 and 110;
  * molhiv_h80: nets.GRU at hidden 80 on the ~52 k rows of a 2 048-graph MolHIV-shaped batch;
  * net_zinc_gru: a whole PNANet(gru=True) training step (4 layers, hidden 75, towers 5, Adam) on the 128-graph batch with the other
    one-call knobs on for both routes.

Each piece is forward + backward (every input and parameter gradient); every step is timed once (host clock around the step and a device
synchronisation); the two routes alternate step by step, so drift hits both.  Launches per step come from a fresh child process of this
tool's own under `rocprofv3 --kernel-trace --stats` (no counters in that run), one pair of children per workload and route.

    python tools/bench_gru.py            # writes profiles/gru_cell.json
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

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_small_train import timed  # noqa: E402
from pna_amd import Graph, functional as PF, layers, nets  # noqa: E402
from pna_amd.synth import molecule_batch  # noqa: E402

AGG, SCA = "mean max min std", "identity amplification attenuation"
WORKLOADS = ("multitask_h16", "zinc_h75", "zinc_h110", "molhiv_h80", "net_zinc_gru")
KNOB_ON = 1 << 30


def _rows_of(workload):
    if workload == "multitask_h16":
        z = np.load(os.path.join(ROOT, "tests", "golden", "c1_train_trace_n15.npz"), allow_pickle=False)
        meta = json.loads(str(z["meta"]))
        return meta["B"], meta["N"]
    if workload == "molhiv_h80":
        return sum(molecule_batch(2048, mean_nodes=25.5, sd_nodes=12, lo=6, hi=222, seed=41, lognormal=True)[2]), None
    return sum(molecule_batch(128, seed=41)[2]), None


def setup(workload, dev):
    """-> (step function, rows, hidden)."""
    torch.manual_seed(0)
    if workload == "net_zinc_gru":
        src, dst, sizes = molecule_batch(128, seed=41)
        V = sum(sizes)
        g = Graph(src, dst, V, sizes).to(dev)
        avg = {"log": torch.log(g.in_degrees().double() + 1).mean().float().cpu()}
        net = nets.PNANet(dict(num_atom_type=28, num_bond_type=4, hidden_dim=75, out_dim=70, in_feat_dropout=0.0, dropout=0.0, L=4,
                               readout="sum", graph_norm=True, batch_norm=True, residual=True, aggregators=AGG, scalers=SCA, avg_d=avg,
                               towers=5, divide_input_first=False, divide_input_last=True, edge_feat=False, edge_dim=0, pretrans_layers=1,
                               posttrans_layers=1, gru=True, device=dev)).to(dev).train()
        gen = torch.Generator().manual_seed(0)
        atoms = torch.randint(0, 28, (V,), generator=gen).to(dev)
        snorm = torch.cat([torch.full((n, 1), n ** -0.5) for n in sizes]).to(dev)
        y = torch.randn(len(sizes), 1, generator=gen).to(dev)
        opt = torch.optim.Adam(net.parameters(), lr=1e-3)
        PF.SMALL_TOWER_TRAIN_ROWS = PF.NET_ENDS_ROWS = KNOB_ON               # the other one-call routes, for both GRU routes

        def step():
            opt.zero_grad()
            net.loss(net(g, atoms, None, snorm), y).backward()
            opt.step()
        return step, V, 75
    rows, N = _rows_of(workload)
    if workload == "multitask_h16":
        H, mod = 16, layers.GRU(16, 16, dev)
        x = torch.randn(rows, N, 2, device=dev).requires_grad_(True)
        h = torch.randn(rows, N, 16, device=dev).requires_grad_(True)
        R = torch.randn(rows, N, 16, device=dev)
        rows = rows * N
    else:
        H = {"zinc_h75": 75, "zinc_h110": 110, "molhiv_h80": 80}[workload]
        mod = nets.GRU(H, H, dev)
        x = torch.randn(rows, H, device=dev).requires_grad_(True)
        h = torch.randn(rows, H, device=dev).requires_grad_(True)
        R = torch.randn(rows, H, device=dev)

    def step():
        mod.zero_grad(set_to_none=True)
        x.grad = h.grad = None
        (mod(x, h) * R).sum().backward()
    return step, rows, H


def measure(workload, dev, steps, warmup):
    step, rows, H = setup(workload, dev)
    knobs = {"parent_route": 0, "one_call_route": KNOB_ON}
    times = {k: [] for k in knobs}
    gc.disable()
    try:
        for i in range(warmup + steps):
            for name, knob in knobs.items():                    # the routes alternate step by step
                PF.GRU_ROWS = knob
                t = timed(step)
                if i >= warmup:
                    times[name].append(t)
    finally:
        gc.enable()
        PF.GRU_ROWS = 0
    ent = {"rows": rows, "hidden": H}
    for name, ts in times.items():
        ent[name] = {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "steps": len(ts)}
    ent["one_call_over_parent"] = ent["one_call_route"]["median_ms"] / ent["parent_route"]["median_ms"]
    return ent


def child(workload, knob, steps):
    dev = torch.device("cuda:0")
    step, _, _ = setup(workload, dev)
    PF.GRU_ROWS = KNOB_ON if knob else 0
    for _ in range(steps):
        step()
    torch.cuda.synchronize()


def _trace_rows(workload, knob, steps):
    d = tempfile.mkdtemp(prefix="gru_trace_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "gru", "--",
           sys.executable, os.path.abspath(__file__), "--child", workload, "--knob", str(knob), "--steps", str(steps)]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        files = glob.glob(os.path.join(d, "**", "gru_kernel_stats.csv"), recursive=True)
        if r.returncode != 0 or not files:
            raise RuntimeError(f"rocprofv3 rc={r.returncode}: {r.stderr[-400:]}")
        return {row["Name"]: (int(row["Calls"]), float(row["TotalDurationNs"])) for row in csv.DictReader(open(files[0]))}
    finally:
        shutil.rmtree(d, ignore_errors=True)


def trace(workload, knob, short=3, long=13):
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
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gru_cell.json"))
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
        if not args.no_trace:
            print(w, "launches per step:", {k: v.get("launches_per_step", v.get("error")) for k, v in ent["trace"].items()}, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
