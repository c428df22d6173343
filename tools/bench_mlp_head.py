#!/usr/bin/env python
"""The dense heads on the one-call route (autograd.MlpHeadFn: pna_mlp_head_fwd_f32 / _bwd_f32; knob PNA_AMD_MLP_HEAD_ROWS covering the
rows) against the route it would replace (knob 0: nn.Linear GEMMs and elementwise activations), in ONE process on one box:

  * readout_70_1_128 / readout_70_1_2048 / readout_70_10_128: nets.MLPReadout(70, 1 or 10) on 128 or 2 048 graph rows;
  * multitask_head_16x15 / multitask_head_16x97: the multitask GNN's nodes_read_out (layers.MLP, 16-16-16-3, LeakyReLU after each
    layer) on (16, N, 16) node rows;
  * embedding_h_15168: the superpixel net's nn.Linear(5, 75) node embedding on the 15 168 rows of a 128-graph CIFAR10-shaped batch;
  * net_hiv: a whole PNANetHIV training step (tools/bench_net_ends.py's 2 048-graph batch, Adam) with the other one-call knobs on for
    both routes;
  * net_multitask: a whole multitask training step (tools/bench_set2set.py's 16 x 15 batch, Adam) with the other one-call knobs on for
    both routes.

Each piece is forward + backward (every input and parameter gradient); every step is timed once (host clock around the step and a device
synchronisation); the two routes alternate step by step, so drift hits both; the garbage collector is off.  Reported: the median of 3
blocks of 20 steps after 5 warm-up steps, the blocks' own medians, and their spread -- the margin a difference has to exceed.  Launches
per step come from fresh child processes of this tool's own under `rocprofv3 --kernel-trace --stats` (no counters in that run).

    python tools/bench_mlp_head.py            # writes profiles/mlp_head.json
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
import bench_net_ends as BN  # noqa: E402
import bench_set2set as BS  # noqa: E402
from bench_small_train import timed  # noqa: E402
from pna_amd import functional as PF, layers, nets  # noqa: E402

WORKLOADS = ("readout_70_1_128", "readout_70_1_2048", "readout_70_10_128", "multitask_head_16x15", "multitask_head_16x97",
             "embedding_h_15168", "net_hiv", "net_multitask")
KNOB_ON = 1 << 30


class _Embedding(torch.nn.Module):
    """PNANetSuperpixels.embedding_h as its forward applies it."""

    def __init__(self, in_dim, hidden):
        super().__init__()
        self.lin = torch.nn.Linear(in_dim, hidden)

    def forward(self, x):
        return nets.linear_rows(self.lin, x)


def setup(workload, dev):
    """-> (step function, rows).  The nets' other one-call knobs are set here, for both routes."""
    torch.manual_seed(0)
    gen = torch.Generator().manual_seed(1)
    if workload == "net_hiv":
        step, V, _, graphs = BN.setup("hiv_2048", "net", dev)
        PF.SMALL_TRAIN_ROWS = PF.NET_ENDS_ROWS = KNOB_ON
        return step, graphs
    if workload == "net_multitask":
        step, B, N = BS.setup("step_16x15", dev)
        BS.set_knobs("step", True)
        return step, B * N
    if workload.startswith("readout"):
        _, _, out, rows = workload.split("_")
        mod, shape, width = nets.MLPReadout(70, int(out)).to(dev).train(), (int(rows), 70), int(out)
    elif workload.startswith("multitask_head"):
        B, N = (int(v) for v in workload.split("_")[2].split("x"))
        mod = layers.MLP(16, 16, 3, 3, mid_activation="LeakyReLU", last_activation="LeakyReLU", device=dev).train()
        shape, width = (B, N, 16), 3
    else:
        mod, shape, width = _Embedding(5, 75).to(dev), (int(workload.split("_")[2]), 5), 75
    x = torch.randn(*shape, generator=gen).to(dev).requires_grad_(True)
    R = torch.randn(*shape[:-1], width, generator=gen).to(dev)

    def step():
        mod.zero_grad(set_to_none=True)
        x.grad = None
        (mod(x) * R).sum().backward()
    rows = 1
    for s in shape[:-1]:
        rows *= s
    return step, rows


def measure(workload, dev, steps, warmup, blocks):
    step, rows = setup(workload, dev)
    knobs = {"parent_route": 0, "one_call_route": KNOB_ON}
    times = {k: [] for k in knobs}
    gc.disable()
    try:
        for i in range(warmup + blocks * steps):
            for name, knob in knobs.items():                    # the routes alternate step by step
                PF.MLP_HEAD_ROWS = knob
                t = timed(step)
                if i >= warmup:
                    times[name].append(t)
    finally:
        gc.enable()
        PF.MLP_HEAD_ROWS = 0
    ent = {"rows": rows}
    for name, ts in times.items():
        meds = [statistics.median(ts[r * steps:(r + 1) * steps]) for r in range(blocks)]
        ent[name] = {"median_ms": statistics.median(meds), "block_median_ms": meds, "block_spread_ms": max(meds) - min(meds),
                     "min_ms": min(ts), "max_ms": max(ts), "steps": len(ts)}
    spread = max(ent[k]["block_spread_ms"] for k in knobs)
    ent["margin_ms"] = spread
    ent["one_call_over_parent"] = ent["one_call_route"]["median_ms"] / ent["parent_route"]["median_ms"]
    ent["one_call_loses_by_more_than_the_spread"] = ent["one_call_route"]["median_ms"] > ent["parent_route"]["median_ms"] + spread
    ent["one_call_wins_by_more_than_the_spread"] = ent["one_call_route"]["median_ms"] < ent["parent_route"]["median_ms"] - spread
    return ent


def child(workload, knob, steps):
    dev = torch.device("cuda:0")
    step, _ = setup(workload, dev)
    PF.MLP_HEAD_ROWS = KNOB_ON if knob else 0
    for _ in range(steps):
        step()
    torch.cuda.synchronize()


def _trace_rows(workload, knob, steps):
    d = tempfile.mkdtemp(prefix="mlp_trace_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "mlp", "--",
           sys.executable, os.path.abspath(__file__), "--child", workload, "--knob", str(knob), "--steps", str(steps)]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        files = glob.glob(os.path.join(d, "**", "mlp_kernel_stats.csv"), recursive=True)
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
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mlp_head.json"))
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--child", default=None)
    ap.add_argument("--knob", type=int, default=0)
    args = ap.parse_args()
    if args.child:
        child(args.child, args.knob, args.steps)
        return
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(dev),
           "method": "one process; garbage collector off; wall clock per step with a device synchronisation, every step timed once, the "
                     f"routes alternating; medians of {args.blocks} blocks of {args.steps} steps after {args.warmup} warm-up steps, the spread "
                     "of the block medians as the margin; launches from rocprofv3 --kernel-trace --stats of fresh child processes",
           "workloads": {}}
    for w in args.workloads.split(","):
        ent = measure(w, dev, args.steps, args.warmup, args.blocks)
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
