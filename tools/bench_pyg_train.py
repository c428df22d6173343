#!/usr/bin/env python
"""pytorch_geometric.PNAConv in fp32: the one-call route (autograd.PygConvFn, pna_pyg_conv_train_fwd_f32 / _bwd_f32; knob
PNA_AMD_PYG_TRAIN_ROWS = V) against the generic route it would replace (the knob at 0 on the same commit), both routes in ONE process on
one box, by the method of tools/bench_tower_aggr_train.py (whose timing and tracing helpers this tool uses):

  * PyG's ZINC example layer (75 -> 75, 5 towers, mean min max std, identity amplification attenuation, divide_input=False) on 128
    ZINC-shaped molecules, forward + backward, with edge_dim 50 and without edge features;
  * a four-layer stack of that layer with BatchNorm1d + ReLU between the layers and Adam, edge_dim 50;
  * a no-grad forward of an 80 -> 80 layer (4 towers) on 128 MolHIV-shaped molecules.

Every step is timed once with a device synchronisation; the two routes alternate step by step; 3 blocks of 20 steps after 5 warm-up
steps.  The figure of a route is the median of its three block medians, its margin the spread (max - min) of the block medians.  Launches
per step come from child processes under `rocprofv3 --kernel-trace --stats` (no counters in that run).  Every workload is measured in a
child process of its own under a time limit; a child that fails or runs out of time ends the tool, which starts nothing after it.

    python tools/bench_pyg_train.py       # writes profiles/pyg_train.json
"""
import argparse
import json
import os
import shutil
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench_tower_train as B  # noqa: E402
import bench_tower_aggr_train as BA  # noqa: E402
from pna_amd.pytorch_geometric import PNAConv  # noqa: E402
from pna_amd.synth import molecule_batch  # noqa: E402

KNOB = "PYG_TRAIN_ROWS"
A4, S3 = ["mean", "min", "max", "std"], ["identity", "amplification", "attenuation"]
#            name: (kind, channels, towers, edge_dim, molecules' seed)
WORKLOADS = {
    "zinc_edge_75_75": ("layer", 75, 5, 50, 41),
    "zinc_75_75": ("layer", 75, 5, 0, 41),
    "zinc_stack4_edge": ("stack", 75, 5, 50, 41),
    "molhiv_nograd_80_80": ("nograd", 80, 4, 0, 43),
}
MEASURE_LIMIT_S = 300


class Stack(torch.nn.Module):
    def __init__(self, C, T, ed, hist, L=4):
        super().__init__()
        self.convs = torch.nn.ModuleList([PNAConv(C, C, A4, S3, hist, edge_dim=ed or None, towers=T, divide_input=False) for _ in range(L)])
        self.bns = torch.nn.ModuleList([torch.nn.BatchNorm1d(C) for _ in range(L - 1)])

    def forward(self, x, ei, e):
        for i, conv in enumerate(self.convs):
            x = conv(x, ei, e)
            if i < len(self.bns):
                x = torch.relu(self.bns[i](x))
        return x


def setup(workload, dev):
    """-> (step function, V, E, graphs)."""
    kind, C, T, ed, seed = WORKLOADS[workload]
    graphs = 128
    src, dst, sizes = molecule_batch(graphs, seed=seed)
    V, E = sum(sizes), src.numel()
    ei = torch.stack([src, dst]).to(dev)
    hist = torch.bincount(torch.bincount(dst, minlength=V)).long()
    torch.manual_seed(0)
    x = torch.randn(V, C, device=dev).requires_grad_(kind != "nograd")
    e = torch.randn(E, ed, device=dev).requires_grad_(True) if ed else None
    R = torch.randn(V, C, device=dev)
    if kind == "stack":
        net = Stack(C, T, ed, hist).to(dev).train()
        opt = torch.optim.Adam(net.parameters(), lr=1e-3)

        def step():
            opt.zero_grad()
            (net(x, ei, e) * R).sum().backward()
            opt.step()
        return step, V, E, graphs
    layer = PNAConv(C, C, A4, S3, hist, edge_dim=ed or None, towers=T, divide_input=False).to(dev)
    if kind == "nograd":
        layer.eval()

        def step():
            with torch.no_grad():
                layer(x, ei, e)
        return step, V, E, graphs
    layer.train()

    def step():
        x.grad = None
        if e is not None:
            e.grad = None
        layer.zero_grad(set_to_none=True)
        (layer(x, ei, e) * R).sum().backward()
    return step, V, E, graphs


def measure_in_child(workload, steps, warmup):
    cmd = [sys.executable, os.path.abspath(__file__), "--measure", workload, "--steps", str(steps), "--warmup", str(warmup)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=MEASURE_LIMIT_S)
    if r.returncode != 0:
        raise SystemExit(f"{workload}: the measuring child ended with {r.returncode}; nothing further is started\n{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pyg_train.json"))
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--child", default=None)
    ap.add_argument("--measure", default=None)
    ap.add_argument("--knob", type=int, default=0)
    args = ap.parse_args()
    BA.KNOB, BA.setup = KNOB, setup                      # bench_tower_aggr_train.measure with this tool's knob and workloads
    if args.child:
        B.child(args.child, args.knob, args.steps, setup=setup, knob_name=KNOB)
        return
    if args.measure:
        dev = torch.device("cuda:0")
        ent = BA.measure(args.measure, dev, args.steps, args.warmup)
        ent["device"] = torch.cuda.get_device_name(dev)
        print(json.dumps(ent), flush=True)
        return
    res = {"device": None,
           "method": "both routes in one process per workload; wall clock per step with a device synchronisation, every step timed once, the "
                     f"routes alternating; {BA.BLOCKS} blocks of {args.steps} steps after {args.warmup} warm-up steps; a route's figure is the median "
                     "of its block medians, its margin their spread; launches from rocprofv3 --kernel-trace --stats of child processes",
           "workloads": {}}

    def save():
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    for w in args.workloads.split(","):
        try:
            ent = measure_in_child(w, args.steps, args.warmup)
        except (subprocess.TimeoutExpired, SystemExit):
            save()
            raise
        res["device"] = ent.pop("device")
        if not args.no_trace and shutil.which("rocprofv3") is None:
            ent["trace"] = {"error": "rocprofv3 not found"}
        elif not args.no_trace:
            ent["trace"] = {}
            for route, knob in (("parent_route", 0), ("one_call_route", 1)):
                ent["trace"][route] = B.trace(w, knob, script=__file__)
                if "error" in ent["trace"][route]:              # a child failed or ran out of time: keep what there is and stop
                    res["workloads"][w] = ent
                    save()
                    raise SystemExit(f"{w}: tracing the {route} failed ({ent['trace'][route]['error']}); nothing further is started")
        res["workloads"][w] = ent
        print(w, json.dumps({k: v for k, v in ent.items() if k != "trace"}), flush=True)
        save()


if __name__ == "__main__":
    main()
