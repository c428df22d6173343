#!/usr/bin/env python
"""PNALayer training with ANOTHER LIST OF AGGREGATORS than mean max min std: the one-call route (autograd.TowerLayerAggrSmallTrainFn,
pna_tower_aggr_train_fwd_f32 / _bwd_f32; knob PNA_AMD_SMALL_TOWER_TRAIN_AGGR_ROWS = V) against the generic route it would replace (the
knob at 0 on the same commit), both routes in ONE process on one box, after tools/bench_tower_drop_train.py (whose batch and whose
tracing this tool uses):

  * the MPNN layer shapes of realworld_benchmark/README.md:91-100 (`sum` or `max` with the identity scaler, 5 towers over slices of the
    input, residual asked for), forward + backward: on 128 ZINC-shaped molecules `sum` at 110 -> 110 and 110 -> 80 and, with edge features
    (edge_dim 50), at 100 -> 100 and 100 -> 70; on 128 CIFAR10-shaped graphs `max` at dropout 0.2, 110 -> 90, with and without edge_dim 20;
  * a whole four-layer `pna_amd.nets.PNANet` training step with `sum` (hidden 110, out 80, readout sum, Adam) on the molecule batch with
    the other one-call knobs that serve this net (PNA_AMD_NET_ENDS_ROWS, PNA_AMD_MLP_HEAD_ROWS) on in BOTH routes.

Every step is timed once with a device synchronisation; the two routes alternate step by step; 3 blocks of 20 steps after 5 warm-up
steps.  The figure of a route is the median of its three block medians, its margin the spread (max - min) of the block medians.  Launches
per step come from child processes under `rocprofv3 --kernel-trace --stats` (no counters in that run).  Every workload is measured in a
child process of its own under a time limit; a child that fails or runs out of time ends the tool, which starts nothing after it.

    python tools/bench_tower_aggr_train.py       # writes profiles/tower_aggr_train.json
"""
import argparse
import gc
import json
import os
import shutil
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench_tower_train as B  # noqa: E402
from bench_tower_drop_train import superpixel_batch  # noqa: E402
from pna_amd import Graph  # noqa: E402
from pna_amd import functional as PF  # noqa: E402
from pna_amd.dgl.pna_layer import PNALayer  # noqa: E402
from pna_amd.synth import molecule_batch  # noqa: E402

KNOB = "SMALL_TOWER_TRAIN_AGGR_ROWS"
OTHER_KNOBS = ("NET_ENDS_ROWS", "MLP_HEAD_ROWS")              # on in both routes of the net workload
#            name: (kind, batch, aggregators, in_dim, out_dim, dropout, edge_dim)
WORKLOADS = {
    "zinc_sum_110_110": ("layer", "zinc", "sum", 110, 110, 0.0, 0), "zinc_sum_110_80": ("layer", "zinc", "sum", 110, 80, 0.0, 0),
    "zinc_sum_edge_100_100": ("layer", "zinc", "sum", 100, 100, 0.0, 50), "zinc_sum_edge_100_70": ("layer", "zinc", "sum", 100, 70, 0.0, 50),
    "cifar_max_110_90_p02": ("layer", "cifar", "max", 110, 90, 0.2, 0), "cifar_max_edge_110_90_p02": ("layer", "cifar", "max", 110, 90, 0.2, 20),
    "net_zinc_sum": ("net", "zinc", "sum", 110, 80, 0.0, 0),
}
MEASURE_LIMIT_S = 300
BLOCKS = 3


def setup(workload, dev):
    """-> (step function, V, E, graphs)."""
    kind, batch, aggs, in_dim, out_dim, dropout, ed = WORKLOADS[workload]
    graphs = 128
    src, dst, sizes = molecule_batch(graphs, seed=41) if batch == "zinc" else superpixel_batch(graphs, 118)
    V, E = sum(sizes), src.numel()
    g = Graph(src, dst, V, sizes).to(dev)
    avg = {"log": torch.log(g.in_degrees().double() + 1).mean().float().cpu()}
    snorm = torch.cat([torch.full((n, 1), n ** -0.5) for n in sizes]).to(dev)
    torch.manual_seed(0)
    gen = torch.Generator().manual_seed(0)
    if kind == "layer":
        layer = PNALayer(in_dim, out_dim, aggs, "identity", avg, dropout, True, True, towers=5, pretrans_layers=1, posttrans_layers=1, divide_input=True,
                         residual=True, edge_features=ed > 0, edge_dim=ed).to(dev).train()
        ef = torch.rand(E, 1, generator=gen).to(dev)
        emb = torch.nn.Linear(1, max(ed, 1)).to(dev)
        h = torch.randn(V, in_dim, device=dev).requires_grad_(True)
        R = torch.randn(V, out_dim, device=dev)

        def step():
            h.grad = None
            layer.zero_grad(set_to_none=True)
            emb.zero_grad(set_to_none=True)
            (layer(g, h, emb(ef) if ed else None, snorm) * R).sum().backward()
    else:
        from pna_amd.nets import PNANet
        for k in OTHER_KNOBS:
            setattr(PF, k, 1 << 20)
        net = PNANet(dict(hidden_dim=in_dim, out_dim=out_dim, L=4, readout="sum", edge_feat=False, gru=False, in_feat_dropout=0.0, dropout=0.0,
                          graph_norm=True, batch_norm=True, residual=True, aggregators=aggs, scalers="identity", avg_d=avg, towers=5, edge_dim=0,
                          pretrans_layers=1, posttrans_layers=1, divide_input_first=True, divide_input_last=True, num_atom_type=28,
                          num_bond_type=4, device=dev)).to(dev).train()
        atoms = torch.randint(0, 28, (V,), generator=gen).to(dev)
        targets = torch.randn(len(sizes), 1, generator=gen).to(dev)
        opt = torch.optim.Adam(net.parameters(), lr=1e-3)

        def step():
            opt.zero_grad()
            net.loss(net(g, atoms, None, snorm), targets).backward()
            opt.step()
    return step, V, E, graphs


def measure(workload, dev, steps, warmup):
    """BLOCKS blocks of `steps` steps per route, the routes alternating step by step -> the entry of the result file."""
    step, V, E, graphs = setup(workload, dev)
    knobs = {"parent_route": 0, "one_call_route": V}
    blocks = {k: [[] for _ in range(BLOCKS)] for k in knobs}
    gc.disable()
    try:
        for i in range(warmup + BLOCKS * steps):
            for name, knob in knobs.items():
                setattr(PF, KNOB, knob)
                t = B.timed(step)
                if i >= warmup:
                    blocks[name][(i - warmup) // steps].append(t)
    finally:
        gc.enable()
        setattr(PF, KNOB, 0)
    ent = {"graphs": graphs, "V": V, "E": E}
    for name, bs in blocks.items():
        meds = [statistics.median(b) for b in bs]
        ent[name] = {"median_ms": statistics.median(meds), "block_medians_ms": meds, "margin_ms": max(meds) - min(meds), "steps_per_block": steps}
    ent["one_call_over_parent"] = ent["one_call_route"]["median_ms"] / ent["parent_route"]["median_ms"]
    return ent


def measure_in_child(workload, steps, warmup):
    """measure() of one workload in a child process under a time limit -> its entry; any failure ends the tool."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tower_aggr_train.json"))
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--child", default=None)
    ap.add_argument("--measure", default=None)
    ap.add_argument("--knob", type=int, default=0)
    args = ap.parse_args()
    if args.child:
        B.child(args.child, args.knob, args.steps, setup=setup, knob_name=KNOB)
        return
    if args.measure:
        dev = torch.device("cuda:0")
        ent = measure(args.measure, dev, args.steps, args.warmup)
        ent["device"] = torch.cuda.get_device_name(dev)
        print(json.dumps(ent), flush=True)
        return
    res = {"device": None,
           "method": "both routes in one process per workload; wall clock per step with a device synchronisation, every step timed once, the "
                     f"routes alternating; {BLOCKS} blocks of {args.steps} steps after {args.warmup} warm-up steps; a route's figure is the median of "
                     "its block medians, its margin their spread; launches from rocprofv3 --kernel-trace --stats of child processes",
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
                if "error" in ent["trace"][route]:                  # a child failed or ran out of time: keep what there is and stop
                    res["workloads"][w] = ent
                    save()
                    raise SystemExit(f"{w}: tracing the {route} failed ({ent['trace'][route]['error']}); nothing further is started")
        res["workloads"][w] = ent
        print(w, json.dumps({k: v for k, v in ent.items() if k != "trace"}), flush=True)
        save()


if __name__ == "__main__":
    main()
