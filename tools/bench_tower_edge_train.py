#!/usr/bin/env python
"""PNALayer training WITH EDGE FEATURES on ZINC-shaped molecule batches: the one-call route (autograd.TowerLayerEdgeSmallTrainFn,
pna_tower_edge_train_fwd_f32 / _bwd_f32; knob PNA_AMD_SMALL_TOWER_TRAIN_EDGE_ROWS = V) against the generic route it would replace (knob
0: torch.stack of the weights, the gather of e[eid], the projection and edge GEMMs, AggregateFn with edge_term and its atomic backward,
per tower PosttransFn / graph norm / BatchNorm, cat / Linear / LeakyReLU), in ONE process on one box, by the method of
tools/bench_tower_train.py (whose timing and tracing functions this tool calls):

  * a ZINC edge-feature layer (realworld_benchmark/README.md:62: 5 towers over slices, edge_dim 50), 70 -> 70 with the residual and
    70 -> 60 without, forward + backward with e = emb[bond type] of a 4-row embedding that takes a gradient, on a synthetic
    128-molecule batch and on a 2 048-molecule batch;
  * a whole ZINC `pna_amd.nets.PNANet` training step (L = 4, hidden 70, out 60, edge_feat True, edge_dim 50, Adam) on both batches.

Every step is timed once with a device synchronisation; the two routes alternate step by step; 20 steps after 5 warm-up steps.  Launches
per step come from a child process under `rocprofv3 --kernel-trace --stats` (no counters in that run).

    python tools/bench_tower_edge_train.py       # writes profiles/tower_edge_train.json
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench_tower_train as B  # noqa: E402
from pna_amd import Graph  # noqa: E402
from pna_amd.dgl.pna_layer import PNALayer  # noqa: E402
from pna_amd.synth import molecule_batch  # noqa: E402

KNOB = "SMALL_TOWER_TRAIN_EDGE_ROWS"
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
    gen = torch.Generator().manual_seed(0)
    bonds = torch.randint(0, 4, (E,), generator=gen).to(dev)
    if kind in ("first", "last"):
        out_dim = 70 if kind == "first" else 60
        layer = PNALayer(70, out_dim, B.AGG, B.SCA, avg, 0.0, True, True, towers=5, pretrans_layers=1, posttrans_layers=1, divide_input=True,
                         residual=True, edge_features=True, edge_dim=50).to(dev).train()
        emb = torch.nn.Embedding(4, 50).to(dev)
        h = torch.randn(V, 70, device=dev).requires_grad_(True)
        R = torch.randn(V, out_dim, device=dev)

        def step():
            h.grad = None
            layer.zero_grad(set_to_none=True)
            emb.zero_grad(set_to_none=True)
            (layer(g, h, emb(bonds), snorm) * R).sum().backward()
    else:
        from pna_amd.nets import PNANet
        net = PNANet(dict(hidden_dim=70, out_dim=60, L=4, readout="sum", edge_feat=True, gru=False, in_feat_dropout=0.0, dropout=0.0,
                          graph_norm=True, batch_norm=True, residual=True, aggregators=B.AGG, scalers=B.SCA, avg_d=avg, towers=5, edge_dim=50,
                          pretrans_layers=1, posttrans_layers=1, divide_input_first=True, divide_input_last=True, num_atom_type=28,
                          num_bond_type=4, device=dev)).to(dev).train()
        atoms = torch.randint(0, 28, (V,), generator=gen).to(dev)
        targets = torch.randn(len(sizes), 1, generator=gen).to(dev)
        opt = torch.optim.Adam(net.parameters(), lr=1e-3)

        def step():
            opt.zero_grad()
            net.loss(net(g, atoms, bonds, snorm), targets).backward()
            opt.step()
    return step, V, E, graphs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tower_edge_train.json"))
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--child", default=None)
    ap.add_argument("--knob", type=int, default=0)
    args = ap.parse_args()
    if args.child:
        B.child(args.child, args.knob, args.steps, setup=setup, knob_name=KNOB)
        return
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(dev),
           "method": "one process; wall clock per step with a device synchronisation, every step timed once, the routes alternating; "
                     f"{args.steps} steps after {args.warmup} warm-up steps; launches from rocprofv3 --kernel-trace --stats of a child process",
           "workloads": {}}
    for w in args.workloads.split(","):
        ent = B.measure(w, dev, args.steps, args.warmup, setup=setup, knob_name=KNOB)
        if not args.no_trace:
            ent["trace"] = {"parent_route": B.trace(w, 0, script=__file__), "one_call_route": B.trace(w, 1, script=__file__)}
        res["workloads"][w] = ent
        print(w, json.dumps({k: v for k, v in ent.items() if k != "trace"}), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
