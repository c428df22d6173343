#!/usr/bin/env python
"""PNALayer training WITH DROPOUT inside the towers on superpixel-shaped batches: the one-call route (autograd.TowerLayerDropSmallTrainFn,
pna_tower_drop_train_fwd_f32 / _bwd_f32; knob PNA_AMD_SMALL_TOWER_TRAIN_DROPOUT_ROWS = V) against the generic route it would replace (knob
0: torch.stack of the weights, the projection GEMMs, AggregateFn, per tower PosttransFn / graph norm / library BatchNorm / dropout node,
cat / Linear / LeakyReLU / residual), both routes in ONE process on one box, by the method of tools/bench_tower_train.py (whose timing
and tracing functions this tool calls):

  * the layer shapes of realworld_benchmark/README.md:65-100 (5 towers over slices of the input, residual asked for): 75 -> 75 and
    75 -> 70, forward + backward, at dropout 0.1 without edge features and at dropout 0.3 with edge_dim 50 (e = a Linear embedding of one
    scalar per edge that takes a gradient, as the net forms it), on a CIFAR10-shaped batch: 128 graphs of about 118 nodes, every node
    with 8 in-edges (about 15 k rows, 121 k edges);
  * a whole four-layer `pna_amd.nets.PNANetSuperpixels` training step (hidden 75, out 70, readout sum, Adam, cross-entropy) on that batch
    at dropout 0.1 without and 0.3 with edge features, and at dropout 0.1 on an MNIST-shaped batch (128 graphs of about 71 nodes).

Every step is timed once with a device synchronisation; the two routes alternate step by step; 20 steps after 5 warm-up steps.  Launches
per step come from child processes under `rocprofv3 --kernel-trace --stats` (no counters in that run).  Every workload is measured in a
child process of its own under a time limit; a child that fails or runs out of time ends the tool, which starts nothing after it.

    python tools/bench_tower_drop_train.py       # writes profiles/tower_drop_train.json
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
from pna_amd import Graph  # noqa: E402
from pna_amd.dgl.pna_layer import PNALayer  # noqa: E402

KNOB = "SMALL_TOWER_TRAIN_DROPOUT_ROWS"
#            name: (kind, out_dim, dropout, edge features, nodes per graph)
WORKLOADS = {
    "cifar_75_75_p01": ("layer", 75, 0.1, False, 118), "cifar_75_70_p01": ("layer", 70, 0.1, False, 118),
    "cifar_75_75_edge_p03": ("layer", 75, 0.3, True, 118), "cifar_75_70_edge_p03": ("layer", 70, 0.3, True, 118),
    "net_cifar_p01": ("net", 70, 0.1, False, 118), "net_cifar_edge_p03": ("net", 70, 0.3, True, 118), "net_mnist_p01": ("net", 70, 0.1, False, 71),
}
MEASURE_LIMIT_S = 240


def superpixel_batch(graphs, nodes, seed=41):
    """`graphs` graphs of nodes - 8 .. nodes + 8 nodes, every node with 8 in-edges from 8 distinct other nodes of its graph (the k = 8
    nearest-neighbour graphs of the superpixel datasets have this degree profile) -> (src, dst, sizes)."""
    gen = torch.Generator().manual_seed(seed)
    sizes = [int(n) for n in torch.randint(nodes - 8, nodes + 9, (graphs,), generator=gen)]
    src, dst, o = [], [], 0
    for n in sizes:
        off = torch.rand(n, n - 1, generator=gen).argsort(1)[:, :8] + 1                # 8 distinct offsets in 1 .. n - 1 per node
        v = torch.arange(n)[:, None]
        src.append(((v + off) % n + o).reshape(-1))
        dst.append((v + o).expand(n, 8).reshape(-1))
        o += n
    src, dst = torch.cat(src), torch.cat(dst)
    order = torch.randperm(src.numel(), generator=gen)
    return src[order].contiguous(), dst[order].contiguous(), sizes


def setup(workload, dev):
    """-> (step function, V, E, graphs)."""
    kind, out_dim, dropout, edge, nodes = WORKLOADS[workload]
    graphs = 128
    src, dst, sizes = superpixel_batch(graphs, nodes)
    V, E = sum(sizes), src.numel()
    g = Graph(src, dst, V, sizes).to(dev)
    avg = {"log": torch.log(g.in_degrees().double() + 1).mean().float().cpu()}
    snorm = torch.cat([torch.full((n, 1), n ** -0.5) for n in sizes]).to(dev)
    torch.manual_seed(0)
    gen = torch.Generator().manual_seed(0)
    ef = torch.rand(E, 1, generator=gen).to(dev)
    if kind == "layer":
        layer = PNALayer(75, out_dim, B.AGG, B.SCA, avg, dropout, True, True, towers=5, pretrans_layers=1, posttrans_layers=1, divide_input=True,
                         residual=True, edge_features=edge, edge_dim=50 if edge else 0).to(dev).train()
        emb = torch.nn.Linear(1, 50).to(dev)
        h = torch.randn(V, 75, device=dev).requires_grad_(True)
        R = torch.randn(V, out_dim, device=dev)

        def step():
            h.grad = None
            layer.zero_grad(set_to_none=True)
            emb.zero_grad(set_to_none=True)
            (layer(g, h, emb(ef) if edge else None, snorm) * R).sum().backward()
    else:
        from pna_amd.nets import PNANetSuperpixels
        net = PNANetSuperpixels(dict(in_dim=5, in_dim_edge=1, hidden_dim=75, out_dim=out_dim, n_classes=10, L=4, readout="sum", edge_feat=edge,
                                     edge_dim=50 if edge else 0, gru=False, in_feat_dropout=0.0, dropout=dropout, graph_norm=True, batch_norm=True,
                                     residual=True, aggregators=B.AGG, scalers=B.SCA, avg_d=avg, towers=5, pretrans_layers=1, posttrans_layers=1,
                                     divide_input_first=True, divide_input_last=True, device=dev)).to(dev).train()
        x = torch.randn(V, 5, generator=gen).to(dev)
        labels = torch.randint(0, 10, (len(sizes),), generator=gen).to(dev)
        opt = torch.optim.Adam(net.parameters(), lr=1e-3)

        def step():
            opt.zero_grad()
            net.loss(net(g, x, ef, snorm), labels).backward()
            opt.step()
    return step, V, E, graphs


def measure_in_child(workload, steps, warmup):
    """B.measure of one workload in a child process under a time limit -> its entry; any failure ends the tool."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tower_drop_train.json"))
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
        ent = B.measure(args.measure, dev, args.steps, args.warmup, setup=setup, knob_name=KNOB)
        ent["device"] = torch.cuda.get_device_name(dev)
        print(json.dumps(ent), flush=True)
        return
    res = {"device": None,
           "method": "both routes in one process per workload; wall clock per step with a device synchronisation, every step timed once, the "
                     f"routes alternating; {args.steps} steps after {args.warmup} warm-up steps; launches from rocprofv3 --kernel-trace --stats of "
                     "child processes",
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
