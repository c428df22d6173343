#!/usr/bin/env python
"""Same-box timing of the fp32 and the bf16 PNALayer forward (inference), and the accuracy figures of the bf16 tower tests.

    python tools/bench_bf16_tower.py [--shapes zinc,zinc_bonds,molhiv,big] [--steps 20] [--warmup 5] [--no-accuracy]
                                     [--out profiles/bf16_tower.json]

Shapes:
  zinc        128 molecule graphs (pna_amd/synth.py::molecule_batch), hidden 75, 5 towers over the whole input
  zinc_bonds  the same with edge features that are an embedding of 4 bond types (edge_dim 50)
  molhiv      the 2 048-graph MolHIV-shaped batch, hidden 80, 8 towers over slices of the input
  big         one tower of F = 75 on the bench graph (powerlaw_graph, seed 1234): V = 1 M, E = 10 M
Every layer: the four standard aggregators, three scalers, graph norm, BatchNorm, residual.  Method: HIP
events around `steps` forwards after `warmup` ones, gc disabled around the timed steps; fp32 first, then bf16, in one process.  The
fp32 figure is whatever path the fp32 layer takes for that shape (the one-call kernel for molecule batches, the one-kernel
degree-ordered layer for the big graph); the bf16 layer is the four launches of functional.tower_layer_bf16.

Accuracy: rho(emu) and rho(gpu) of every tower fixture and both sides of the net-level bar, computed by the functions the tests
assert on (tests/test_gpu_bf16_tower_layers.py)."""
import argparse
import copy
import gc
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

AGGS, SCALERS = "mean max min std", "identity amplification attenuation"
SHAPES = ("zinc", "zinc_bonds", "molhiv", "big")


def setup(shape, dev):
    """-> (graph, fp32 layer, bf16 layer, (h, e, snorm_n) in fp32, the same in bf16, description)"""
    from pna_amd.dgl.pna_layer import PNALayer
    from pna_amd.graph import Graph
    from pna_amd.synth import molecule_batch, powerlaw_graph
    torch.manual_seed(0)
    if shape == "big":
        V, E, hidden, towers, divide, ed = 1_000_000, 10_000_000, 75, 1, False, 0
        src, dst = powerlaw_graph(V, E, seed=1234, device=dev)
        g = Graph(src, dst, V)
        snorm = torch.full((V, 1), 1e-3, device=dev)
    else:
        if shape == "molhiv":
            src, dst, sizes = molecule_batch(2048, mean_nodes=25.5, sd_nodes=12, lo=6, hi=222, seed=41, lognormal=True)
            hidden, towers, divide, ed = 80, 8, True, 0
        else:
            src, dst, sizes = molecule_batch(128, seed=41)
            hidden, towers, divide, ed = 75, 5, False, 50 if shape == "zinc_bonds" else 0
        V, E = int(sum(sizes)), src.numel()
        g = Graph(src, dst, V, sizes).to(dev)
        snorm = g.snorm_n()
    avg_log = torch.log(g.in_degrees().double() + 1).mean().float()
    layer = PNALayer(hidden, hidden, AGGS, SCALERS, {"log": avg_log}, 0.0, True, True, towers=towers, divide_input=divide, residual=True,
                     edge_features=ed > 0, edge_dim=ed).to(dev).eval()
    with torch.no_grad():
        for p in layer.parameters():
            if p.dim() == 2:
                p.copy_(torch.randn_like(p) / p.shape[1] ** 0.5)
    h = torch.randn(V, hidden, device=dev)
    e = None
    if ed:
        table = torch.randn(4, ed, device=dev)
        e = table[torch.randint(0, 4, (E,), device=dev)]
    bf = lambda t: None if t is None else t.to(torch.bfloat16)
    desc = {"V": V, "E": E, "hidden": hidden, "towers": towers, "divide_input": divide, "edge_dim": ed}
    return g, layer, copy.deepcopy(layer).to(torch.bfloat16), (h, e, snorm), (bf(h), bf(e), bf(snorm)), desc


def time_forward(layer, g, inputs, steps, warmup):
    h, e, sn = inputs
    with torch.no_grad():
        for _ in range(warmup):
            layer(g, h, e, sn)
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        gc.disable()
        try:
            t0.record()
            for _ in range(steps):
                layer(g, h, e, sn)
            t1.record()
            torch.cuda.synchronize()
        finally:
            gc.enable()
    return t0.elapsed_time(t1) / steps


def accuracy(dev):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_gpu_bf16_tower_layers as T
    return {"bar_layers": "rho(gpu) <= 2 rho(emu), rho(x) = max |x - ref64| / E", "layers": [T.layer_figures(n, dev) for n in T.TOWER_FIXTURES],
            "bar_nets": "max |gpu - emu| <= 2 max |emu - ref|", "nets": [T.net_figures(n, dev) for n in T.NET_FIXTURES]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-accuracy", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bf16_tower.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(dev), "method": f"HIP events, {args.warmup} warm-up + {args.steps} timed forwards, gc disabled; "
           "fp32 then bf16 in one process", "shapes": {}}
    for shape in [s for s in args.shapes.split(",") if s]:
        g, l32, l16, in32, in16, desc = setup(shape, dev)
        with torch.no_grad():
            assert l16._bf16_path(g, in16[0], in16[1])
        ms32 = time_forward(l32, g, in32, args.steps, args.warmup)
        ms16 = time_forward(l16, g, in16, args.steps, args.warmup)
        ent = dict(desc, fp32_ms_per_step=ms32, bf16_ms_per_step=ms16, bf16_over_fp32=ms16 / ms32)
        res["shapes"][shape] = ent
        print(json.dumps({shape: ent}), flush=True)
        del g, l32, l16, in32, in16
        torch.cuda.empty_cache()
    if not args.no_accuracy:
        res["accuracy"] = accuracy(dev)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
