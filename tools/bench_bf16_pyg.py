#!/usr/bin/env python
"""Same-box timing of the fp32 and the bf16 forward (inference) of the PyG front end: PNAConv, PNAConvSimple.

    python tools/bench_bf16_pyg.py [--shapes molhiv,zinc,big,big_deep,zinc_deep] [--steps 20] [--warmup 5] [--out profiles/bf16_pyg.json]

Shapes:
  molhiv     the 2 048-graph MolHIV-shaped batch (pna_amd/synth.py::molecule_batch), PNAConvSimple 80 -> 80
  zinc       128 molecule graphs, PNAConv 75 -> 75 with 5 towers over the whole input and edge features that take 4 bond-type values
  big        PNAConv, one tower of F = 75, on the bench graph (powerlaw_graph, seed 1234): V = 1 M, E = 10 M
  big_deep   the same with pre_layers = 2: fp32 gathers both endpoint rows into an (E, 150) tensor for library GEMMs, bf16 runs
             pna_edge_mlp_bf16 on the node-level terms of the first Linear
  zinc_deep  the zinc batch with pre_layers = 2
Every layer: the aggregators mean / min / max / std and the scalers identity / amplification / attenuation.  Method (DESIGN.md section
6): HIP events around `steps` forwards after `warmup` ones, gc disabled around the timed steps; fp32 first, then bf16, in one process.
The last bf16 output is compared with the fp32 one on a sample of rows (largest difference over the largest fp32 magnitude)."""
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

AGGS, SCALERS = ["mean", "min", "max", "std"], ["identity", "amplification", "attenuation"]
SHAPES = ("molhiv", "zinc", "big", "big_deep", "zinc_deep")


def setup(shape, dev):
    """-> (fp32 layer, bf16 layer, (x, edge_index, edge_attr) in fp32, the same in bf16, description)"""
    from pna_amd.pytorch_geometric import PNAConv, PNAConvSimple
    from pna_amd.synth import molecule_batch, powerlaw_graph
    torch.manual_seed(0)
    pre_layers, ed, towers = 2 if shape.endswith("_deep") else 1, 0, 1
    if shape.startswith("big"):
        V, hidden = 1_000_000, 75
        src, dst = powerlaw_graph(V, 10_000_000, seed=1234, device=dev)
    elif shape == "molhiv":
        src, dst, sizes = molecule_batch(2048, mean_nodes=25.5, sd_nodes=12, lo=6, hi=222, seed=41, lognormal=True)
        V, hidden = int(sum(sizes)), 80
    else:
        src, dst, sizes = molecule_batch(128, seed=41)
        V, hidden, ed, towers = int(sum(sizes)), 75, 50, 5
    ei = torch.stack([torch.as_tensor(src), torch.as_tensor(dst)]).long().to(dev)
    E = ei.shape[1]
    hist = torch.bincount(torch.bincount(ei[1], minlength=V))
    if shape == "molhiv":
        layer = PNAConvSimple(hidden, hidden, AGGS, SCALERS, hist)
    else:
        layer = PNAConv(hidden, hidden, AGGS, SCALERS, hist, edge_dim=ed or None, towers=towers, pre_layers=pre_layers)
    layer = layer.to(dev).eval()
    x = torch.randn(V, hidden, device=dev)
    ea = None
    if ed:
        table = torch.randn(4, ed, device=dev)
        ea = table[torch.randint(0, 4, (E,), device=dev)]
    bf = lambda t: None if t is None else t.to(torch.bfloat16)   # noqa: E731
    desc = {"layer": type(layer).__name__, "V": V, "E": E, "hidden": hidden, "towers": towers, "edge_dim": ed, "pre_layers": pre_layers}
    return layer, copy.deepcopy(layer).to(torch.bfloat16), (x, ei, ea), (bf(x), ei, bf(ea)), desc


def time_forward(layer, inputs, steps, warmup):
    with torch.no_grad():
        for _ in range(warmup):
            layer(*inputs)
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        gc.disable()
        try:
            t0.record()
            for _ in range(steps):
                out = layer(*inputs)
            t1.record()
            torch.cuda.synchronize()
        finally:
            gc.enable()
    return t0.elapsed_time(t1) / steps, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bf16_pyg.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(dev), "method": f"HIP events, {args.warmup} warm-up + {args.steps} timed forwards, gc disabled; "
           "fp32 then bf16 in one process", "shapes": {}}
    for shape in [s for s in args.shapes.split(",") if s]:
        l32, l16, in32, in16, desc = setup(shape, dev)
        with torch.no_grad():
            assert l16._bf16_path(in16[0], in16[2]) if desc["layer"] == "PNAConv" else l16._bf16_path(in16[0])
        ms32, out32 = time_forward(l32, in32, args.steps, args.warmup)
        ms16, out16 = time_forward(l16, in16, args.steps, args.warmup)
        rows = torch.linspace(0, desc["V"] - 1, 4096, device=dev).long()
        diff = float((out16[rows].float() - out32[rows]).abs().max() / out32[rows].abs().max())
        ent = dict(desc, fp32_ms_per_step=ms32, bf16_ms_per_step=ms16, bf16_over_fp32=ms16 / ms32, sampled_max_diff_over_max_fp32=diff)
        res["shapes"][shape] = ent
        print(json.dumps({shape: ent}), flush=True)
        del l32, l16, in32, in16, out32, out16
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
