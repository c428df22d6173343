"""Host cost of the one-kernel layer's drivers (pna_amd/functional.py: FusedDegreeCall / FusedTowerCall / FusedMultiTowerCall, DESIGN.md
4.8.9): what a forward pays in the interpreter before and between its launches.  The two tower calls are constructed on every forward.

    python tools/bench_fused_call_host.py [--number 300] [--repeat 5] [--out FILE]

Times with timeit, each warm (plan, weight images, tile orders and the allocator's blocks in place): the construction of each of the three
calls, a set_spare(True) / set_spare(False) pair of each (the warm hit of the tile-order binding, in front of every launch), and one eager
forward of a 3-tower divide_input=False PNALayer (launches are asynchronous: the loop times the host, the device is synchronised outside
it).  Per entry the median and the spread (max - min) of the repeats, in microseconds per call.  The graph is the one of
tests/test_gpu_fused_call_blocks.py (3000 nodes: eight degree groups, 119 rest rows).  Only names that the drivers have had since they
exist are used, so the same file run from a checkout of an earlier commit gives that commit's numbers (profiles/fused_call_host.json
holds both)."""
import argparse
import json
import os
import statistics
import sys
import timeit

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

AGGS, SCALERS = "mean max min std", "identity amplification attenuation"
V = 3000


def entries(dev):
    from pna_amd import Graph, degree_groups as DG, functional as PF
    from pna_amd.dgl import pna_layer as PL
    DG.ENABLED, DG.MIN_ROWS, DG.MIN_OUT, DG.FUSED, PF.SMALL_TOWER_ROWS, PF.SMALL_SIMPLE_ROWS = True, 1, 1, True, 0, 0
    rng = np.random.default_rng(7)
    src, dst = rng.integers(0, V, 12000), rng.integers(0, V, 12000)
    src, dst = np.concatenate([src, rng.integers(0, V, 300)]), np.concatenate([dst, np.full(300, 1500)])
    g = Graph(torch.from_numpy(src).to(dev), torch.from_numpy(dst).to(dev), V)
    avg = {"log": torch.tensor(1.6)}
    torch.manual_seed(0)
    simple = PL.PNASimpleLayer(75, 75, AGGS, SCALERS, avg, 0.0, True, True).to(dev).eval()
    one = PL.PNALayer(75, 75, AGGS, SCALERS, avg, 0.0, True, True, towers=1, divide_input=False, residual=True).to(dev).eval()
    multi = PL.PNALayer(64, 48, AGGS, SCALERS, avg, 0.0, True, True, towers=3, divide_input=False, residual=False).to(dev).eval()
    h75, h64 = torch.randn(V, 80, device=dev)[:, :75], torch.randn(V, 64, device=dev)
    snorm = torch.rand(V, 1, device=dev) + 0.5
    Wpad, bpad = PL._projection_cache_padded(one.towers[0], 75, PF.tower_projection_pitch(75))
    x_cat = PF.linear_act(h75, Wpad, bpad)
    Wt, _ = PL._projection_cache_padded_multi(list(multi.towers), 64, PF.tower_projection_pitch(64))
    x_src = torch.mm(h64, Wt)
    assert DG.fused_applies(g, h75, 75, 75) and PF.tower_layer_degree_fused_applies(one, g, h75) and PF.tower_layer_degree_fused_applies(multi, g, h64)
    ctors = {
        "FusedDegreeCall": lambda: PF.FusedDegreeCall(simple, g, h75, x=h75),
        "FusedTowerCall": lambda: PF.FusedTowerCall(one, g, h75, snorm, x_cat),
        "FusedMultiTowerCall": lambda: PF.FusedMultiTowerCall(multi, g, h64, snorm, x_src),
    }
    out = {f"construct {name}": fn for name, fn in ctors.items()}
    for name, fn in ctors.items():
        call = fn()

        def pair(call=call):
            call.set_spare(True)
            call.set_spare(False)
        out[f"set_spare pair {name}"] = pair
    out["eager 3-tower layer forward (host)"] = lambda: multi(g, h64, None, snorm)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--number", type=int, default=300)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {}
    with torch.no_grad():
        for name, fn in entries(dev).items():
            fn(), fn()
            us = []
            for _ in range(args.repeat):
                torch.cuda.synchronize()
                us.append(timeit.timeit(fn, number=args.number) / args.number * 1e6)
                torch.cuda.synchronize()
            res[name] = {"median_us": round(statistics.median(us), 3), "spread_us": round(max(us) - min(us), 3), "repeats_us": [round(u, 3) for u in us]}
            print(f"{name:45s} {res[name]['median_us']:9.3f} us  (spread {res[name]['spread_us']:.3f})", flush=True)
    out = {"number": args.number, "repeat": args.repeat, "host_us_per_call": res}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
