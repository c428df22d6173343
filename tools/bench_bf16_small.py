#!/usr/bin/env python
"""Same-box timing of the bf16 one-call tower layer (pna_tower_layer_bf16) against the multi-launch bf16 path and the fp32 layer,
eager and as a hipGraph replay.

    python tools/bench_bf16_small.py [--shapes zinc,zinc_bonds,molhiv,molhiv_simple,zinc_simple,net_zinc] [--steps 50] [--warmup 10] [--rounds 3]
                                     [--out profiles/bf16_small.json]

Shapes (the first three are those of tools/bench_bf16_tower.py):
  zinc           PNALayer, 128 molecule graphs, hidden 75, 5 towers over the whole input
  zinc_bonds     the same with edge features that are an embedding of 4 bond types (edge_dim 50), types registered on the graph as
                 PNANet does, so that captures take the edge-type table too
  molhiv         PNALayer, the 2 048-graph MolHIV-shaped batch, hidden 80, 8 towers over slices of the input
  molhiv_simple  PNASimpleLayer, hidden 80, on the same batch
  zinc_simple    PNASimpleLayer, hidden 80, on the 128-molecule batch
  net_zinc       a 4-layer PNANet (hidden 75, 5 towers, bond types) on the 128-molecule batch, atoms and bonds as inputs
Legs: fp32 eager, fp32 replay, bf16 multi-launch eager (BF16_SMALL_ROWS = 0: the path before the one-call kernel), bf16 multi-launch
replay, bf16 one-call eager, bf16 one-call replay.  Method: one process per shape; every leg is warmed up (and
its replay captured) first, then `rounds` rounds time every leg in turn -- HIP events around `steps` calls, gc disabled -- so the
spread of each leg over the rounds is on record.  `one_call_launches` counts the calls of ops.tower_layer_bf16 per forward."""
import argparse
import copy
import gc
import json
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

AGGS, SCALERS = "mean max min std", "identity amplification attenuation"
SHAPES = ("zinc", "zinc_bonds", "molhiv", "molhiv_simple", "zinc_simple", "net_zinc")
BF = torch.bfloat16


def setup(shape, dev):
    """-> ({precision: (callable(*inputs), inputs, prepare())}, description); prepare() runs before a leg of that precision."""
    from pna_amd.dgl.pna_layer import PNALayer, PNASimpleLayer
    from pna_amd.graph import Graph
    from pna_amd.nets import PNANet
    from pna_amd.synth import molecule_batch
    torch.manual_seed(0)
    if shape.startswith("molhiv"):
        src, dst, sizes = molecule_batch(2048, mean_nodes=25.5, sd_nodes=12, lo=6, hi=222, seed=41, lognormal=True)
    else:
        src, dst, sizes = molecule_batch(128, seed=41)
    V, E = int(sum(sizes)), src.numel()
    g = Graph(src, dst, V, sizes).to(dev)
    sn = g.snorm_n()
    avg_log = torch.log(g.in_degrees().double() + 1).mean().float()
    desc = {"V": V, "E": E, "max_in_degree": int(g.in_degrees().max())}
    nothing = lambda: None   # noqa: E731

    def randomize(m):
        with torch.no_grad():
            for p in m.parameters():
                if p.dim() == 2:
                    p.copy_(torch.randn_like(p) / p.shape[1] ** 0.5)
        return m

    if shape == "net_zinc":
        net = randomize(PNANet(dict(num_atom_type=28, num_bond_type=4, hidden_dim=75, out_dim=75, in_feat_dropout=0.0, dropout=0.0, L=4,
                                    readout="sum", graph_norm=True, batch_norm=True, residual=True, aggregators=AGGS, scalers=SCALERS,
                                    avg_d={"log": avg_log}, towers=5, divide_input_first=False, divide_input_last=True, edge_feat=True,
                                    edge_dim=50, pretrans_layers=1, posttrans_layers=1, gru=False, device=dev)).to(dev).eval())
        net16 = copy.deepcopy(net).to(BF)
        atoms, bonds = torch.randint(0, 28, (V,), device=dev), torch.randint(0, 4, (E,), device=dev)
        sn16 = sn.to(BF)
        desc.update(hidden=75, towers=5, layers=4, edge_dim=50)
        return {"fp32": (lambda a, b: net(g, a, b, sn, None), (atoms, bonds), nothing),
                "bf16": (lambda a, b: net16(g, a, b, sn16, None), (atoms, bonds), nothing)}, desc
    if shape.endswith("_simple"):
        layer = randomize(PNASimpleLayer(80, 80, AGGS, SCALERS, {"log": avg_log}, 0.0, True, True).to(dev).eval())
        layer16 = copy.deepcopy(layer).to(BF)
        h = torch.randn(V, 80, device=dev)
        desc.update(hidden=80)
        return {"fp32": (lambda x: layer(g, x), (h,), nothing), "bf16": (lambda x: layer16(g, x), (h.to(BF),), nothing)}, desc
    hidden, towers, divide, ed = (80, 8, True, 0) if shape == "molhiv" else (75, 5, False, 50 if shape == "zinc_bonds" else 0)
    layer = randomize(PNALayer(hidden, hidden, AGGS, SCALERS, {"log": avg_log}, 0.0, True, True, towers=towers, divide_input=divide,
                               residual=True, edge_features=ed > 0, edge_dim=ed).to(dev).eval())
    layer16 = copy.deepcopy(layer).to(BF)
    h = torch.randn(V, hidden, device=dev)
    desc.update(hidden=hidden, towers=towers, divide_input=divide, edge_dim=ed)
    e = e16 = None
    prep32 = prep16 = nothing
    if ed:
        table, types = torch.randn(4, ed, device=dev), torch.randint(0, 4, (E,), device=dev)
        e, table16 = table[types], table.to(BF)
        e16 = table16[types]
        prep32 = lambda: g.register_edge_types(e, types, table)          # noqa: E731  (one slot per graph: the leg's own tensor)
        prep16 = lambda: g.register_edge_types(e16, types, table16)      # noqa: E731
    sn16 = sn.to(BF)
    return {"fp32": (lambda x: layer(g, x, e, sn), (h,), prep32), "bf16": (lambda x: layer16(g, x, e16, sn16), (h.to(BF),), prep16)}, desc


def timed(fn, inputs, steps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    gc.disable()
    try:
        t0.record()
        for _ in range(steps):
            fn(*inputs)
        t1.record()
        torch.cuda.synchronize()
    finally:
        gc.enable()
    return t0.elapsed_time(t1) / steps


def run_shape(shape, steps, warmup, rounds):
    from pna_amd import functional as PF
    from pna_amd import ops
    from pna_amd.capture import GraphedForward
    dev = torch.device("cuda:0")
    models, desc = setup(shape, dev)
    calls = [0]
    inner = ops.tower_layer_bf16
    ops.tower_layer_bf16 = lambda *a, **k: (calls.__setitem__(0, calls[0] + 1), inner(*a, **k))[1]
    legs = [("fp32_eager", "fp32", None, False), ("fp32_replay", "fp32", None, True),
            ("bf16_multi_eager", "bf16", 0, False), ("bf16_multi_replay", "bf16", 0, True),
            ("bf16_one_eager", "bf16", 1 << 30, False), ("bf16_one_replay", "bf16", 1 << 30, True)]
    default_rows = PF.BF16_SMALL_ROWS
    runners, launches = {}, {}
    with torch.no_grad():
        for name, prec, rows, replay in legs:
            fn, inputs, prepare = models[prec]
            PF.BF16_SMALL_ROWS = default_rows if rows is None else rows
            prepare()
            for _ in range(warmup):
                fn(*inputs)
            calls[0] = 0
            fn(*inputs)
            launches[name] = calls[0]
            runners[name] = GraphedForward(fn, *inputs, alias_inputs=True) if replay else fn
            torch.cuda.synchronize()
        ms = {name: [] for name, *_ in legs}
        for _ in range(rounds):
            for name, prec, rows, replay in legs:
                fn, inputs, prepare = models[prec]
                PF.BF16_SMALL_ROWS = default_rows if rows is None else rows
                prepare()
                for _ in range(warmup):
                    runners[name](*inputs)
                torch.cuda.synchronize()
                ms[name].append(timed(runners[name], inputs, steps))
    PF.BF16_SMALL_ROWS = default_rows
    out = dict(desc, default_rows=default_rows, one_call_launches=launches)
    for name, v in ms.items():
        out[name] = {"ms": sorted(v)[len(v) // 2], "min": min(v), "max": max(v), "rounds": v}
    one, multi = out["bf16_one_eager"], out["bf16_multi_eager"]
    margin = max(one["max"] - one["min"], multi["max"] - multi["min"])
    out["one_call_not_slower"] = one["ms"] <= multi["ms"] + margin
    out["margin_ms"] = margin
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bf16_small.json"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        print("RESULT " + json.dumps(run_shape(args.child, args.steps, args.warmup, args.rounds)), flush=True)
        return
    res = {"method": f"HIP events, one process per shape, {args.rounds} rounds over all legs in turn, {args.warmup} warm-up + {args.steps} "
                     "timed calls per leg and round, gc disabled; ms = median over the rounds", "shapes": {}}
    for shape in [s for s in args.shapes.split(",") if s]:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", shape, "--steps", str(args.steps), "--warmup", str(args.warmup),
                            "--rounds", str(args.rounds)], capture_output=True, text=True, timeout=600)
        line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            print(p.stdout[-2000:], p.stderr[-4000:], file=sys.stderr)
            raise SystemExit(f"{shape}: the child process failed ({p.returncode}); nothing further is started")
        res["shapes"][shape] = json.loads(line[0][len("RESULT "):])
        print(json.dumps({shape: {k: (v["ms"] if isinstance(v, dict) and "ms" in v else v) for k, v in res["shapes"][shape].items()}}), flush=True)
    import torch.cuda
    res["device"] = torch.cuda.get_device_name(0)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
