#!/usr/bin/env python
"""The two ends of the molecule nets -- the atom encoder / atom-type embedding and the per-graph readout -- on the one-call route
(autograd.EmbedSumFn / ReadoutFn: pna_embed_sum_*_f32, pna_readout_*_f32; knob PNA_AMD_NET_ENDS_ROWS covering the batch) against the
route they would replace (knob 0: nine index_select + adds with one-hot GEMM backwards; the generic aggregate over the readout graph),
in ONE process on one box:

  * hiv_2048: the 2 048-graph MolHIV-shaped batch of tools/bench_small_train.py -- the nine-table encoder at width 80, the mean readout
    at width 80, and the whole PNANetHIV training step (4 layers, hidden 80, Adam);
  * zinc_128: a 128-graph ZINC-shaped batch -- the single atom-type table (28 x 70), the sum readout at width 70, and the same net.

Each piece is forward + backward; every step is timed once (host clock around the step and a device synchronisation); the two routes
alternate step by step, so drift hits both.  Launches per step come from a fresh child process of this tool's own under
`rocprofv3 --kernel-trace --stats` (no counters in that run), one pair of children per workload, piece and route.

    python tools/bench_net_ends.py            # writes profiles/net_ends.json
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
from bench_small_train import timed  # noqa: E402
from pna_amd import Graph, functional as PF, nets  # noqa: E402
from pna_amd.synth import molecule_batch  # noqa: E402

AGG, SCA = "mean max min std", "identity amplification attenuation"
WORKLOADS = ("hiv_2048", "zinc_128")
PIECES = ("encoder", "readout", "net")
KNOB_ON = 1 << 30


def setup(workload, piece, dev):
    """-> (step function, V, E, graphs)."""
    if workload == "hiv_2048":
        src, dst, sizes = molecule_batch(2048, mean_nodes=25.5, sd_nodes=12, lo=6, hi=222, seed=41, lognormal=True)
        width, op = 80, "mean"
    else:
        src, dst, sizes = molecule_batch(128, seed=41)
        width, op = 70, "sum"
    V, E = sum(sizes), src.numel()
    g = Graph(src, dst, V, sizes).to(dev)
    torch.manual_seed(0)
    gen = torch.Generator().manual_seed(0)
    atoms = torch.stack([torch.randint(0, d, (V,), generator=gen) for d in nets.AtomEncoderStandIn.DIMS], dim=1).to(dev)
    if piece == "encoder":
        enc = nets.AtomEncoderStandIn(width).to(dev) if workload == "hiv_2048" else torch.nn.Embedding(28, width).to(dev)
        idx = atoms if workload == "hiv_2048" else (atoms[:, 0] % 28).contiguous()
        R = torch.randn(V, width, device=dev)

        def step():
            enc.zero_grad(set_to_none=True)
            out = enc(idx) if workload == "hiv_2048" else nets.embed(enc, idx)
            (out * R).sum().backward()
    elif piece == "readout":
        h = torch.randn(V, width, device=dev).requires_grad_(True)
        R = torch.randn(len(sizes), width, device=dev)

        def step():
            h.grad = None
            (nets.readout_nodes(g, h, op) * R).sum().backward()
    else:
        avg = {"log": torch.log(g.in_degrees().double() + 1).mean().float().cpu()}
        net = nets.PNANetHIV(dict(hidden_dim=80, out_dim=80, in_feat_dropout=0.0, dropout=0.3, L=4, readout="mean", batch_norm=True,
                                  residual=True, aggregators=AGG, scalers=SCA, avg_d=avg, posttrans_layers=1, device=dev)).to(dev).train()
        labels = torch.randint(0, 2, (len(sizes),), generator=gen)
        opt = torch.optim.Adam(net.parameters(), lr=1e-3)

        def step():
            opt.zero_grad()
            net.loss(net(g, atoms), labels).backward()
            opt.step()
    return step, V, E, len(sizes)


def measure(workload, piece, dev, steps, warmup):
    step, V, E, graphs = setup(workload, piece, dev)
    knobs = {"parent_route": 0, "one_call_route": KNOB_ON}
    times = {k: [] for k in knobs}
    gc.disable()
    try:
        for i in range(warmup + steps):
            for name, knob in knobs.items():                    # the routes alternate step by step
                PF.NET_ENDS_ROWS = knob
                t = timed(step)
                if i >= warmup:
                    times[name].append(t)
    finally:
        gc.enable()
        PF.NET_ENDS_ROWS = 0
    ent = {"graphs": graphs, "V": V, "E": E}
    for name, ts in times.items():
        ent[name] = {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "steps": len(ts)}
    ent["one_call_over_parent"] = ent["one_call_route"]["median_ms"] / ent["parent_route"]["median_ms"]
    return ent


def child(workload, piece, knob, steps):
    dev = torch.device("cuda:0")
    step, _, _, _ = setup(workload, piece, dev)
    PF.NET_ENDS_ROWS = KNOB_ON if knob else 0
    for _ in range(steps):
        step()
    torch.cuda.synchronize()


def _trace_rows(workload, piece, knob, steps):
    d = tempfile.mkdtemp(prefix="net_ends_trace_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "ne", "--",
           sys.executable, os.path.abspath(__file__), "--child", workload, "--piece", piece, "--knob", str(knob), "--steps", str(steps)]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        files = glob.glob(os.path.join(d, "**", "ne_kernel_stats.csv"), recursive=True)
        if r.returncode != 0 or not files:
            raise RuntimeError(f"rocprofv3 rc={r.returncode}: {r.stderr[-400:]}")
        return {row["Name"]: (int(row["Calls"]), float(row["TotalDurationNs"])) for row in csv.DictReader(open(files[0]))}
    finally:
        shutil.rmtree(d, ignore_errors=True)


def trace(workload, piece, knob, short=3, long=13):
    """Launches per step and the per-kernel split of the device time: the difference between the kernel statistics of a child that runs
    `long` steps and one that runs `short` (what the set-up launches cancels out of)."""
    if shutil.which("rocprofv3") is None:
        return {"error": "rocprofv3 not found"}
    try:
        a, b = _trace_rows(workload, piece, knob, short), _trace_rows(workload, piece, knob, long)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "net_ends.json"))
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--child", default=None)
    ap.add_argument("--piece", default="net")
    ap.add_argument("--knob", type=int, default=0)
    args = ap.parse_args()
    if args.child:
        child(args.child, args.piece, args.knob, args.steps)
        return
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(dev),
           "method": "one process; wall clock per step with a device synchronisation, every step timed once, the routes alternating; "
                     f"{args.steps} steps after {args.warmup} warm-up steps; launches from rocprofv3 --kernel-trace --stats of a child process",
           "workloads": {}}
    for w in args.workloads.split(","):
        res["workloads"][w] = {}
        for piece in PIECES:
            ent = measure(w, piece, dev, args.steps, args.warmup)
            if not args.no_trace:
                ent["trace"] = {"parent_route": trace(w, piece, 0), "one_call_route": trace(w, piece, 1)}
            res["workloads"][w][piece] = ent
            print(w, piece, json.dumps({k: v for k, v in ent.items() if k != "trace"}), flush=True)
            if not args.no_trace:
                print(w, piece, "launches per step:", {k: v.get("launches_per_step", v.get("error")) for k, v in ent["trace"].items()}, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
