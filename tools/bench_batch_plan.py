#!/usr/bin/env python
"""What a FRESH batch costs before its first layer runs, on the route of today against the batch plan (pna_batch_plan_i32; knob
PNA_AMD_BATCH_PLAN_ROWS covering the batch), in ONE process on one box, a different pre-generated batch every step:

  (a) prepare_*: Graph.collate_flat(train=True, avg_d=...) from edge arrays resident on the device and host-side counts, then everything
      the first training forward and backward still ask the graph for -- heavy_schedule, work_items, edge_ids32, snorm_n, degree_scalers,
      nets._readout_offsets, autograd._transposed_whole_rows and the transposed edges' CSR positions -- on
        zinc_128    128 ZINC-shaped molecules (pna_amd.synth.molecule_batch),
        hiv_2048    2 048 MolHIV-shaped molecules (tools/bench_net_ends.py's batch),
        cifar_128   128 CIFAR10-superpixel-shaped graphs (100 .. 150 nodes, 8 in-edges a node).
      Milliseconds, kernel launches per batch (rocprofv3 --kernel-trace --stats of fresh child processes, the difference between a long
      and a short run) and host synchronisations per batch (torch.cuda.set_sync_debug_mode: every blocking copy either way, so the
      host-to-device copies of the count tables are in it for both routes).
  (b) net_zinc / net_hiv: one training step (collate_flat + forward + loss + backward + Adam) of PNANet on 128 ZINC-shaped molecules and
      of PNANetHIV on 2 048 MolHIV-shaped ones with the other one-call knobs on for both routes.

Every step is timed once (host clock around the step and a device synchronisation); the two routes alternate step by step, so drift hits
both; the garbage collector is off.  Reported: the median of 3 blocks of 20 steps after 5 warm-up steps, the blocks' own medians and
their spread -- the margin a difference has to exceed.

    python tools/bench_batch_plan.py            # writes profiles/batch_plan.json
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
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_small_train import timed  # noqa: E402
from pna_amd import autograd as AG, functional as PF, graph as G, nets  # noqa: E402
from pna_amd.graph import Graph  # noqa: E402
from pna_amd.synth import molecule_batch  # noqa: E402

AGG, SCA = "mean max min std", "identity amplification attenuation"
PREPARE = ("prepare_zinc_128", "prepare_hiv_2048", "prepare_cifar_128")
NETS = ("net_zinc", "net_hiv")
KNOB_ON = 1 << 30
N_BATCHES = 8
AVG_LOG = 1.1


def _local(src, dst, sizes):
    """A batch of pna_amd.synth (global ids, members one after the other) as local ids + edge counts."""
    sz = torch.tensor(sizes)
    member = torch.repeat_interleave(torch.arange(len(sizes)), sz)[src]
    off = (sz.cumsum(0) - sz)[member]
    return src - off, dst - off, torch.bincount(member, minlength=len(sizes)).tolist(), list(sizes)


def _superpixels(n_graphs, seed):
    rng = np.random.default_rng(seed)
    sizes = rng.integers(100, 151, n_graphs)
    srcs, dsts = [], []
    for n in sizes:
        d = np.repeat(np.arange(n), 8)
        s = (d + rng.integers(1, n, d.size)) % n                      # eight in-neighbours a node, never the node itself
        order = rng.permutation(d.size)
        srcs.append(s[order])
        dsts.append(d[order])
    return (torch.from_numpy(np.concatenate(srcs)), torch.from_numpy(np.concatenate(dsts)), [8 * int(n) for n in sizes], [int(n) for n in sizes])


def batches(shape, dev, n=N_BATCHES):
    """n different batches of one shape: (src_local, dst_local) as int32 on the device, (edge_counts, num_nodes) as host lists."""
    out = []
    for i in range(n):
        if shape == "zinc_128":
            b = _local(*molecule_batch(128, seed=41 + i))
        elif shape == "hiv_2048":
            b = _local(*molecule_batch(2048, mean_nodes=25.5, sd_nodes=12, lo=6, hi=222, seed=41 + i, lognormal=True))
        else:
            b = _superpixels(128, 41 + i)
        out.append((b[0].to(torch.int32).to(dev), b[1].to(torch.int32).to(dev), b[2], b[3]))
    return out


def prepare(b, dev, with_edges=True):
    """The batch's Graph with every array of a first training forward and backward built."""
    g = Graph.collate_flat(b[0], b[1], b[2], b[3], device=dev, train=True, avg_d=AVG_LOG)
    g.heavy_schedule()
    g.work_items()
    g.snorm_n()
    g.degree_scalers(AVG_LOG)
    nets._readout_offsets(g, g.device)
    AG._transposed_whole_rows(g)
    if with_edges:
        g.edge_ids32()
        gT = g._pna_amd_transposed
        if getattr(gT, "_pna_amd_pos_t", None) is None:               # (autograd._TowerTrainPlan's construction)
            gT._pna_amd_pos_t = gT.csr.eid.to(torch.int32).contiguous()
    return g


def setup(workload, dev):
    """-> (step function taking the step number, graphs, mean V, mean E)."""
    shape = workload.split("_", 1)[1] if workload.startswith("prepare") else {"net_zinc": "zinc_128", "net_hiv": "hiv_2048"}[workload]
    bs = batches(shape, dev)
    V = [sum(b[3]) for b in bs]
    E = [int(b[0].numel()) for b in bs]
    if workload.startswith("prepare"):
        return (lambda i: prepare(bs[i % len(bs)], dev)), len(bs[0][3]), statistics.mean(V), statistics.mean(E)
    PF.SMALL_TOWER_TRAIN_ROWS = PF.SMALL_TOWER_TRAIN_EDGE_ROWS = PF.SMALL_TRAIN_ROWS = PF.NET_ENDS_ROWS = PF.MLP_HEAD_ROWS = KNOB_ON
    torch.manual_seed(0)
    gen = torch.Generator().manual_seed(0)
    avg = {"log": torch.tensor(AVG_LOG)}
    if workload == "net_hiv":
        net = nets.PNANetHIV(dict(hidden_dim=80, out_dim=80, in_feat_dropout=0.0, dropout=0.3, L=4, readout="mean", batch_norm=True,
                                  residual=True, aggregators=AGG, scalers=SCA, avg_d=avg, posttrans_layers=1, device=dev)).to(dev).train()
        feats = [torch.stack([torch.randint(0, d, (v,), generator=gen) for d in nets.AtomEncoderStandIn.DIMS], dim=1).to(dev) for v in V]
        labels = [torch.randint(0, 2, (len(b[3]),), generator=gen) for b in bs]
    else:
        net = nets.PNANet(dict(num_atom_type=28, num_bond_type=4, hidden_dim=75, out_dim=70, in_feat_dropout=0.0, dropout=0.0, L=4, readout="sum",
                               graph_norm=True, batch_norm=True, residual=True, aggregators=AGG, scalers=SCA, avg_d=avg, towers=5,
                               divide_input_first=False, divide_input_last=True, edge_feat=True, edge_dim=50, pretrans_layers=1,
                               posttrans_layers=1, gru=False, device=dev)).to(dev).train()
        feats = [(torch.randint(0, 28, (v,), generator=gen).to(dev), torch.randint(0, 4, (e,), generator=gen).to(dev)) for v, e in zip(V, E)]
        labels = [torch.randn(len(b[3]), 1, generator=gen).to(dev) for b in bs]
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)

    def step(i):
        k = i % len(bs)
        b = bs[k]
        g = Graph.collate_flat(b[0], b[1], b[2], b[3], device=dev, train=True, avg_d=avg)
        opt.zero_grad()
        if workload == "net_hiv":
            out = net(g, feats[k])
        else:
            out = net(g, feats[k][0], feats[k][1], g.snorm_n(), None)
        net.loss(out, labels[k]).backward()
        opt.step()
    return step, len(bs[0][3]), statistics.mean(V), statistics.mean(E)


def syncs_per_step(step, n=4):
    """Blocking host <-> device operations of one step, counted by torch's sync debug mode (a warning each)."""
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            for i in range(n):
                step(i)
        return sum("synchroniz" in str(x.message) for x in w) / n
    finally:
        torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()


def measure(workload, dev, steps, warmup, blocks):
    step, graphs, V, E = setup(workload, dev)
    knobs = {"route_of_today": 0, "batch_plan": KNOB_ON}
    times = {k: [] for k in knobs}
    gc.disable()
    try:
        for i in range(warmup + blocks * steps):
            for name, knob in knobs.items():                    # the routes alternate step by step
                G.BATCH_PLAN_ROWS = knob
                t = timed(lambda: step(i))
                if i >= warmup:
                    times[name].append(t)
        ent = {"graphs": graphs, "mean_V": V, "mean_E": E, "different_batches": N_BATCHES}
        for name, knob in knobs.items():
            G.BATCH_PLAN_ROWS = knob
            meds = [statistics.median(times[name][r * steps:(r + 1) * steps]) for r in range(blocks)]
            ent[name] = {"median_ms": statistics.median(meds), "block_median_ms": meds, "block_spread_ms": max(meds) - min(meds),
                         "min_ms": min(times[name]), "max_ms": max(times[name]), "steps": len(times[name]),
                         "host_synchronisations_per_step": syncs_per_step(step)}
    finally:
        gc.enable()
        G.BATCH_PLAN_ROWS = 0
    spread = max(ent[k]["block_spread_ms"] for k in knobs)
    ent["margin_ms"] = spread
    ent["plan_over_today"] = ent["batch_plan"]["median_ms"] / ent["route_of_today"]["median_ms"]
    ent["plan_loses_by_more_than_the_spread"] = ent["batch_plan"]["median_ms"] > ent["route_of_today"]["median_ms"] + spread
    ent["plan_wins_by_more_than_the_spread"] = ent["batch_plan"]["median_ms"] < ent["route_of_today"]["median_ms"] - spread
    return ent


def child(workload, knob, steps):
    dev = torch.device("cuda:0")
    step, _, _, _ = setup(workload, dev)
    G.BATCH_PLAN_ROWS = KNOB_ON if knob else 0
    for i in range(steps):
        step(i)
    torch.cuda.synchronize()


def _trace_rows(workload, knob, steps):
    d = tempfile.mkdtemp(prefix="plan_trace_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "bp", "--",
           sys.executable, os.path.abspath(__file__), "--child", workload, "--knob", str(knob), "--steps", str(steps)]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        files = glob.glob(os.path.join(d, "**", "bp_kernel_stats.csv"), recursive=True)
        if r.returncode != 0 or not files:
            raise RuntimeError(f"rocprofv3 rc={r.returncode}: {r.stderr[-400:]}")
        return {row["Name"]: (int(row["Calls"]), float(row["TotalDurationNs"])) for row in csv.DictReader(open(files[0]))}
    finally:
        shutil.rmtree(d, ignore_errors=True)


def trace(workload, knob, short=2, long=10):
    """Launches per step and the per-kernel split of the device time: the difference between the kernel statistics of a child that runs
    `long` steps and one that runs `short` (what the set-up launches cancel out of)."""
    if shutil.which("rocprofv3") is None:
        return {"error": "rocprofv3 not found"}
    try:
        a, b = _trace_rows(workload, knob, short), _trace_rows(workload, knob, long)
    except (RuntimeError, subprocess.TimeoutExpired) as ex:
        return {"error": str(ex)}
    n = long - short
    rows = [(k, (b[k][0] - a.get(k, (0, 0.0))[0]) / n, (b[k][1] - a.get(k, (0, 0.0))[1]) / n / 1e3) for k in b]
    rows = [r for r in rows if r[1] > 0]
    top = sorted(rows, key=lambda x: -x[2])[:6]
    return {"steps": n, "launches_per_step": sum(r[1] for r in rows), "kernel_us_per_step": sum(r[2] for r in rows),
            "top_kernels": [{"name": k[:80], "calls_per_step": c, "us_per_step": t} for k, c, t in top]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--workloads", default=",".join(PREPARE + NETS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_plan.json"))
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--child", default=None)
    ap.add_argument("--knob", type=int, default=0)
    args = ap.parse_args()
    if args.child:
        child(args.child, args.knob, args.steps)
        return
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(dev),
           "method": "one process; a different pre-generated batch every step; garbage collector off; wall clock per step with a device "
                     f"synchronisation, every step timed once, the routes alternating; medians of {args.blocks} blocks of {args.steps} steps "
                     f"after {args.warmup} warm-up steps, the spread of the block medians as the margin; launches from rocprofv3 --kernel-trace "
                     "--stats of fresh child processes (prepare_* only); host synchronisations from torch.cuda.set_sync_debug_mode",
           "workloads": {}}
    for w in args.workloads.split(","):
        ent = measure(w, dev, args.steps, args.warmup, args.blocks)
        if not args.no_trace and w.startswith("prepare"):
            ent["trace"] = {"route_of_today": trace(w, 0), "batch_plan": trace(w, 1)}
        res["workloads"][w] = ent
        print(w, json.dumps({k: v for k, v in ent.items() if k != "trace"}), flush=True)
        if "trace" in ent:
            print(w, "launches per step:", {k: v.get("launches_per_step", v.get("error")) for k, v in ent["trace"].items()}, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
