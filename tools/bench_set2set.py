#!/usr/bin/env python
"""The Set2Set graph readout (pna_amd.layers.Set2Set) on the one-call route (autograd.Set2SetFn: pna_set2set_fwd_f32 / _bwd_f32; knob
PNA_AMD_S2S_ROWS covering B N) against the route it would replace (knob 0: per round a one-step nn.LSTM, a batched matmul, a softmax, a
product, a sum and a concatenation, and autograd's backward of each), in ONE process on one box:

  * s2s_BxN:  layers.Set2Set(16) forward + backward (the input's and the four LSTM parameters' gradients), steps = N;
  * step_BxN: one training step of the README model built from the package (pytorch.gnn_framework.GNN: hidden 16, 4 towers, fixed, variable
              N / 2 layers, shared GRU): forward in train mode, the multitask loss, backward, Adam -- with PNA_AMD_DENSE_LAYER_ROWS,
              PNA_AMD_GRU_ROWS and PNA_AMD_S2S_ROWS all off against all on;
  at (B, N) = (16, 15), (64, 25), (16, 97): the dense-layer benchmark's shapes.

Every step is timed once (host clock around the step and a device synchronisation) with the garbage collector off; the two routes alternate
step by step, so drift hits both; `repeats` blocks of `steps` steps follow the warm-up and the spread of the blocks' medians is recorded
beside the overall median: a route "loses" where its median exceeds the other's by more than that spread.  The outputs of the two routes
are compared at the timed size.  Launches per step come from a fresh child process of this tool's own under `rocprofv3 --kernel-trace
--stats` (no counters in that run), one pair of children per traced workload and route.

    python tools/bench_set2set.py            # writes profiles/set2set.json
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
import types

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench_dense_layer as BD  # noqa: E402
from bench_small_train import timed  # noqa: E402
from pna_amd import functional as PF, layers  # noqa: E402
from pna_amd.pytorch.gnn_framework import GNN  # noqa: E402
from pna_amd.pytorch.pna.layer import PNALayer  # noqa: E402

SHAPES = BD.SHAPES
WORKLOADS = tuple(f"{kind}_{B}x{N}" for kind in ("s2s", "step") for B, N in SHAPES)
TRACED = ("s2s_16x15", "s2s_16x97", "step_16x15")
KNOB_ON = 1 << 30


def set_knobs(kind, on):
    PF.S2S_ROWS = KNOB_ON if on else 0
    if kind == "step":
        PF.DENSE_LAYER_ROWS = PF.GRU_ROWS = KNOB_ON if on else 0


def setup(workload, dev):
    """-> (step function returning the output, B, N)."""
    kind, shape = workload.split("_")
    B, N = (int(v) for v in shape.split("x"))
    torch.manual_seed(0)
    gen = torch.Generator().manual_seed(1)
    if kind == "s2s":
        m = layers.Set2Set(16, device=dev).train()
        x = torch.randn(B, N, 16, generator=gen).to(dev).requires_grad_(True)
        R = torch.randn(B, 32, generator=gen).to(dev)

        def step():
            m.zero_grad(set_to_none=True)
            x.grad = None
            out = m(x)
            (out * R).sum().backward()
            return out.detach()
        return step, B, N
    adj = BD._graphs(B, N, gen).to(dev)
    deg = adj.sum(-1)
    avg_d = {"log": torch.log(deg + 1).mean(), "lin": deg.mean()}                     # 0-dim device scalars
    conv = dict(aggregators=BD.AGG, scalers=BD.SCA, avg_d=avg_d, towers=4, self_loop=False, pretrans_layers=1, posttrans_layers=1)
    net = GNN(nfeat=2, nhid=16, nodes_out=3, graph_out=3, dropout=0.0, conv_layers=lambda a: a.shape[1] // 2, fc_layers=3,
              first_conv_descr=dict(layer_type=PNALayer, args=dict(conv, divide_input=False)),
              middle_conv_descr=types.SimpleNamespace(layer_type=PNALayer, args=dict(conv, divide_input=True)),
              final_activation="LeakyReLU", gru=True, fixed=True, variable=True, device=dev).to(dev).train()
    state0 = {k: v.detach().clone() for k, v in net.state_dict().items()}
    x = torch.randn(B, N, 2, generator=gen).to(dev)
    nl, gl = torch.randn(B, N, 3, generator=gen).to(dev), torch.randn(B, 3, generator=gen).to(dev)
    opt = torch.optim.Adam(net.parameters(), lr=0.003, weight_decay=1e-6)

    def step():
        net.load_state_dict(state0)                              # every timed step starts from the same parameters (both routes pay the copy)
        opt.zero_grad(set_to_none=True)
        nodes, graph = net(x, adj)
        loss = (F.mse_loss(nodes, nl) * 3 + F.mse_loss(graph, gl) * 3) / 6          # multitask_benchmark/util/util.py:51-66, mse
        loss.backward()
        opt.step()
        return torch.cat([nodes.detach().reshape(-1), graph.detach().reshape(-1)])
    return step, B, N


def measure(workload, dev, steps, warmup, repeats):
    kind = workload.split("_")[0]
    step, B, N = setup(workload, dev)
    routes = {"parent_route": False, "one_call_route": True}
    times = {k: [] for k in routes}
    outs = {}
    gc.disable()
    try:
        for i in range(warmup + repeats * steps):
            for name, on in routes.items():                      # the routes alternate step by step
                set_knobs(kind, on)
                out = [None]
                t = timed(lambda: out.__setitem__(0, step()))
                outs[name] = out[0]
                if i >= warmup:
                    times[name].append(t)
    finally:
        gc.enable()
        set_knobs("step", False)
    ent = {"B": B, "N": N, "rows": B * N}
    for name, ts in times.items():
        blocks = [statistics.median(ts[r * steps:(r + 1) * steps]) for r in range(repeats)]
        ent[name] = {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "steps": len(ts), "repeat_median_ms": blocks,
                     "repeat_spread_ms": max(blocks) - min(blocks)}
    spread = max(ent[k]["repeat_spread_ms"] for k in routes)
    ent["one_call_over_parent"] = ent["one_call_route"]["median_ms"] / ent["parent_route"]["median_ms"]
    ent["one_call_loses_by_more_than_the_spread"] = ent["one_call_route"]["median_ms"] > ent["parent_route"]["median_ms"] + spread
    ent["routes_max_abs_diff"] = float((outs["one_call_route"] - outs["parent_route"]).abs().max())
    ent["output_max_abs"] = float(outs["parent_route"].abs().max())
    return ent


def child(workload, knob, steps):
    dev = torch.device("cuda:0")
    step, _, _ = setup(workload, dev)
    set_knobs(workload.split("_")[0], bool(knob))
    for _ in range(steps):
        step()
    torch.cuda.synchronize()


def _trace_rows(workload, knob, steps):
    d = tempfile.mkdtemp(prefix="s2s_trace_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "s2s", "--",
           sys.executable, os.path.abspath(__file__), "--child", workload, "--knob", str(knob), "--steps", str(steps)]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        files = glob.glob(os.path.join(d, "**", "s2s_kernel_stats.csv"), recursive=True)
        if r.returncode != 0 or not files:
            raise RuntimeError(f"rocprofv3 rc={r.returncode}: {r.stderr[-400:]}")
        return {row["Name"]: (int(row["Calls"]), float(row["TotalDurationNs"])) for row in csv.DictReader(open(files[0]))}
    finally:
        shutil.rmtree(d, ignore_errors=True)


def trace(workload, knob, short=2, long=6):
    """Launches per step and the per-kernel split of the device time: the difference between the kernel statistics of a child that runs
    `long` steps and one that runs `short` (what the set-up launches cancels out of; bench_dense_layer.py's scheme)."""
    if shutil.which("rocprofv3") is None:
        return {"error": "rocprofv3 not found"}
    try:
        a, b = _trace_rows(workload, knob, short), _trace_rows(workload, knob, long)
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
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    ap.add_argument("--traced", default=",".join(TRACED))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "set2set.json"))
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--child", default=None)
    ap.add_argument("--knob", type=int, default=0)
    args = ap.parse_args()
    if args.child:
        child(args.child, args.knob, args.steps)
        return
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(dev),
           "method": "one process; wall clock per step with a device synchronisation, the garbage collector off, every step timed once, the "
                     f"routes alternating; {args.repeats} blocks of {args.steps} steps after {args.warmup} warm-up steps; repeat_spread_ms = the "
                     "range of the blocks' medians; launches from rocprofv3 --kernel-trace --stats of a child process (traced workloads only)",
           "workloads": {}}
    traced = set(args.traced.split(",")) if not args.no_trace else set()
    for w in args.workloads.split(","):
        ent = measure(w, dev, args.steps, args.warmup, args.repeats)
        if w in traced:
            ent["trace"] = {"parent_route": trace(w, 0), "one_call_route": trace(w, 1)}
            if any("error" in v for v in ent["trace"].values()):                       # a child that failed: start no further one
                traced = set()
        res["workloads"][w] = ent
        print(w, json.dumps({k: v for k, v in ent.items() if k != "trace"}), flush=True)
        if "trace" in ent:
            print(w, "launches per step:", {k: v.get("launches_per_step", v.get("error")) for k, v in ent["trace"].items()}, flush=True)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)      # (written after every workload: a later failure loses nothing)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
