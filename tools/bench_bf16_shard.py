#!/usr/bin/env python
"""fp32 against bf16 sharded steps of PNASimpleLayer: two ranks on ONE GPU over gloo, both dtypes in the same process pair.

    python tools/bench_bf16_shard.py [--nodes 1000000] [--edges 10000000] [--feat 75] [--steps 10] [--warmup 3]
                                     [--out profiles/bf16_shard.json]

Graph: pna_amd/synth.py::powerlaw_graph(seed 1234), sharded by equal node counts.  fp32: features in the shard's resident
[local | halo] table at the dense pitch (the route bench.py takes with more than one GPU); bf16: features at a pitch of round8(F),
halo rows in a buffer of their own.  Reported per rank: the mean step time of both dtypes (host wall clock around
`steps` synchronised forwards after `warmup` ones, the ranks kept in step by the exchange itself) and the bytes a rank hands to the
collective per layer.  gloo STAGES DEVICE TENSORS THROUGH THE HOST: the exchange part of these times says nothing about a link
between GPUs; they compare the compute side (pack, two gather launches, contraction) only.  Nothing is asserted.
"""
import argparse
import copy
import json
import os
import socket
import sys
import time

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AGGS, SCALERS = "mean max min std", "identity amplification attenuation"


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _time(fn, steps, warmup, dev):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize(dev)
    dist.barrier()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) / steps * 1e3


def _worker(rank, world, port, a, out_path):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from pna_amd.dgl.pna_layer import PNASimpleLayer
        from pna_amd.shard import shard_graph
        from pna_amd.synth import powerlaw_graph
        V, E, F = a.nodes, a.edges, a.feat
        src, dst = powerlaw_graph(V, E, seed=1234, device=dev)
        gs = shard_graph(src, dst, V)
        avg_log = torch.log(torch.bincount(dst, minlength=V).double() + 1).mean().float()
        del src, dst
        torch.manual_seed(0)
        l32 = PNASimpleLayer(F, F, AGGS, SCALERS, {"log": avg_log}, 0.0, True, True).to(dev).eval()
        l16 = copy.deepcopy(l32).to(torch.bfloat16)
        n, P = gs.num_nodes, (F + 7) // 8 * 8
        h32 = gs.alloc_features(F)
        h32.copy_(torch.randn(n, F, device=dev, generator=torch.Generator(device=dev).manual_seed(3 + rank)))
        h16 = torch.zeros(n, P, dtype=torch.bfloat16, device=dev)[:, :F]
        h16.copy_(h32)
        with torch.no_grad():
            assert l16._bf16_path(gs, h16)
            ms32 = _time(lambda: l32(gs, h32), a.steps, a.warmup, dev)
            ms16 = _time(lambda: l16(gs, h16), a.steps, a.warmup, dev)
        n_send = sum(gs.send_splits)
        interior, boundary = gs.split_rows()
        res = {"rank": rank, "local_rows": n, "halo_rows": gs.n_halo, "rows_sent": n_send, "interior_rows": int(interior.numel()),
               "boundary_light_rows": int(boundary.numel()), "heavy_rows": gs.heavy_schedule().n_heavy,
               "fp32_ms_per_step": round(ms32, 4), "bf16_ms_per_step": round(ms16, 4),
               "fp32_wire_bytes_per_layer": n_send * F * 4, "bf16_wire_bytes_per_layer": n_send * P * 2}
        gathered = [None] * world
        dist.all_gather_object(gathered, res)
        if rank == 0:
            doc = {"tool": "tools/bench_bf16_shard.py", "world": world, "backend": "gloo, both ranks on one GPU",
                   "note": "gloo stages device tensors through the host: the times compare the compute side only, not a GPU-to-GPU exchange",
                   "nodes": V, "edges": E, "feat": F, "steps": a.steps, "warmup": a.warmup, "device": torch.cuda.get_device_name(dev),
                   "bf16_over_fp32_wire_bytes": round(res["bf16_wire_bytes_per_layer"] / max(1, res["fp32_wire_bytes_per_layer"]), 4),
                   "ranks": gathered}
            print("gloo stages device tensors through the host: these times show the compute side only")
            for r in gathered:
                print(f"rank {r['rank']}: fp32 {r['fp32_ms_per_step']} ms/step, bf16 {r['bf16_ms_per_step']} ms/step; wire bytes per layer "
                      f"fp32 {r['fp32_wire_bytes_per_layer']}, bf16 {r['bf16_wire_bytes_per_layer']}")
            os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
            with open(out_path, "w") as fh:
                json.dump(doc, fh, indent=1)
                fh.write("\n")
            print(json.dumps({k: v for k, v in doc.items() if k != "ranks"}))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--nodes", type=int, default=1_000_000)
    ap.add_argument("--edges", type=int, default=10_000_000)
    ap.add_argument("--feat", type=int, default=75)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bf16_shard.json"))
    a = ap.parse_args()
    mp.spawn(_worker, args=(2, _free_port(), a, a.out), nprocs=2, join=True)


if __name__ == "__main__":
    main()
