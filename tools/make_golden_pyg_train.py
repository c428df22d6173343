#!/usr/bin/env python
"""Golden vectors of PNAConv's TRAINING step: runs the reference's `models/pytorch_geometric/pna.py` (unmodified, imported over
oracle/pyg_standin.py) through loss.backward() on the CPU, in float64 and in fp32, with loss = sum(out * R).  TEST INFRASTRUCTURE ONLY;
needs the reference checkout on sys.path the way oracle/make_golden_pyg.py does.
    python tools/make_golden_pyg_train.py        # writes tests/golden/pyg_conv_train_step.npz
Only the recorded arrays are kept: the inputs, the state dict, and per precision the output and every gradient.  The graph has two
nodes without in-edges (the PyG variant defines them: scalers.py:16-19, 26-29) and no repeated (source, destination) pair.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import pyg_standin  # noqa: E402

pyg_standin.install()
from models.pytorch_geometric.pna import PNAConv as RefConv  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "pyg_conv_train_step.npz")


def step(layer, x, ei, ea, R, dtype):
    layer = layer.to(dtype)
    layer.zero_grad()
    x = x.to(dtype).clone().requires_grad_(True)
    ea = ea.to(dtype).clone().requires_grad_(True)
    out = layer(x, ei, ea)
    (out * R.to(dtype)).sum().backward()
    res = {"out": out.detach(), "grad_x": x.grad, "grad_edge_attr": ea.grad}
    res.update({"grad/" + k: p.grad for k, p in layer.named_parameters()})
    return {k: v.clone().numpy() for k, v in res.items()}


def main(seed=21, N=50, E=150, in_c=16, out_c=16, towers=4, edge_dim=6, isolated=2):     # (sized to stay under 100 KiB)
    torch.set_num_threads(1)
    gen = torch.Generator().manual_seed(seed)
    src, dst = torch.randint(0, N, (2 * E,), generator=gen), torch.randint(0, N - isolated, (2 * E,), generator=gen)
    key = torch.unique(src * N + dst)
    key = key[torch.randperm(key.numel(), generator=gen)][:E]
    ei = torch.stack([key // N, key % N])
    deg_hist = torch.bincount(torch.bincount(ei[1], minlength=N)).long()
    aggregators, scalers = ["mean", "min", "max", "std"], ["identity", "amplification", "attenuation"]
    layer = RefConv(in_c, out_c, aggregators, scalers, deg_hist, edge_dim=edge_dim, towers=towers, pre_layers=1, post_layers=1, divide_input=True)
    with torch.no_grad():
        for p in layer.parameters():
            p.copy_(torch.randn(p.shape, generator=gen) / p.shape[1] ** 0.5 if p.dim() == 2 else 0.1 * torch.randn(p.shape, generator=gen))
    x, ea = torch.randn(N, in_c, generator=gen), torch.randn(ei.shape[1], edge_dim, generator=gen)
    R = torch.randn(N, out_c, generator=gen)
    sd = {"sd/" + k: v.detach().clone().numpy() for k, v in layer.state_dict().items()}
    arrays = dict(edge_index=ei.numpy(), deg_hist=deg_hist.numpy(), x=x.numpy(), edge_attr=ea.numpy(), R=R.numpy())
    arrays.update({"f32/" + k: v for k, v in step(layer, x, ei, ea, R, torch.float32).items()})
    arrays.update({"f64/" + k: v for k, v in step(layer, x, ei, ea, R, torch.float64).items()})
    meta = dict(kind="pyg_conv_train", seed=seed, N=N, in_c=in_c, out_c=out_c, aggregators=aggregators, scalers=scalers, towers=towers,
                divide_input=True, edge_dim=edge_dim, pre_layers=1, post_layers=1)
    np.savez_compressed(OUT, meta=json.dumps(meta), **arrays, **sd)
    print(f"{OUT}: {os.path.getsize(OUT) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
