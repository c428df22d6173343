"""bf16 inference on shards with REAL halos on one GPU: two processes share cuda:0 and exchange over gloo (the pattern of
tests/test_gpu_sharded_two_ranks.py).  Each rank's rows must EQUAL the rows [lo, hi) of the unsharded bf16 layer on the whole graph:
every row is reduced by one lane group (or the heavy schedule) in its edge order, the halo rows are copies of the owner's bits,
and the contractions sum each output row over that row alone in a fixed order.  Every wait is bounded."""
import os
import socket
import sys
import time
from datetime import timedelta

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = 4000
SCALERS = "identity amplification attenuation"


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _graphs():
    """(name, src, dst, balance) of the two graphs, generated on the host: seed 11 without locality (hubs; a few rows of each rank
    emptied), seed 12 with locality (mostly interior rows)."""
    from pna_amd.synth import powerlaw_graph
    src, dst = powerlaw_graph(V, 40000, seed=11, device="cpu")
    deg = torch.bincount(dst, minlength=V)
    empty = torch.tensor([3, 700, 1999, 2000, 2900, V - 1])
    assert int(deg[empty].max()) <= 128
    keep = ~torch.isin(dst, empty)
    src2, dst2 = powerlaw_graph(V, 2 * V + 600, seed=12, device="cpu")
    return [("seed11", src[keep], dst[keep], "nodes"), ("seed12", src2, dst2, "edges")]


def _worker(rank, world, port):
    os.environ["PNA_AMD_BF16_SMALL_ROWS"] = "0"   # the unsharded reference runs the multi-launch kernels (bit-identity is between those)
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=timedelta(seconds=120))
    try:
        from pna_amd import Graph
        from pna_amd.dgl.pna_layer import PNALayer, PNASimpleLayer
        from pna_amd.shard import shard_graph
        bf = torch.bfloat16
        avg = {"log": torch.tensor(2.0)}

        def rnd(*shape, seed):
            return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(bf).to(dev)

        for name, src, dst, balance in _graphs():
            src, dst = src.to(dev), dst.to(dev)
            gs, g = shard_graph(src, dst, V, balance=balance), Graph(src, dst, V)
            lo, hi = gs.lo, gs.hi
            # the properties the asserts below rely on
            interior, boundary = gs.split_rows()
            ldeg = gs.csr.rowptr[1:] - gs.csr.rowptr[:-1]
            assert gs.n_halo > 0 and interior.numel() > 0 and boundary.numel() > 0, (name, gs.n_halo, interior.numel(), boundary.numel())
            if name == "seed11":
                assert gs.heavy_schedule().n_heavy >= 1 and int((ldeg == 0).sum()) >= 1
            snorm = (torch.rand(V, 1, generator=torch.Generator().manual_seed(4)) + 0.5).to(bf).to(dev)

            def same(layer, call_whole, call_shard):
                with torch.no_grad():
                    want = call_whole(layer)[lo:hi]
                    got = call_shard(layer)
                    assert gs._pending is None
                    again = call_shard(layer)
                    assert gs._pending is None
                assert got.dtype == bf and got.shape == want.shape
                assert torch.equal(got.view(torch.int16), want.contiguous().view(torch.int16)), (name, type(layer).__name__)
                assert torch.equal(again.view(torch.int16), got.view(torch.int16))

            for F in (20, 75):
                torch.manual_seed(0)
                simple = PNASimpleLayer(F, F, "mean max min std", SCALERS, avg, 0.0, True, True).to(dev).eval().to(bf)
                assert simple.batch_norm and simple.residual
                with torch.no_grad():                                   # BatchNorm statistics that are not the identity
                    simple.batchnorm_h.running_mean.copy_(rnd(F, seed=8) * 0.1)
                    simple.batchnorm_h.running_var.copy_(rnd(F, seed=9).abs() + 0.5)
                h = rnd(V, F, seed=3)
                with torch.no_grad():
                    assert simple._bf16_path(gs, h[lo:hi])
                same(simple, lambda m: m(g, h), lambda m: m(gs, h[lo:hi]))                       # a plain slice
                wide = torch.zeros(hi - lo, F + 5, dtype=bf, device=dev)[:, :F]
                wide.copy_(h[lo:hi])
                same(simple, lambda m: m(g, h), lambda m: m(gs, wide))                           # a tensor at pitch F + 5
            F = 20
            h = rnd(V, F, seed=3)
            torch.manual_seed(1)
            tower = PNALayer(F, F, "mean max min std", SCALERS, avg, 0.0, True, True, towers=5, divide_input=False,
                             residual=True).to(dev).eval().to(bf)
            with torch.no_grad():
                assert tower._bf16_path(gs, h[lo:hi])
            same(tower, lambda m: m(g, h, None, snorm), lambda m: m(gs, h[lo:hi], None, snorm[lo:hi]))
            # divide_input towers with per-edge bf16 edge features (random rows: no edge-type table); the shard gets e[mine]
            ed = 6
            e = rnd(src.numel(), ed, seed=5)
            mine = (dst >= lo) & (dst < hi)
            torch.manual_seed(2)
            div = PNALayer(F, F, "mean max min std", SCALERS, avg, 0.0, True, True, towers=4, divide_input=True, residual=True,
                           edge_features=True, edge_dim=ed).to(dev).eval().to(bf)
            with torch.no_grad():
                assert div._bf16_path(gs, h[lo:hi], e[mine])
            same(div, lambda m: m(g, h, e, snorm), lambda m: m(gs, h[lo:hi], e[mine], snorm[lo:hi]))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def _spawn_bounded(fn, args, nprocs, deadline):
    """mp.spawn whose wait ends: a rank that fails in front of a collective takes the others down with it (join raises), and after
    `deadline` seconds the children are terminated."""
    ctx = mp.spawn(fn, args=args, nprocs=nprocs, join=False)
    end = time.monotonic() + deadline
    try:
        while not ctx.join(timeout=1.0):
            if time.monotonic() > end:
                raise TimeoutError(f"the ranks did not finish within {deadline} s")
    finally:
        for p in ctx.processes:
            if p.is_alive():
                p.terminate()
        for p in ctx.processes:
            p.join(10)


def test_two_rank_bf16_layers_on_shards_equal_the_unsharded_layers():
    _spawn_bounded(_worker, (2, _free_port()), 2, 240)
