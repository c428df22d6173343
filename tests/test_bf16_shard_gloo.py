"""HaloGraph.start_halo on CPU bf16 tensors over gloo (world 2 and 3): ONE async all_to_all_single of rows round8(F) elements wide
into a buffer of the halo rows alone; with the local rows in front it is the table the shard's source ids index, bit for bit."""
import os
import socket
import sys
import time
from datetime import timedelta

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _bits(t):
    return t.contiguous().view(torch.int16)


def _worker(rank, world, port):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=timedelta(seconds=60))
    try:
        from pna_amd.shard import shard_graph
        from pna_amd.synth import powerlaw_graph
        calls = []
        real = dist.all_to_all_single

        def recording(out, inp, *a, **k):
            calls.append((inp.numel() * inp.element_size(), inp.dtype, k.get("async_op", False)))
            return real(out, inp, *a, **k)

        V = 500
        src, dst = powerlaw_graph(V, 6000, seed=11, device="cpu")
        gs = shard_graph(src, dst, V)
        lo, hi = gs.lo, gs.hi
        mine = (dst >= lo) & (dst < hi)
        assert gs.n_halo > 0
        dist.all_to_all_single = recording
        try:
            for F, pitch in ((5, 5), (75, 80), (16, 32)):                       # dense rows; padded rows; the left half of wider rows
                P = (F + 7) // 8 * 8
                x = torch.randn(V, pitch, generator=torch.Generator().manual_seed(F)).to(torch.bfloat16)[:, :F]
                local = x[lo:hi]
                del calls[:]
                halo = gs.start_halo(local, F)
                assert gs._pending is not None
                gs.finish_exchange()
                assert gs._pending is None
                assert calls == [(sum(gs.send_splits) * P * 2, torch.bfloat16, True)], calls
                assert halo.shape == (gs.n_halo, P) and halo.dtype == torch.bfloat16
                assert int(torch.count_nonzero(_bits(halo[:, F:]))) == 0            # the padding columns
                table = torch.cat([local, halo[:, :F]])
                assert torch.equal(_bits(table[gs.src]), _bits(x[src[mine]]))
                assert gs.start_halo(local, F) is halo                              # the buffer is kept on the graph
                gs.finish_exchange()
            with pytest.raises(ValueError):
                gs.start_halo(x[lo:hi].float(), 5)
            # only the LAST rank has a halo: every rank enters the collective, the others with an empty buffer
            a = torch.arange(40)
            half = 40 // world
            src2 = torch.cat([a[: half * world], torch.tensor([0])])
            dst2 = torch.cat([(a[: half * world] // half) * half + (a[: half * world] % half + 1) % half, torch.tensor([half * world - 1])])
            g2 = shard_graph(src2, dst2, half * world)
            assert g2.any_exchange and g2.n_halo == (1 if rank == world - 1 else 0)
            y = torch.randn(half * world, 3, generator=torch.Generator().manual_seed(1)).to(torch.bfloat16)
            del calls[:]
            halo2 = g2.start_halo(y[g2.lo:g2.hi], 3)
            g2.finish_exchange()
            assert len(calls) == 1 and halo2.shape == (g2.n_halo, 8)
            m2 = (dst2 >= g2.lo) & (dst2 < g2.hi)
            assert torch.equal(_bits(torch.cat([y[g2.lo:g2.hi], halo2[:, :3]])[g2.src]), _bits(y[src2[m2]]))
            # NO rank has a halo: nobody enters it
            g3 = shard_graph(src2[:-1], dst2[:-1], half * world)
            assert not g3.any_exchange
            del calls[:]
            assert g3.start_halo(y[g3.lo:g3.hi], 3).shape == (0, 8) and g3._pending is None and not calls
        finally:
            dist.all_to_all_single = real
        dist.barrier()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_start_halo_exchanges_bf16_rows_at_the_wire_pitch(world):
    ctx = mp.spawn(_worker, args=(world, _free_port()), nprocs=world, join=False)
    end = time.monotonic() + 120
    try:
        while not ctx.join(timeout=1.0):
            assert time.monotonic() < end, "the ranks did not finish"
    finally:
        for p in ctx.processes:
            if p.is_alive():
                p.terminate()
        for p in ctx.processes:
            p.join(10)
