"""Host side of the one-call training route of PNASimpleLayer (no GPU): the route predicate clause by clause, the exported symbols and
their args struct, the workspace size."""
import ctypes
import importlib
import os
import re
import shutil
import subprocess

import torch

from pna_amd import _lib
from pna_amd import functional as PF
from pna_amd.dgl.pna_layer import PNASimpleLayer
from pna_amd.graph import Graph
from pna_amd.shard import HaloGraph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _OnGpu:
    """A stand-in for fp32 features on the GPU (the predicate reads shape, dtype, is_cuda, dim, requires_grad and nothing else)."""

    def __init__(self, V, F, dtype=torch.float32, requires_grad=True):
        self.shape, self.dtype, self.is_cuda, self.requires_grad = (V, F), dtype, True, requires_grad

    def dim(self):
        return 2


def _graph(V=40, cls=Graph):
    src, dst = torch.arange(V), (torch.arange(V) + 1) % V
    if cls is Graph:
        return Graph(src, dst, V)
    return HaloGraph(src, dst, V, 0, torch.zeros(0, dtype=torch.long), [0], [0], None, 0, V, V)


def _layer(F=20, N=12, aggs="mean max min std", scalers="identity amplification", batch_norm=True, layers=1, residual=False):
    layer = PNASimpleLayer(F, N, aggs, scalers, {"log": 1.0}, 0.0, batch_norm, residual, posttrans_layers=layers).train()
    return layer


def test_route_is_off_by_default_and_read_from_the_environment(monkeypatch):
    monkeypatch.delenv("PNA_AMD_SMALL_TRAIN_ROWS", raising=False)
    try:
        assert importlib.reload(PF).SMALL_TRAIN_ROWS == 0
        monkeypatch.setenv("PNA_AMD_SMALL_TRAIN_ROWS", "4096")
        assert importlib.reload(PF).SMALL_TRAIN_ROWS == 4096
    finally:
        monkeypatch.delenv("PNA_AMD_SMALL_TRAIN_ROWS", raising=False)
        importlib.reload(PF)


def test_small_train_path_clause_by_clause(monkeypatch):
    g, shard, h = _graph(), _graph(cls=HaloGraph), _OnGpu(40, 20)
    assert g.csr.max_degree == 1                                                  # (built on the host, before tensors pretend below)
    # the 16-bit ranks of the max / min gradient (0xFFFF: none): in-degree 65534 is the last the route admits, 65535 the first it declines
    hubs = {d: _graph() for d in (65534, 65535)}
    for d, hub in hubs.items():
        hub._csr = hub.csr._replace(max_degree=d)
    # parameters and buffers report is_cuda -- the predicate's residency clause -- without a GPU
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    monkeypatch.setattr(PF, "SMALL_TRAIN_ROWS", 0)
    assert not _layer()._small_train_path(g, h)                                   # the knob at 0
    monkeypatch.setattr(PF, "SMALL_TRAIN_ROWS", 4096)
    assert _layer()._small_train_path(g, h)
    assert _layer(residual=True, N=20)._small_train_path(g, h)
    assert _layer()._small_train_path(hubs[65534], h) and not _layer()._small_train_path(hubs[65535], h)
    assert not _layer().eval()._small_train_path(g, h)                            # eval mode
    half = _layer()
    half.batchnorm_h.eval()
    assert not half._small_train_path(g, h)                                       # the BatchNorm alone in eval mode
    assert not _layer()._small_train_path(g, _OnGpu(40, 20, torch.bfloat16))      # bf16 features
    assert not _layer()._small_train_path(shard, h)               # a shard
    assert not _layer(layers=2)._small_train_path(g, h)                           # a 2-layer posttrans
    assert not _layer(batch_norm=False)._small_train_path(g, h)                   # no BatchNorm
    assert not _layer(aggs="mean min max std")._small_train_path(g, h)            # other aggregators, or another order
    assert not _layer(aggs="mean max min")._small_train_path(g, h)
    monkeypatch.setattr(PF, "SMALL_TRAIN_ROWS", 39)
    assert not _layer()._small_train_path(g, h)                                   # V above the knob
    monkeypatch.setattr(PF, "SMALL_TRAIN_ROWS", 4096)
    assert not _layer(F=3)._small_train_path(g, _OnGpu(40, 3))                    # outside the calls' widths
    assert not _layer(F=132, N=12)._small_train_path(g, _OnGpu(40, 132))
    frozen = _layer()
    for p in frozen.parameters():
        p.requires_grad_(False)
    assert not frozen._small_train_path(g, _OnGpu(40, 20, requires_grad=False))   # nothing requires a gradient
    assert frozen._small_train_path(g, h)
    cumulative = _layer()
    cumulative.batchnorm_h.momentum = None
    assert not cumulative._small_train_path(g, h)                                 # running statistics bn_tail_applies does not accept
    h_cpu = _OnGpu(40, 20)
    h_cpu.is_cuda = False
    assert not _layer()._small_train_path(g, h_cpu)


def test_symbols_are_exported_and_the_struct_has_gccs_layout(tmp_path):
    L = _lib.lib()
    for name in ("pna_simple_train_fwd_f32", "pna_simple_train_bwd_f32", "pna_simple_train_workspace_bytes"):
        assert hasattr(L, name), name
    assert L.pna_abi_version() == _lib.PNA_ABI_VERSION == 23
    header = open(os.path.join(ROOT, "include", "pna_amd.h")).read()
    assert "23, additive: + pna_simple_train_fwd_f32" in header
    # a short struct is refused before anything else is looked at
    L.pna_last_error.restype = ctypes.c_char_p
    for fn in (L.pna_simple_train_fwd_f32, L.pna_simple_train_bwd_f32):
        a = _lib.PnaSimpleTrainArgs()
        assert a.struct_size == ctypes.sizeof(_lib.PnaSimpleTrainArgs)
        for short in (0, ctypes.sizeof(_lib.PnaSimpleTrainArgs) - 8):
            a.struct_size = short
            assert fn(ctypes.byref(a), None) == -1 and b"struct_size" in L.pna_last_error()
    # the binding's layout is gcc's (the check tests/test_integration_stub.py runs on the generated mirrors)
    gcc = shutil.which("gcc")
    if gcc is None:
        return
    cls = _lib.PnaSimpleTrainArgs
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "pna_amd.h"', "int main(void) {",
             '  printf(". %zu 0\\n", sizeof(pna_simple_train_args));']
    for f, *_ in cls._fields_:
        lines.append(f'  printf("{f} %zu %zu\\n", sizeof(((pna_simple_train_args*)0)->{f}), offsetof(pna_simple_train_args, {f}));')
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "l.c", tmp_path / "l"
    src.write_text("\n".join(lines))
    subprocess.run([gcc, "-std=c11", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True)
    for f, size, off in (l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()):
        if f == ".":
            assert ctypes.sizeof(cls) == int(size)
        else:
            fld = getattr(cls, f)
            assert (fld.size, fld.offset) == (int(size), int(off)), (f, fld.size, fld.offset, size, off)
    block = re.search(r"class PnaSimpleTrainArgs\(_PnaArgs\)", open(os.path.join(ROOT, "INTEGRATION.md")).read())
    assert block, "INTEGRATION.md's generated mirrors lack the new struct"


def test_workspace_bytes_is_monotone_and_refuses_shapes_outside_the_scope():
    ws = _lib.lib().pna_simple_train_workspace_bytes
    for F, N, S in ((20, 12, 2), (75, 75, 3), (4, 1, 1), (128, 128, 3)):
        sizes = [ws(V, 4 * V, F, N, S) for V in (2, 15, 16, 17, 250, 400, 4096, 65536, 65537, 200000)]
        assert all(s > 0 and s % 256 == 0 for s in sizes)
        assert sizes == sorted(sizes) and sizes[0] < sizes[-1]
        assert ws(400, 0, F, N, S) <= ws(400, 4000, F, N, S) <= ws(400, 400000, F, N, S)
    for V, E, F, N, S in ((1, 0, 20, 12, 2), (400, -1, 20, 12, 2), (400, 10, 3, 12, 2), (400, 10, 129, 12, 2), (400, 10, 20, 0, 2),
                          (400, 10, 20, 129, 2), (400, 10, 20, 12, 0), (400, 10, 20, 12, 4)):
        assert ws(V, E, F, N, S) == -1, (V, E, F, N, S)
