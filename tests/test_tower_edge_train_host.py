"""Host side of the one-call training route of PNALayer WITH EDGE FEATURES (no GPU): the knob, the route predicate clause by clause, the
exported symbols and their args struct, the workspace size and its Python mirror, the new kernels' resources."""
import ctypes
import importlib
import os
import re
import shutil
import subprocess

import pytest
import torch

from pna_amd import _lib
from pna_amd import functional as PF
from pna_amd.dgl.pna_layer import PNALayer
from pna_amd.graph import Graph
from pna_amd.shard import HaloGraph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _OnGpu:
    """A stand-in for an fp32 tensor on the GPU (the predicate reads shape, dtype, is_cuda, dim, requires_grad, numel and nothing else)."""

    def __init__(self, V, F, dtype=torch.float32, requires_grad=True):
        self.shape, self.dtype, self.is_cuda, self.requires_grad = (V, F), dtype, True, requires_grad

    def dim(self):
        return 2

    def numel(self):
        return self.shape[0] * self.shape[1]


def _graph(V=40, cls=Graph):
    src, dst = torch.arange(V), (torch.arange(V) + 1) % V
    if cls is Graph:
        return Graph(src, dst, V)
    return HaloGraph(src, dst, V, 0, torch.zeros(0, dtype=torch.long), [0], [0], None, 0, V, V)


def _layer(in_dim=24, out_dim=24, towers=4, scalers="identity amplification attenuation", aggs="mean max min std", dropout=0.0, graph_norm=True,
           batch_norm=True, pre=1, post=1, divide_input=True, residual=True, edge_features=True, edge_dim=3):
    return PNALayer(in_dim, out_dim, aggs, scalers, {"log": 1.0}, dropout, graph_norm, batch_norm, towers=towers, pretrans_layers=pre,
                    posttrans_layers=post, divide_input=divide_input, residual=residual, edge_features=edge_features,
                    edge_dim=edge_dim if edge_features else 0).train()


def test_route_is_off_by_default_and_read_from_the_environment(monkeypatch):
    monkeypatch.delenv("PNA_AMD_SMALL_TOWER_TRAIN_EDGE_ROWS", raising=False)
    try:
        assert importlib.reload(PF).SMALL_TOWER_TRAIN_EDGE_ROWS == 0
        monkeypatch.setenv("PNA_AMD_SMALL_TOWER_TRAIN_EDGE_ROWS", "4096")
        mod = importlib.reload(PF)
        assert mod.SMALL_TOWER_TRAIN_EDGE_ROWS == 4096 and mod.SMALL_TOWER_TRAIN_ROWS == 0      # a knob of its own
    finally:
        monkeypatch.delenv("PNA_AMD_SMALL_TOWER_TRAIN_EDGE_ROWS", raising=False)
        importlib.reload(PF)


def test_small_tower_train_edge_path_clause_by_clause(monkeypatch):
    g, shard, h, n = _graph(), _graph(cls=HaloGraph), _OnGpu(40, 24), _OnGpu(40, 1, requires_grad=False)
    e = _OnGpu(40, 3, requires_grad=False)
    assert g.csr.max_degree == 1 and g.csr.col.numel() == 40                      # (built on the host, before tensors pretend below)
    # the 16-bit ranks of the max / min gradient (0xFFFF: none): in-degree 65534 is the last the route admits, 65535 the first it declines
    hubs = {d: _graph() for d in (65534, 65535)}
    for d, hub in hubs.items():
        hub._csr = hub.csr._replace(max_degree=d)
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    monkeypatch.setattr(PF, "SMALL_TOWER_TRAIN_EDGE_ROWS", 0)
    monkeypatch.setattr(PF, "SMALL_TOWER_TRAIN_ROWS", 4096)
    assert not _layer()._small_tower_train_edge_path(g, h, e, n)                  # the knob at 0 (the other route's knob does not open it)
    assert not _layer()._small_tower_train_path(g, h, n)                          # ... and that route still refuses edge features
    monkeypatch.setattr(PF, "SMALL_TOWER_TRAIN_EDGE_ROWS", 4096)
    monkeypatch.setattr(PF, "SMALL_TOWER_TRAIN_ROWS", 0)
    assert _layer()._small_tower_train_edge_path(g, h, e, n)
    assert _layer(residual=False)._small_tower_train_edge_path(g, h, e, n)
    assert _layer()._small_tower_train_edge_path(hubs[65534], h, e, n) and not _layer()._small_tower_train_edge_path(hubs[65535], h, e, n)
    assert _layer(graph_norm=False)._small_tower_train_edge_path(g, h, e, None)
    assert _layer(divide_input=False)._small_tower_train_edge_path(g, h, e, n)
    assert _layer(in_dim=70, out_dim=70, towers=5, edge_dim=50)._small_tower_train_edge_path(g, _OnGpu(40, 70), _OnGpu(40, 50), n)      # ZINC's first layers
    assert _layer(in_dim=70, out_dim=60, towers=5, edge_dim=50)._small_tower_train_edge_path(g, _OnGpu(40, 70), _OnGpu(40, 50), n)      # ... and its last
    assert _layer(edge_dim=1)._small_tower_train_edge_path(g, h, _OnGpu(40, 1), n)
    assert _layer(edge_dim=64)._small_tower_train_edge_path(g, h, _OnGpu(40, 64), n)
    # each of the following alone sends the call to the old route: first the clauses about the edge features
    assert not _layer(edge_features=False)._small_tower_train_edge_path(g, h, e, n)          # a layer without edge features
    assert not _layer(edge_dim=65)._small_tower_train_edge_path(g, h, _OnGpu(40, 65), n)     # edge_dim above 64
    assert not _layer()._small_tower_train_edge_path(g, h, None, n)                          # no e
    assert not _layer()._small_tower_train_edge_path(g, h, _OnGpu(40, 3, torch.float64), n)  # fp64 e
    assert not _layer()._small_tower_train_edge_path(g, h, _OnGpu(39, 3), n)                 # a wrong row count
    assert not _layer()._small_tower_train_edge_path(g, h, _OnGpu(40, 4), n)                 # a wrong width
    e_cpu = _OnGpu(40, 3)
    e_cpu.is_cuda = False
    assert not _layer()._small_tower_train_edge_path(g, h, e_cpu, n)
    odd = _layer()
    odd.towers[1].edge_dim = 4
    assert not odd._small_tower_train_edge_path(g, h, e, n)                       # one tower with another edge_dim
    odd = _layer()
    odd.towers[2].edge_features = False
    assert not odd._small_tower_train_edge_path(g, h, e, n)                       # one tower without edge features
    odd = _layer()
    odd.towers[0].pretrans.fully_connected[0].linear = torch.nn.Linear(2 * 6 + 2, 6)
    assert not odd._small_tower_train_edge_path(g, h, e, n)                       # a pretrans weight of another shape
    # ... then the clauses shared with the route without edge features
    assert not _layer(dropout=0.3)._small_tower_train_edge_path(g, h, e, n)
    assert not _layer().eval()._small_tower_train_edge_path(g, h, e, n)
    half = _layer()
    half.towers[2].batchnorm_h.eval()
    assert not half._small_tower_train_edge_path(g, h, e, n)
    assert not _layer(pre=2)._small_tower_train_edge_path(g, h, e, n)
    assert not _layer(post=2)._small_tower_train_edge_path(g, h, e, n)
    assert not _layer(in_dim=130, out_dim=130, towers=5)._small_tower_train_edge_path(g, _OnGpu(40, 130), e, n)
    assert not _layer(in_dim=520, out_dim=40, towers=4)._small_tower_train_edge_path(g, _OnGpu(40, 520), e, n)
    assert not _layer()._small_tower_train_edge_path(_graph(1), _OnGpu(1, 24), _OnGpu(1, 3), _OnGpu(1, 1))
    assert not _layer()._small_tower_train_edge_path(g, _OnGpu(40, 24, torch.float64), e, n)
    assert not _layer()._small_tower_train_edge_path(shard, h, e, n)
    assert not _layer(batch_norm=False)._small_tower_train_edge_path(g, h, e, n)
    assert not _layer(aggs="mean min max std")._small_tower_train_edge_path(g, h, e, n)
    assert not _layer(towers=12, in_dim=48, out_dim=48)._small_tower_train_edge_path(g, _OnGpu(40, 48), e, n)
    assert not _layer(in_dim=12, out_dim=24)._small_tower_train_edge_path(g, _OnGpu(40, 12), e, n)                         # Fi = 3
    assert not _layer()._small_tower_train_edge_path(g, h, e, None)               # graph norm without its factor
    monkeypatch.setattr(PF, "SMALL_TOWER_TRAIN_EDGE_ROWS", 39)
    assert not _layer()._small_tower_train_edge_path(g, h, e, n)                  # V above the knob
    monkeypatch.setattr(PF, "SMALL_TOWER_TRAIN_EDGE_ROWS", 4096)
    frozen = _layer()
    for p in frozen.parameters():
        p.requires_grad_(False)
    h_ng = _OnGpu(40, 24, requires_grad=False)
    assert not frozen._small_tower_train_edge_path(g, h_ng, e, n)                 # nothing requires a gradient
    assert frozen._small_tower_train_edge_path(g, h, e, n)                        # h does
    assert frozen._small_tower_train_edge_path(g, h_ng, _OnGpu(40, 3, requires_grad=True), n)         # e does
    cumulative = _layer()
    cumulative.towers[0].batchnorm_h.momentum = None
    assert not cumulative._small_tower_train_edge_path(g, h, e, n)
    for field, value in (("eps", 1e-3), ("momentum", 0.2)):
        odd = _layer()
        setattr(odd.towers[1].batchnorm_h, field, value)
        assert not odd._small_tower_train_edge_path(g, h, e, n)
    assert not _layer().double()._small_tower_train_edge_path(g, h, e, n)
    mixdrop = _layer()
    mixdrop.mixing_network.dropout = torch.nn.Dropout(0.2)
    assert not mixdrop._small_tower_train_edge_path(g, h, e, n)
    h_cpu = _OnGpu(40, 24)
    h_cpu.is_cuda = False
    assert not _layer()._small_tower_train_edge_path(g, h_cpu, e, n)


def test_symbols_are_exported_and_the_struct_has_gccs_layout(tmp_path):
    L = _lib.lib()
    for name in ("pna_tower_edge_train_fwd_f32", "pna_tower_edge_train_bwd_f32", "pna_tower_edge_train_workspace_bytes"):
        assert hasattr(L, name), name
    assert L.pna_abi_version() == _lib.PNA_ABI_VERSION == 23
    header = open(os.path.join(ROOT, "include", "pna_amd.h")).read()
    assert "23, additive: + pna_tower_edge_train_fwd_f32" in header and "models/dgl/pna_layer.py:35-40" in header
    L.pna_last_error.restype = ctypes.c_char_p
    cls = _lib.PnaTowerEdgeTrainArgs
    for fn in (L.pna_tower_edge_train_fwd_f32, L.pna_tower_edge_train_bwd_f32):
        a = cls()
        assert a.struct_size == ctypes.sizeof(cls)
        for short in (0, ctypes.sizeof(cls) - 8):
            a.struct_size = short
            assert fn(ctypes.byref(a), None) == -1 and b"struct_size" in L.pna_last_error()
        a = cls()
        assert fn(ctypes.byref(a), None) == -1 and b"pna_tower_edge_train" in L.pna_last_error()      # a NULL base: refused with a message
    gcc = shutil.which("gcc")
    if gcc is None:
        return
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "pna_amd.h"', "int main(void) {",
             '  printf(". %zu 0\\n", sizeof(pna_tower_edge_train_args));']
    for f, *_ in cls._fields_:
        lines.append(f'  printf("{f} %zu %zu\\n", sizeof(((pna_tower_edge_train_args*)0)->{f}), offsetof(pna_tower_edge_train_args, {f}));')
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
    assert re.search(r"class PnaTowerEdgeTrainArgs\(_PnaArgs\)", open(os.path.join(ROOT, "INTEGRATION.md")).read()), \
        "INTEGRATION.md's generated mirrors lack the new struct"


def test_workspace_bytes_is_monotone_refuses_shapes_outside_the_scope_and_the_mirror_agrees():
    ws = _lib.lib().pna_tower_edge_train_workspace_bytes
    base = _lib.lib().pna_tower_train_workspace_bytes
    for T, Fi, Fo, S, div, ed in ((5, 14, 14, 3, 1, 50), (5, 14, 12, 3, 1, 50), (3, 18, 6, 3, 0, 5), (1, 20, 20, 1, 0, 1), (8, 16, 16, 3, 1, 64),
                                  (1, 128, 128, 3, 0, 64), (2, 4, 4, 3, 1, 64)):
        sizes = [ws(V, 4 * V, T, Fi, Fo, S, div, ed) for V in (2, 15, 16, 17, 250, 400, 4096, 65536, 65537, 200000)]
        assert all(s > 0 and s % 256 == 0 for s in sizes)
        assert sizes == sorted(sizes) and sizes[0] < sizes[-1]                     # monotone in V ...
        by_e = [ws(400, E, T, Fi, Fo, S, div, ed) for E in (0, 1, 15, 16, 17, 255, 256, 257, 4000, 400000)]
        assert by_e == sorted(by_e) and by_e[0] < by_e[-1]                         # ... and in E (dm and the CSR copy of e grow with it)
    for args in ((1, 0, 4, 6, 6, 3, 1, 3), (400, -1, 4, 6, 6, 3, 1, 3), (400, 10, 0, 6, 6, 3, 1, 3), (400, 10, 9, 6, 6, 3, 1, 3), (400, 10, 4, 3, 6, 3, 1, 3),
                 (400, 10, 4, 130, 6, 3, 1, 3), (400, 10, 4, 6, 0, 3, 1, 3), (400, 10, 4, 6, 33, 3, 1, 3), (400, 10, 4, 6, 6, 0, 1, 3), (400, 10, 4, 6, 6, 4, 1, 3),
                 (400, 10, 4, 6, 6, 3, 2, 3), (400, 10, 4, 6, 6, 3, 1, 0), (400, 10, 4, 6, 6, 3, 1, -1), (400, 10, 4, 6, 6, 3, 1, 65)):
        assert ws(*args) == -1, args
    for T in (0, 1, 5, 8, 9):
        for Fi in (3, 4, 14, 64, 65, 128, 129):
            for Fo in (0, 1, 12, 16, 26, 128, 129):
                for S in (0, 1, 3, 4):
                    for ed in (0, 1, 50, 64, 65):
                        fits = PF.small_tower_train_edge_fits(T, Fi, Fo, S, ed)
                        want = 1 <= T <= 8 and 4 <= Fi <= 128 and T * Fi <= 512 and 1 <= Fo and T * Fo <= 128 and 1 <= S <= 3 and 1 <= ed <= 64
                        assert fits == want == (ws(400, 1000, T, Fi, Fo, S, 1, ed) >= 0), (T, Fi, Fo, S, ed)
                        if fits:                                                   # inside the scope of the route without edge features
                            assert base(400, 1000, T, Fi, Fo, S, 1) >= 0


def test_kernels_use_no_scratch(tmp_path):
    """The recipe of tests/test_build_resources.py::test_no_kernel_uses_scratch on pna_tower_train.hip: the new kernels are there (the
    rows kernel in both forms) and no kernel uses scratch."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "pna_amd", "csrc")
    out_s = str(tmp_path / "out.s")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
           "-S", "--cuda-device-only", "-o", out_s, os.path.join(csrc, "pna_tower_train.hip"), "-Rpass-analysis=kernel-resource-usage"]
    out = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    names = re.findall(r"Function Name: (\S+)", out)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", out)]
    assert len(names) == len(scratch) and len(names) >= 19          # 12 plain kernels + the rows kernels: forward 3 x 2, backward 3
    for key in ("k_tt_edge_project", "k_tt_edge_dm", "k_tt_edge_pull", "k_tt_edge_grad_e", "k_tt_project", "k_tt_grad_h", "k_tt_dw_plain"):
        assert any(key in n for n in names), key
    assert sum("k_tt_rows_fwd" in n for n in names) == 6
    bad = [(n, s) for n, s in zip(names, scratch) if s != 0]
    assert not bad, f"kernels using scratch: {bad}"
    assert "v_mfma_f32_16x16x4_f32" in open(out_s).read()
