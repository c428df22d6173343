"""Host side of the net-ends route (no GPU): the float64 references of tests/net_ends_cases.py against torch autograd, the two route
predicates clause by clause, the exported symbols with their struct layouts and scope checks, the workspace size formula, and the
compiler's resource report of pna_net_ends.hip."""
import ctypes
import importlib
import os
import re
import shutil
import subprocess

import pytest
import torch
import torch.nn as nn

import net_ends_cases as C
from pna_amd import _lib, nets
from pna_amd import functional as PF
from pna_amd.graph import Graph
from pna_amd.shard import HaloGraph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pna_amd", "csrc")


# ---- the references ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["v2_f4_t9", "slab_plus_1_f80_t1", "unselected_row", "every_node_one_row"])
def test_embedding_reference_is_autograd_of_a_sum_of_embeddings(name):
    V, F, rows, idx, tables, go = C.embed_case(name)
    embs = [nn.Embedding(r, F).double() for r in rows]
    for e, w in zip(embs, tables):
        e.weight.data.copy_(w.double())
    out = 0
    for j, e in enumerate(embs):
        out = out + e(idx[:, j])
    torch.testing.assert_close(C.embed_ref64(idx, tables), out.detach(), rtol=1e-14, atol=1e-14)
    grads = torch.autograd.grad(out, [e.weight for e in embs], go.double())
    for j, ((ref, n, mass), g) in enumerate(zip(C.embed_grad_ref64(idx, rows, go), grads)):
        torch.testing.assert_close(ref, g, rtol=1e-13, atol=1e-13)
        assert torch.equal(n, torch.bincount(idx[:, j], minlength=rows[j]).double())
        assert (mass >= ref.abs() - 1e-12).all() and (ref[n == 0] == 0).all()
    if name == "unselected_row":
        assert C.embed_grad_ref64(idx, rows, go)[0][1][3] == 0
    if name == "every_node_one_row":
        assert C.embed_grad_ref64(idx, rows, go)[0][1].max() == V


@pytest.mark.parametrize("op", C.READOUT_OPS)
@pytest.mark.parametrize("tie", [False, True])
def test_readout_reference_is_autograd_of_a_segment_reduction(op, tie):
    sizes, h, go = C.readout_case("mixed", 70, tie=tie)
    h64 = h.double().requires_grad_(True)
    parts = torch.split(h64, sizes)
    if op == "max" and tie:
        # torch's max spreads nothing: amax would halve a tied gradient, max(0) sends it to one row -- the reference sends it to the FIRST
        vals, args = C.readout_ref64(h, sizes, op)
        g = sizes.index(sorted(sizes)[-2])
        at = sum(sizes[:g])
        assert (args[g] == at + 5).all() and (vals[g] == 9.0).all()
        gh = C.readout_grad_ref64(h, sizes, op, go)
        assert torch.equal(gh[at + 5], go[g].double()) and (gh[at + 11] == 0).all()
        return
    out = torch.stack([p.sum(0) if op == "sum" else p.mean(0) if op == "mean" else p.max(0).values for p in parts])
    vals, args = C.readout_ref64(h, sizes, op)
    torch.testing.assert_close(vals, out.detach(), rtol=1e-14, atol=1e-14)
    (gh,) = torch.autograd.grad(out, h64, go.double())
    torch.testing.assert_close(C.readout_grad_ref64(h, sizes, op, go), gh, rtol=1e-14, atol=1e-14)
    if op == "max":
        assert torch.equal(h.double()[args, torch.arange(70)], vals)


def test_the_serial_sum_bound():
    n, mass = torch.tensor([0.0, 1.0, 5.0]), torch.tensor([[0.0], [2.0], [3.0]])
    assert C.serial_sum_bound(n, mass).flatten().tolist() == [0.0, 2.0 * 2.0 ** -24, 15.0 * 2.0 ** -24]
    assert C.SLAB == _lib.PNA_EMBED_SLAB_ROWS and C.MAX_SLABS == _lib.PNA_EMBED_MAX_SLABS
    assert C.ATOM_DIMS == nets.AtomEncoderStandIn.DIMS


# ---- the knob and the predicates --------------------------------------------------------------------------------------------------------
def test_route_is_off_by_default_and_read_from_the_environment(monkeypatch):
    monkeypatch.delenv("PNA_AMD_NET_ENDS_ROWS", raising=False)
    try:
        assert importlib.reload(PF).NET_ENDS_ROWS == 0
        monkeypatch.setenv("PNA_AMD_NET_ENDS_ROWS", "4096")
        assert importlib.reload(PF).NET_ENDS_ROWS == 4096
    finally:
        monkeypatch.delenv("PNA_AMD_NET_ENDS_ROWS", raising=False)
        importlib.reload(PF)


class _OnGpu:
    """A stand-in for feature rows on the GPU (the readout predicate reads shape, dtype, is_cuda, dim, device and nothing else)."""

    def __init__(self, V, F, dtype=torch.float32):
        self.shape, self.dtype, self.is_cuda, self.device = (V, F), dtype, True, torch.device("cpu")

    def dim(self):
        return len(self.shape)


def _encoder(F=16, dims=C.ATOM_DIMS):
    return list(nets.AtomEncoderStandIn(F, dims).atom_embedding_list)


def test_embed_sum_path_clause_by_clause(monkeypatch):
    V = 40
    x = C._idx(V, C.ATOM_DIMS, 0)
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))     # residency without a GPU
    monkeypatch.setattr(PF, "NET_ENDS_ROWS", 0)
    assert not nets._embed_sum_path(_encoder(), x)                                # the knob at 0
    monkeypatch.setattr(PF, "NET_ENDS_ROWS", 4096)
    assert nets._embed_sum_path(_encoder(), x)
    assert nets._embed_sum_path(_encoder(128), x)                                 # the atom encoder at F = 128: 88 576 bytes
    assert nets._embed_sum_path([nn.Embedding(28, 70)], x[:, 0])                  # one table, a strided 1-D index
    monkeypatch.setattr(PF, "NET_ENDS_ROWS", V - 1)
    assert not nets._embed_sum_path(_encoder(), x)                                # more rows than the knob covers
    monkeypatch.setattr(PF, "NET_ENDS_ROWS", V)
    assert nets._embed_sum_path(_encoder(), x)
    monkeypatch.setattr(PF, "NET_ENDS_ROWS", 4096)
    assert not nets._embed_sum_path(_encoder(), x.to(torch.int32))                # another index type
    assert not nets._embed_sum_path(_encoder(), x[:, :8])                         # not one column per table
    assert not nets._embed_sum_path(_encoder(), x[:, 0])
    assert nets._embed_sum_path([nn.Embedding(28, 70)], x[:, :1])                 # an encoder of one table: one column
    assert not nets._embed_sum_path(_encoder(), x[:0])                            # no rows
    assert not nets._embed_sum_path([nn.Embedding(28, 70, padding_idx=0)], x[:, 0])
    assert not nets._embed_sum_path([nn.Embedding(28, 70, max_norm=1.0)], x[:, 0])
    half = _encoder()
    half[4] = half[4].to(torch.bfloat16)
    assert not nets._embed_sum_path(half, x)                                      # a bf16 table
    assert not nets._embed_sum_path([e.to(torch.bfloat16) for e in _encoder()], x)
    mixed = _encoder()
    mixed[2] = nn.Embedding(12, 20)
    assert not nets._embed_sum_path(mixed, x)                                     # tables of two widths
    assert not nets._embed_sum_path(_encoder(260), x)                             # outside the width
    assert nets._embed_sum_path(_encoder(188), x) and not nets._embed_sum_path(_encoder(192), x)   # 173 rows: 127.0 KiB and 129.75 KiB
    assert not nets._embed_sum_path([nn.Embedding(3, 8)] * 17, torch.zeros(V, 17, dtype=torch.int64))
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: False))
    assert not nets._embed_sum_path(_encoder(), x)                                # on the host


def test_embed_sum_path_at_the_lds_limit(monkeypatch):
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    monkeypatch.setattr(PF, "NET_ENDS_ROWS", 4096)
    x = torch.zeros(8, dtype=torch.int64)
    assert nets._embed_sum_path([nn.Embedding(256, 128)], x) and not nets._embed_sum_path([nn.Embedding(257, 128)], x)
    assert nets._embed_sum_path([nn.Embedding(256, 125)], x) and not nets._embed_sum_path([nn.Embedding(257, 125)], x)   # round4(F)
    assert PF.embed_sum_fits(C.ATOM_DIMS, 128) and sum(C.ATOM_DIMS) * 128 * 4 == 88576


def _graph(sizes, cls=Graph):
    V = sum(sizes)
    src, dst = torch.arange(V), torch.arange(V)
    if cls is Graph:
        return Graph(src, dst, V, sizes)
    return HaloGraph(src, dst, V, 0, torch.zeros(0, dtype=torch.long), [0], [0], None, 0, V, V)


def test_readout_path_clause_by_clause(monkeypatch):
    sizes = [3, 1, 36]
    g, h = _graph(sizes), _OnGpu(40, 70)
    monkeypatch.setattr(PF, "NET_ENDS_ROWS", 0)
    assert not nets._readout_path(g, h)                                           # the knob at 0
    monkeypatch.setattr(PF, "NET_ENDS_ROWS", 4096)
    assert nets._readout_path(g, h)
    assert nets._readout_offsets(g, h.device).tolist() == [0, 3, 4, 40] and nets._readout_offsets(g, h.device).dtype == torch.int32
    monkeypatch.setattr(PF, "NET_ENDS_ROWS", 39)
    assert not nets._readout_path(g, h)                                           # more nodes than the knob covers
    monkeypatch.setattr(PF, "NET_ENDS_ROWS", 40)
    assert nets._readout_path(g, h)
    assert not nets._readout_path(g, _OnGpu(40, 70, torch.bfloat16))              # bf16 rows keep their own kernel
    assert nets._readout_path(g, _OnGpu(40, 512)) and not nets._readout_path(g, _OnGpu(40, 513))
    assert not nets._readout_path(g, _OnGpu(39, 70))                              # not one row per node
    h_cpu = _OnGpu(40, 70)
    h_cpu.is_cuda = False
    assert not nets._readout_path(g, h_cpu)
    assert not nets._readout_path(_graph([3, 0, 37]), h)                          # an empty graph in the batch
    assert not nets._readout_path(_graph(sizes, cls=HaloGraph), h)                # a shard
    assert nets._readout_path(_graph([40]), h)                                    # an unbatched graph is one segment
    short = _graph(sizes)
    short.batch_num_nodes = [3, 1, 30]
    assert not nets._readout_path(short, h)                                       # sizes that do not cover the nodes


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------------
STRUCTS = {"pna_embed_sum_args": "PnaEmbedSumArgs", "pna_readout_args": "PnaReadoutArgs"}


def test_symbols_are_exported_and_the_structs_have_gccs_layout(tmp_path):
    L = _lib.lib()
    for name in ("pna_embed_sum_fwd_f32", "pna_embed_sum_bwd_f32", "pna_embed_sum_workspace_bytes", "pna_readout_fwd_f32", "pna_readout_bwd_f32"):
        assert hasattr(L, name), name
    assert L.pna_abi_version() == _lib.PNA_ABI_VERSION == 23
    assert "23, additive: + pna_embed_sum_fwd_f32" in open(os.path.join(ROOT, "include", "pna_amd.h")).read()
    L.pna_last_error.restype = ctypes.c_char_p
    for cls, fns in ((_lib.PnaEmbedSumArgs, (L.pna_embed_sum_fwd_f32, L.pna_embed_sum_bwd_f32)), (_lib.PnaReadoutArgs, (L.pna_readout_fwd_f32, L.pna_readout_bwd_f32))):
        for fn in fns:
            a = cls()
            assert a.struct_size == ctypes.sizeof(cls)
            for short in (0, ctypes.sizeof(cls) - 8):
                a.struct_size = short
                assert fn(ctypes.byref(a), None) == -1 and b"struct_size" in L.pna_last_error()
            a.struct_size = ctypes.sizeof(cls)
            assert fn(ctypes.byref(a), None) == -1 and b"struct_size" not in L.pna_last_error()          # all-zero: outside the scope
    gcc = shutil.which("gcc")
    if gcc is None:
        return
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "pna_amd.h"', "int main(void) {"]
    for s, c in STRUCTS.items():
        lines.append(f'  printf("{c} . %zu 0\\n", sizeof({s}));')
        for f, *_ in getattr(_lib, c)._fields_:
            lines.append(f'  printf("{c} {f} %zu %zu\\n", sizeof((({s}*)0)->{f}), offsetof({s}, {f}));')
    lines += ['  printf("consts %d %d %d\\n", PNA_MAX_EMBED_TABLE, PNA_EMBED_SLAB_ROWS, PNA_EMBED_MAX_SLABS);', "  return 0;", "}"]
    src, exe = tmp_path / "l.c", tmp_path / "l"
    src.write_text("\n".join(lines))
    subprocess.run([gcc, "-std=c11", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True)
    for c, f, size, off in (l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()):
        if c == "consts":
            assert (int(f), int(size), int(off)) == (_lib.PNA_MAX_EMBED_TABLE, _lib.PNA_EMBED_SLAB_ROWS, _lib.PNA_EMBED_MAX_SLABS)
            continue
        cls = getattr(_lib, c)
        if f == ".":
            assert ctypes.sizeof(cls) == int(size)
        else:
            fld = getattr(cls, f)
            assert (fld.size, fld.offset) == (int(size), int(off)), (c, f, fld.size, fld.offset, size, off)
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for c in STRUCTS.values():
        assert re.search(rf"class {c}\(_PnaArgs\)", text), f"INTEGRATION.md's generated mirrors lack {c}"


def _ws(V, rows, F):
    return _lib.lib().pna_embed_sum_workspace_bytes(V, len(rows), (ctypes.c_int32 * max(1, len(rows)))(*rows), F)


def test_workspace_bytes_formula_and_scope():
    for rows, F in ((C.ATOM_DIMS, 128), (C.ATOM_DIMS, 75), ((28,), 70), ((1,), 1), ((16,) * 16, 128)):
        image = sum(rows) * ((F + 3) // 4 * 4) * 4
        for V in (1, 2, C.SLAB - 1, C.SLAB, C.SLAB + 1, 3 * C.SLAB + 17, C.SLAB * C.MAX_SLABS, C.SLAB * C.MAX_SLABS + 1, 52000, 10 ** 6, 2 ** 31 - 1):
            L = max(C.SLAB, -(-V // C.MAX_SLABS))
            n_slab = -(-V // L)
            assert n_slab <= C.MAX_SLABS                                           # bounded however large V is
            assert _ws(V, rows, F) == n_slab * image == PF.embed_sum_workspace_bytes(V, rows, F), (V, rows, F)
            assert max(_lib.PNA_EMBED_SLAB_ROWS, -(-V // _lib.PNA_EMBED_MAX_SLABS)) == L
    # the LDS limit: one fp32 image of all tables within 128 KiB -- a positive size just inside, -1 just outside
    assert _ws(100, (256,), 128) == 2 * 128 * 1024 and _ws(100, (257,), 128) == -1
    assert _ws(100, (119, 137), 128) > 0 and _ws(100, (119, 138), 128) == -1
    assert _ws(100, (128,), 256) > 0 and _ws(100, (129,), 256) == -1
    assert _ws(100, (256,), 125) > 0 and _ws(100, (257,), 125) == -1               # the image's pitch is round4(F)
    assert PF.embed_sum_workspace_bytes(100, (257,), 128) == -1
    for V, rows, F in ((0, (5,), 8), (-3, (5,), 8), (2 ** 31, (5,), 8), (10, (), 8), (10, (2,) * 17, 8), (10, (5,), 0), (10, (5,), 257), (10, (5, 0), 8)):
        assert _ws(V, rows, F) == -1, (V, rows, F)
    assert _lib.lib().pna_embed_sum_workspace_bytes(10, 1, None, 8) == -1


# ---- the compiler's report ----------------------------------------------------------------------------------------------------------------
def test_no_kernel_of_the_file_uses_scratch(tmp_path):
    """As tests/test_build_resources.py does for the files it lists: the slab kernel indexes its by-value argument block (table
    pointers, row counts) with run-time table numbers, which must stay loads from the argument segment and never become a stack copy."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
           "-S", "--cuda-device-only", "-o", str(tmp_path / "out.s"), os.path.join(CSRC, "pna_net_ends.hip"), "-Rpass-analysis=kernel-resource-usage"]
    out = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    names = re.findall(r"Function Name: (\S+)", out)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", out)]
    assert len(names) == len(scratch) == 5, names
    for k in ("k_embed_sum_fwd", "k_embed_sum_bwd_slab", "k_embed_sum_bwd_final", "k_readout_fwd", "k_readout_bwd"):
        assert any(k in n for n in names), k
    assert not [(n, s) for n, s in zip(names, scratch) if s != 0]
