"""Host side of the one-call training route of PNALayer WITH DROPOUT inside the towers (no GPU): the numpy restatement of Philox4x32-10
and of the mask rule against known answers, the knob, the route predicate, the exported symbols and their args struct, the argument
checks that need no device, the masked float64 oracle, the new kernel instantiations' resources."""
import ctypes
import importlib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import tower_drop_train_cases as C
from oracle import torch_oracle as O
from pna_amd import _lib
from pna_amd import autograd as AG
from pna_amd import functional as PF
from pna_amd.dgl.pna_layer import PNALayer
from pna_amd.graph import Graph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _OnGpu:
    """A stand-in for an fp32 tensor on the GPU (the predicate reads shape, dtype, is_cuda, dim, requires_grad, numel and nothing else)."""

    def __init__(self, V, F, dtype=torch.float32, requires_grad=True):
        self.shape, self.dtype, self.is_cuda, self.requires_grad = (V, F), dtype, True, requires_grad

    def dim(self):
        return 2

    def numel(self):
        return self.shape[0] * self.shape[1]


def _graph(V=40):
    return Graph(torch.arange(V), (torch.arange(V) + 1) % V, V)


def _layer(dropout=0.3, edge_features=False, edge_dim=3, in_dim=24, out_dim=24, towers=4, **kw):
    return PNALayer(in_dim, out_dim, "mean max min std", "identity amplification attenuation", {"log": 1.0}, dropout, True, True, towers=towers,
                    pretrans_layers=1, posttrans_layers=1, divide_input=True, residual=True, edge_features=edge_features,
                    edge_dim=edge_dim if edge_features else 0, **kw).train()


def test_philox_restatement_reproduces_the_known_answers():
    for counter, key, want in C.KNOWN_ANSWERS:
        assert tuple(int(w) for w in C.philox4x32_10(counter, key)) == want
    # vectorised = one at a time, and element e reads word e & 3 of quad e >> 2 with the offset in the counter's high half
    seed, offset = (9 << 32) | 5, (3 << 32) | 8
    words = C.host_words(10, seed, offset, first=6)
    for i, e in enumerate(range(6, 16)):
        one = C.philox4x32_10((e >> 2, 0, offset & C.MASK32, offset >> 32), (seed & C.MASK32, seed >> 32))
        assert int(words[i]) == int(one[e & 3])


def test_threshold_and_scale_of_the_mask_rule():
    assert C.thr_of(0.0) == 0
    assert C.thr_of(0.1) == int(float(np.float32(0.1)) * 2 ** 32) == 0x199999A0      # (float) 0.1 = 0x3DCCCCCD: 13421773 2^-27, times 2^32 exactly
    assert C.thr_of(0.3) == int(float(np.float32(0.3)) * 2 ** 32) == 0x4CCCCD00
    last = np.nextafter(np.float32(1.0), np.float32(0.0))
    assert C.thr_of(last) == 0xFFFFFF00 and C.thr_of(1.0) == 0xFFFFFFFF              # (p = 1 itself is refused by the calls: the cap only)
    assert C.scale_of(0.0) == np.float32(1.0) and C.scale_of(0.3).dtype == np.float32
    assert C.scale_of(0.3) == np.float32(1.0) / np.float32(0.7)                      # (1.0f - 0.3f rounds to (float) 0.7)
    m = C.host_mask(45, 75, 0.0, 1, 0)
    assert m.dtype == np.float32 and bool((m == 1.0).all())                          # p = 0 keeps everything, factor 1
    m = C.host_mask(45, 75, 0.3, 1, 0)
    assert set(np.unique(m)) == {np.float32(0.0), C.scale_of(0.3)} and 0.25 < float((m == 0).mean()) < 0.35
    assert not np.array_equal(m, C.host_mask(45, 75, 0.3, 1, 4)) and not np.array_equal(m, C.host_mask(45, 75, 0.3, 2, 0))


def test_route_is_off_by_default_and_read_from_the_environment(monkeypatch):
    monkeypatch.delenv("PNA_AMD_SMALL_TOWER_TRAIN_DROPOUT_ROWS", raising=False)
    try:
        assert importlib.reload(PF).SMALL_TOWER_TRAIN_DROPOUT_ROWS == 0
        monkeypatch.setenv("PNA_AMD_SMALL_TOWER_TRAIN_DROPOUT_ROWS", "4096")
        mod = importlib.reload(PF)
        assert mod.SMALL_TOWER_TRAIN_DROPOUT_ROWS == 4096 and mod.SMALL_TOWER_TRAIN_ROWS == 0 and mod.SMALL_TOWER_TRAIN_EDGE_ROWS == 0
    finally:
        monkeypatch.delenv("PNA_AMD_SMALL_TOWER_TRAIN_DROPOUT_ROWS", raising=False)
        importlib.reload(PF)


def test_small_tower_drop_train_path(monkeypatch):
    g, h, n, e = _graph(), _OnGpu(40, 24), _OnGpu(40, 1, requires_grad=False), _OnGpu(40, 3, requires_grad=False)
    assert g.csr.col.numel() == 40
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    monkeypatch.setattr(PF, "SMALL_TOWER_TRAIN_DROPOUT_ROWS", 4096)
    # served: tower dropout 0.1 / 0.3, with and without edge features
    for p in (0.1, 0.3):
        assert _layer(p)._small_tower_drop_train_path(g, h, None, n)
        assert _layer(p, edge_features=True)._small_tower_drop_train_path(g, h, e, n)
    assert _layer(0.1, in_dim=75, out_dim=70, towers=5)._small_tower_drop_train_path(g, _OnGpu(40, 75), None, n)          # the CIFAR10 / MNIST layers
    assert _layer(0.3, in_dim=75, out_dim=75, towers=5, edge_features=True, edge_dim=50)._small_tower_drop_train_path(g, _OnGpu(40, 75), _OnGpu(40, 50), n)
    # refused: no dropout (the other routes' layers), p >= 1, unequal tower dropouts, mixing-network dropout, eval, the knob off or too small
    assert not _layer(0.0)._small_tower_drop_train_path(g, h, None, n)
    assert not _layer(1.0)._small_tower_drop_train_path(g, h, None, n)
    assert not _layer(1.5)._small_tower_drop_train_path(g, h, None, n)
    odd = _layer(0.3)
    odd.towers[2].dropout = 0.1
    assert not odd._small_tower_drop_train_path(g, h, None, n)
    odd = _layer(0.3)
    odd.towers[1].dropout = 0.0
    assert not odd._small_tower_drop_train_path(g, h, None, n)
    mixdrop = _layer(0.3)
    mixdrop.mixing_network.dropout = torch.nn.Dropout(0.2)
    assert not mixdrop._small_tower_drop_train_path(g, h, None, n)
    assert not _layer(0.3).eval()._small_tower_drop_train_path(g, h, None, n)
    # ... the edge clauses apply when the layer has edge features, and only then
    assert not _layer(0.3, edge_features=True)._small_tower_drop_train_path(g, h, None, n)
    assert not _layer(0.3, edge_features=True)._small_tower_drop_train_path(g, h, _OnGpu(40, 4), n)
    assert not _layer(0.3, edge_features=True, edge_dim=65)._small_tower_drop_train_path(g, h, _OnGpu(40, 65), n)
    assert _layer(0.3)._small_tower_drop_train_path(g, h, e, n)                   # (a layer without edge features ignores e, as its forward does)
    # ... and the shared ones: a sample of them
    assert not _layer(0.3)._small_tower_drop_train_path(g, _OnGpu(40, 24, torch.float64), None, n)
    assert not _layer(0.3)._small_tower_drop_train_path(g, h, None, None)         # graph norm without its factor
    assert not _layer(0.3, in_dim=12, out_dim=24)._small_tower_drop_train_path(g, _OnGpu(40, 12), None, n)                # Fi = 3
    frozen = _layer(0.3)
    for q in frozen.parameters():
        q.requires_grad_(False)
    assert not frozen._small_tower_drop_train_path(g, _OnGpu(40, 24, requires_grad=False), None, n)
    monkeypatch.setattr(PF, "SMALL_TOWER_TRAIN_DROPOUT_ROWS", 39)
    assert not _layer(0.3)._small_tower_drop_train_path(g, h, None, n)
    monkeypatch.setattr(PF, "SMALL_TOWER_TRAIN_DROPOUT_ROWS", 0)
    monkeypatch.setattr(PF, "SMALL_TOWER_TRAIN_ROWS", 4096)
    monkeypatch.setattr(PF, "SMALL_TOWER_TRAIN_EDGE_ROWS", 4096)
    assert not _layer(0.3)._small_tower_drop_train_path(g, h, None, n)            # the other routes' knobs do not open it
    assert not _layer(0.3, edge_features=True)._small_tower_drop_train_path(g, h, e, n)
    # not while the stream is being captured: a replay would repeat the captured mask
    monkeypatch.setattr(PF, "SMALL_TOWER_TRAIN_DROPOUT_ROWS", 4096)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    assert not _layer(0.3)._small_tower_drop_train_path(g, h, None, n)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    assert _layer(0.3)._small_tower_drop_train_path(g, h, None, n)


def test_the_two_existing_predicates_still_refuse_dropout(monkeypatch):
    g, h, n, e = _graph(), _OnGpu(40, 24), _OnGpu(40, 1, requires_grad=False), _OnGpu(40, 3, requires_grad=False)
    assert g.csr.max_degree == 1                                                  # (built on the host, before tensors pretend below)
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    for name in ("SMALL_TOWER_TRAIN_ROWS", "SMALL_TOWER_TRAIN_EDGE_ROWS", "SMALL_TOWER_TRAIN_DROPOUT_ROWS"):
        monkeypatch.setattr(PF, name, 4096)
    assert _layer(0.0)._small_tower_train_path(g, h, n) and _layer(0.0, edge_features=True)._small_tower_train_edge_path(g, h, e, n)
    for p in (0.1, 0.3):
        assert not _layer(p)._small_tower_train_path(g, h, n)
        assert not _layer(p, edge_features=True)._small_tower_train_edge_path(g, h, e, n)


def test_symbols_are_declared_bound_and_the_struct_has_gccs_layout(tmp_path):
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "pna_amd.h")).read()
    for name in ("pna_tower_drop_train_fwd_f32", "pna_tower_drop_train_bwd_f32", "pna_dropout_mask_f32"):
        assert hasattr(L, name), name
        assert re.search(r"\bint " + name + r"\(", header), name
        assert getattr(L, name).argtypes is not None, name
    assert "pna_tower_drop_args" in header and "23, additive: + pna_tower_drop_train_fwd_f32" in header and "models/dgl/pna_layer.py:71-75" in header
    assert L.pna_abi_version() == _lib.PNA_ABI_VERSION == 23
    assert hasattr(AG, "TowerLayerDropSmallTrainFn") and hasattr(PF, "dropout_mask") and hasattr(PF, "tower_dropout_key")
    cls = _lib.PnaTowerDropArgs
    assert [f for f, *_ in cls._fields_] == ["struct_size", "_abi_reserved", "base", "edge", "p", "_pad0", "seed", "offset"]
    gcc = shutil.which("gcc")
    if gcc is None:
        return
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "pna_amd.h"', "int main(void) {", '  printf(". %zu 0\\n", sizeof(pna_tower_drop_args));']
    for f, *_ in cls._fields_:
        lines.append(f'  printf("{f} %zu %zu\\n", sizeof(((pna_tower_drop_args*)0)->{f}), offsetof(pna_tower_drop_args, {f}));')
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
    assert re.search(r"class PnaTowerDropArgs\(_PnaArgs\)", open(os.path.join(ROOT, "INTEGRATION.md")).read()), \
        "INTEGRATION.md's generated mirrors lack the new struct"


def test_a_short_or_inconsistent_args_struct_is_refused():
    """PNA_E_INVALID before anything touches a device: a short struct, p outside [0, 1) or NaN, no base, an edge block around another base."""
    L = _lib.lib()
    L.pna_last_error.restype = ctypes.c_char_p
    cls = _lib.PnaTowerDropArgs
    for fn in (L.pna_tower_drop_train_fwd_f32, L.pna_tower_drop_train_bwd_f32):
        d = cls()
        assert d.struct_size == ctypes.sizeof(cls)
        for short in (0, ctypes.sizeof(cls) - 8):
            d.struct_size = short
            assert fn(ctypes.byref(d), None) == -1 and b"struct_size" in L.pna_last_error()
        base, other = _lib.PnaTowerTrainArgs(), _lib.PnaTowerTrainArgs()
        for p in (-0.1, 1.0, 1.5, float("nan"), float("inf")):
            d = cls()
            d.base, d.p = ctypes.cast(ctypes.pointer(base), ctypes.c_void_p), p
            assert fn(ctypes.byref(d), None) == -1 and b"0 <= p < 1" in L.pna_last_error(), p
        d = cls()
        d.p = 0.3
        assert fn(ctypes.byref(d), None) == -1 and b"pna_tower_drop_train" in L.pna_last_error()          # a NULL base
        q = _lib.PnaTowerEdgeTrainArgs()
        q.base, q.edge_dim = ctypes.cast(ctypes.pointer(other), ctypes.c_void_p), 3
        d.base, d.edge = ctypes.cast(ctypes.pointer(base), ctypes.c_void_p), ctypes.cast(ctypes.pointer(q), ctypes.c_void_p)
        assert fn(ctypes.byref(d), None) == -1 and b"edge->base == base" in L.pna_last_error()
        q.base, q.struct_size = d.base, ctypes.sizeof(_lib.PnaTowerEdgeTrainArgs) - 8
        assert fn(ctypes.byref(d), None) == -1 and b"struct_size" in L.pna_last_error()                    # a short edge block
        q.struct_size = ctypes.sizeof(_lib.PnaTowerEdgeTrainArgs)
        assert fn(ctypes.byref(d), None) == -1                                                             # consistent now; the empty base is out of scope
    out = (ctypes.c_float * 4)()
    for bad in (dict(p=1.0), dict(p=float("nan")), dict(p=-0.5), dict(C=0), dict(ld=1), dict(V=-1), dict(out=None)):
        kw = dict(out=ctypes.cast(out, ctypes.c_void_p), ld=2, V=2, C=2, p=0.5)
        kw.update(bad)
        assert L.pna_dropout_mask_f32(kw["out"], kw["ld"], kw["V"], kw["C"], kw["p"], 1, 0, None) == -1, bad
    assert L.pna_dropout_mask_f32(ctypes.cast(out, ctypes.c_void_p), 2, 0, 2, 0.5, 1, 0, None) == 0         # nothing to write: no launch


def test_masked_oracle_with_a_mask_of_ones_is_the_oracles_layer():
    """The restatement of tower_drop_train_cases with mask = 1 equals oracle.dgl_layer_forward in train mode (float64), with and without
    edge features; with a real mask it differs, and a dropped column of a row does not reach the output: the mixing Linear sees a zero."""
    for name in C.CASES:
        meta, a, sd, ref, key = C.case(name)
        sdd = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
        edge = meta["edge_dim"] > 0
        args = (a["src"], a["dst"], meta["N"], a["h"].double(), a["e"].double(), a["snorm_n"].double())
        run_a, run_b = {}, {}
        want = O.dgl_layer_forward(sdd, *args, C.AGGS, meta["scalers"].split(), a["avg_log"].double(), meta["towers"], meta["divide_input"], True, True,
                                   True, edge, running=run_a)
        got = C.masked_layer_forward(sdd, *args, meta["scalers"].split(), a["avg_log"].double(), meta["towers"], meta["divide_input"], edge, True,
                                     torch.ones(meta["N"], meta["out_dim"], dtype=torch.float64), run_b)
        assert torch.equal(got, want) and run_a.keys() == run_b.keys() and all(torch.equal(run_a[k], run_b[k]) for k in run_a)
        assert not torch.equal(ref.out, want if meta["residual"] else want - a["h"].double()) or key[0] == 0
        assert {k: v for k, v in ref.running.items()}.keys() == run_a.keys()
        for k in run_a:                                                             # BatchNorm sees the undropped rows
            assert torch.equal(ref.running[k], run_a[k])


@pytest.mark.parametrize("name", list(C.CASES))
def test_fp32_oracle_under_the_same_mask_is_inside_the_bars(name):
    """What the case seeds were picked for: the fp32 oracle alone, under the case's mask, passes the bars the GPU tests apply."""
    meta, a, sd, ref, key = C.case(name)
    assert float(ref.ill.sum()) / meta["N"] <= 0.15 and C.pmin_of(ref.out, a, meta) >= 1e-5
    r32 = ref.ref32
    C.check_step(meta, ref, r32["out"], r32["grad_h"], r32["grads"], r32["running"])
    if ref.grad_e is not None:
        C.check_grad_e(ref, r32["grad_e"])


def test_new_kernel_instantiations_use_no_scratch(tmp_path):
    """The recipe of tests/test_build_resources.py::test_no_kernel_uses_scratch on pna_tower_train.hip: both mixing kernels exist with and
    without dropout, the mask kernel is there, and no kernel of the file uses scratch."""
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
    assert len(names) == len(scratch) and len(names) >= 22
    assert sum("k_tt_mix_fwd" in n for n in names) == 2 and sum("k_tt_mix_bwd" in n for n in names) == 2
    assert any("k_dropout_mask" in n for n in names)
    bad = [(n, s) for n, s in zip(names, scratch) if s != 0]
    assert not bad, f"kernels using scratch: {bad}"
