"""Host side of the one-call training route of PNALayer FOR ANY LIST OF AGGREGATORS (no GPU): the knob, the route predicate clause by
clause (and the other three routes' predicates on such a layer), the exported symbols and their args struct, the argument checks that
need no device, the workspace query and functional.small_tower_aggr_train_fits, the fp32 oracle inside the bars on every case, the
per-edge message gradient kernel's instantiations."""
import ctypes
import importlib
import os
import re
import shutil
import subprocess

import pytest
import torch

import tower_aggr_train_cases as C
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


def _layer(aggs="sum", scalers="identity", dropout=0.0, edge_features=False, edge_dim=3, in_dim=24, out_dim=24, towers=4, **kw):
    return PNALayer(in_dim, out_dim, aggs, scalers, {"log": 1.0}, dropout, True, True, towers=towers, pretrans_layers=1, posttrans_layers=1,
                    divide_input=True, residual=True, edge_features=edge_features, edge_dim=edge_dim if edge_features else 0, **kw).train()


def test_route_is_off_by_default_and_read_from_the_environment(monkeypatch):
    monkeypatch.delenv("PNA_AMD_SMALL_TOWER_TRAIN_AGGR_ROWS", raising=False)
    try:
        assert importlib.reload(PF).SMALL_TOWER_TRAIN_AGGR_ROWS == 0
        monkeypatch.setenv("PNA_AMD_SMALL_TOWER_TRAIN_AGGR_ROWS", "4096")
        mod = importlib.reload(PF)
        assert mod.SMALL_TOWER_TRAIN_AGGR_ROWS == 4096
        assert mod.SMALL_TOWER_TRAIN_ROWS == 0 and mod.SMALL_TOWER_TRAIN_EDGE_ROWS == 0 and mod.SMALL_TOWER_TRAIN_DROPOUT_ROWS == 0
    finally:
        monkeypatch.delenv("PNA_AMD_SMALL_TOWER_TRAIN_AGGR_ROWS", raising=False)
        importlib.reload(PF)


def test_small_tower_aggr_train_path_clause_by_clause(monkeypatch):
    g, h, n, e = _graph(), _OnGpu(40, 24), _OnGpu(40, 1, requires_grad=False), _OnGpu(40, 3, requires_grad=False)
    assert g.csr.col.numel() == 40 and g.csr.max_degree == 1
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    assert not _layer()._small_tower_aggr_train_path(g, h, None, n)               # the knob at 0
    monkeypatch.setattr(PF, "SMALL_TOWER_TRAIN_AGGR_ROWS", 4096)
    # served: the MPNN rows, ablations, var, any order, with and without edge features and tower dropout
    for aggs in ("sum", "max", "mean", "std", "var", "mean sum max", "sum var min", "var mean", "mean min max std", "std min max mean", "min std sum max",
                 "mean sum max min", "sum var max min"):
        for scalers in ("identity", "identity amplification attenuation"):
            assert _layer(aggs, scalers)._small_tower_aggr_train_path(g, h, None, n), aggs
        assert _layer(aggs, edge_features=True)._small_tower_aggr_train_path(g, h, e, n), aggs
        assert _layer(aggs, dropout=0.2)._small_tower_aggr_train_path(g, h, None, n), aggs
        assert _layer(aggs, dropout=0.2, edge_features=True)._small_tower_aggr_train_path(g, h, e, n), aggs
    assert _layer("sum", in_dim=110, out_dim=80, towers=5)._small_tower_aggr_train_path(g, _OnGpu(40, 110), None, n)       # README:91, the last layer
    assert _layer("max", in_dim=110, out_dim=90, towers=5, edge_features=True, edge_dim=20, dropout=0.2)._small_tower_aggr_train_path(
        g, _OnGpu(40, 110), _OnGpu(40, 20), n)
    # the list: the standard one stays with the other three routes; five names; a repeated name; towers with different lists
    assert not _layer("mean max min std")._small_tower_aggr_train_path(g, h, None, n)
    assert not _layer("mean max min std", edge_features=True)._small_tower_aggr_train_path(g, h, e, n)
    assert not _layer("mean max min std", dropout=0.2)._small_tower_aggr_train_path(g, h, None, n)
    assert not _layer("mean sum max min std")._small_tower_aggr_train_path(g, h, None, n)
    assert not _layer("sum sum")._small_tower_aggr_train_path(g, h, None, n)
    assert not _layer("mean max sum max")._small_tower_aggr_train_path(g, h, None, n)
    assert not _layer("moment3")._small_tower_aggr_train_path(g, h, None, n)      # a name of the reference outside the six
    with pytest.raises(KeyError):
        _layer("median")                                                          # (an unknown name never becomes a layer: pna_layer.py:107-108)
    odd = _layer("sum max")
    odd.towers[1].aggregators = ["max", "sum"]
    assert not odd._small_tower_aggr_train_path(g, h, None, n)
    renamed = _layer("sum")
    for t in renamed.towers:
        t.aggregators = ["median"]
    assert not renamed._small_tower_aggr_train_path(g, h, None, n)                # a name the kernels do not know
    wrong = _layer("sum max")
    for t in wrong.towers:
        t.aggregators = ["sum"]                                                   # the posttrans weight is that of two aggregators
    assert not wrong._small_tower_aggr_train_path(g, h, None, n)
    # dropout: 0 everywhere or one 0 < p < 1; with p > 0 not while the stream is being captured
    assert not _layer(dropout=1.0)._small_tower_aggr_train_path(g, h, None, n)
    uneven = _layer(dropout=0.2)
    uneven.towers[2].dropout = 0.0
    assert not uneven._small_tower_aggr_train_path(g, h, None, n)
    uneven = _layer()
    uneven.towers[1].dropout = 0.2
    assert not uneven._small_tower_aggr_train_path(g, h, None, n)
    mixdrop = _layer()
    mixdrop.mixing_network.dropout = torch.nn.Dropout(0.2)
    assert not mixdrop._small_tower_aggr_train_path(g, h, None, n)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    assert not _layer(dropout=0.2)._small_tower_aggr_train_path(g, h, None, n)
    assert _layer()._small_tower_aggr_train_path(g, h, None, n)                   # (no key to draw: capture is fine)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    assert _layer(dropout=0.2)._small_tower_aggr_train_path(g, h, None, n)
    # the edge clauses apply when the layer has edge features, and only then
    assert not _layer(edge_features=True)._small_tower_aggr_train_path(g, h, None, n)
    assert not _layer(edge_features=True)._small_tower_aggr_train_path(g, h, _OnGpu(40, 4), n)
    assert not _layer(edge_features=True, edge_dim=65)._small_tower_aggr_train_path(g, h, _OnGpu(40, 65), n)
    assert _layer()._small_tower_aggr_train_path(g, h, e, n)                      # (a layer without edge features ignores e, as its forward does)
    # the shared clauses: a sample of them
    assert not _layer().eval()._small_tower_aggr_train_path(g, h, None, n)
    assert not _layer()._small_tower_aggr_train_path(g, _OnGpu(40, 24, torch.float64), None, n)
    assert not _layer()._small_tower_aggr_train_path(g, h, None, None)            # graph norm without its factor
    assert not _layer(in_dim=12, out_dim=24)._small_tower_aggr_train_path(g, _OnGpu(40, 12), None, n)                      # Fi = 3
    assert not _layer(in_dim=130, out_dim=130, towers=5)._small_tower_aggr_train_path(g, _OnGpu(40, 130), None, n)         # out_dim 130
    assert not _layer("sum", "identity amplification attenuation identity")._small_tower_aggr_train_path(g, h, None, n)   # four scalers
    frozen = _layer()
    for q in frozen.parameters():
        q.requires_grad_(False)
    assert not frozen._small_tower_aggr_train_path(g, _OnGpu(40, 24, requires_grad=False), None, n)
    monkeypatch.setattr(PF, "SMALL_TOWER_TRAIN_AGGR_ROWS", 39)
    assert not _layer()._small_tower_aggr_train_path(g, h, None, n)               # V above the knob
    monkeypatch.setattr(PF, "SMALL_TOWER_TRAIN_AGGR_ROWS", 0)
    for knob in ("SMALL_TOWER_TRAIN_ROWS", "SMALL_TOWER_TRAIN_EDGE_ROWS", "SMALL_TOWER_TRAIN_DROPOUT_ROWS"):
        monkeypatch.setattr(PF, knob, 4096)
    assert not _layer()._small_tower_aggr_train_path(g, h, None, n)               # the other routes' knobs do not open it


def test_the_four_routes_are_disjoint(monkeypatch):
    """With every knob on, a `sum` layer is refused by the three older predicates (with edge features and dropout too), and a standard
    layer by the new one; the existing pin -- "mean min max std" outside _small_tower_train_path -- stays true."""
    g, h, n, e = _graph(), _OnGpu(40, 24), _OnGpu(40, 1, requires_grad=False), _OnGpu(40, 3, requires_grad=False)
    assert g.csr.max_degree == 1
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    for knob in ("SMALL_TOWER_TRAIN_ROWS", "SMALL_TOWER_TRAIN_EDGE_ROWS", "SMALL_TOWER_TRAIN_DROPOUT_ROWS", "SMALL_TOWER_TRAIN_AGGR_ROWS"):
        monkeypatch.setattr(PF, knob, 4096)
    for aggs in ("sum", "max", "mean min max std", "var"):
        assert not _layer(aggs)._small_tower_train_path(g, h, n)
        assert not _layer(aggs, edge_features=True)._small_tower_train_edge_path(g, h, e, n)
        assert not _layer(aggs, dropout=0.2)._small_tower_drop_train_path(g, h, None, n)
        assert not _layer(aggs, dropout=0.2, edge_features=True)._small_tower_drop_train_path(g, h, e, n)
    std = "identity amplification attenuation"
    assert _layer("mean max min std", std)._small_tower_train_path(g, h, n)
    assert _layer("mean max min std", std, edge_features=True)._small_tower_train_edge_path(g, h, e, n)
    assert _layer("mean max min std", std, dropout=0.2)._small_tower_drop_train_path(g, h, None, n)
    for kw in (dict(), dict(edge_features=True), dict(dropout=0.2)):
        assert not _layer("mean max min std", std, **kw)._small_tower_aggr_train_path(g, h, e, n)


def test_symbols_are_declared_bound_and_the_struct_has_gccs_layout(tmp_path):
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "pna_amd.h")).read()
    for name in ("pna_tower_aggr_train_fwd_f32", "pna_tower_aggr_train_bwd_f32", "pna_tower_aggr_train_workspace_bytes"):
        assert hasattr(L, name), name
        assert re.search(r"\b(int|int64_t) " + name + r"\(", header), name
        assert getattr(L, name).argtypes is not None, name
    assert "pna_tower_aggr_train_args" in header and "23, additive: + pna_tower_aggr_train_fwd_f32" in header
    assert "models/dgl/aggregators.py:6-26, 50-51" in header and "realworld_benchmark/README.md:54 and :91-100" in header
    assert L.pna_abi_version() == _lib.PNA_ABI_VERSION == 23
    assert hasattr(AG, "TowerLayerAggrSmallTrainFn") and hasattr(PF, "small_tower_aggr_train_fits")
    cls = _lib.PnaTowerAggrTrainArgs
    assert [f for f, *_ in cls._fields_] == ["struct_size", "_abi_reserved", "base", "edge", "drop", "n_aggr", "aggr", "_pad0", "row_mean", "pos_t"]
    gcc = shutil.which("gcc")
    if gcc is None:
        return
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "pna_amd.h"', "int main(void) {", '  printf(". %zu 0\\n", sizeof(pna_tower_aggr_train_args));']
    for f, *_ in cls._fields_:
        lines.append(f'  printf("{f} %zu %zu\\n", sizeof(((pna_tower_aggr_train_args*)0)->{f}), offsetof(pna_tower_aggr_train_args, {f}));')
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
    assert re.search(r"class PnaTowerAggrTrainArgs\(_PnaArgs\)", open(os.path.join(ROOT, "INTEGRATION.md")).read()), \
        "INTEGRATION.md's generated mirrors lack the new struct"


def test_a_short_or_inconsistent_args_struct_is_refused():
    """PNA_E_INVALID before anything touches a device: a short struct, a bad list, no base, blocks around another base, a bad p."""
    L = _lib.lib()
    L.pna_last_error.restype = ctypes.c_char_p
    cls = _lib.PnaTowerAggrTrainArgs
    void = lambda x: ctypes.cast(ctypes.pointer(x), ctypes.c_void_p)   # noqa: E731
    for fn in (L.pna_tower_aggr_train_fwd_f32, L.pna_tower_aggr_train_bwd_f32):
        r = cls()
        assert r.struct_size == ctypes.sizeof(cls)
        for short in (0, ctypes.sizeof(cls) - 8):
            r.struct_size = short
            assert fn(ctypes.byref(r), None) == -1 and b"struct_size" in L.pna_last_error()
        base, other = _lib.PnaTowerTrainArgs(), _lib.PnaTowerTrainArgs()
        for codes in ((), (1, 1), (0, 1, 2, 3, 4), (6,), (-1,), (2, 3, 2)):
            r = cls()
            r.base, r.n_aggr = void(base), len(codes)
            for i, c in enumerate(codes):
                r.aggr[i] = c
            assert fn(ctypes.byref(r), None) == -1 and b"1 <= n_aggr <= 4 distinct codes" in L.pna_last_error(), codes
        r = cls()
        r.n_aggr, r.aggr[0] = 1, 1
        assert fn(ctypes.byref(r), None) == -1 and b"pna_tower_aggr_train" in L.pna_last_error()           # a NULL base
        q = _lib.PnaTowerEdgeTrainArgs()
        q.base, q.edge_dim = void(other), 3
        r.base, r.edge = void(base), void(q)
        assert fn(ctypes.byref(r), None) == -1 and b"edge->base == base" in L.pna_last_error()
        q.base, q.struct_size = r.base, ctypes.sizeof(_lib.PnaTowerEdgeTrainArgs) - 8
        assert fn(ctypes.byref(r), None) == -1 and b"struct_size" in L.pna_last_error()                    # a short edge block
        q.struct_size = ctypes.sizeof(_lib.PnaTowerEdgeTrainArgs)
        d = _lib.PnaTowerDropArgs()
        d.base, d.p = r.base, 0.2                                                                          # d.edge NULL, r.edge not
        r.drop = void(d)
        assert fn(ctypes.byref(r), None) == -1 and b"drop->edge == edge" in L.pna_last_error()
        d.edge = r.edge
        for p in (-0.1, 1.0, float("nan")):
            d.p = p
            assert fn(ctypes.byref(r), None) == -1 and b"0 <= p < 1" in L.pna_last_error()
        d.p, d.struct_size = 0.2, ctypes.sizeof(_lib.PnaTowerDropArgs) - 8
        assert fn(ctypes.byref(r), None) == -1 and b"struct_size" in L.pna_last_error()                    # a short drop block
        d.struct_size = ctypes.sizeof(_lib.PnaTowerDropArgs)
        assert fn(ctypes.byref(r), None) == -1                                                             # consistent now; the empty base is out of scope


def _codes(*names):
    return (ctypes.c_int32 * len(names))(*[_lib.AGG_CODES[n] for n in names])


def test_workspace_bytes_is_monotone_refuses_what_is_outside_the_scope_and_fits_agrees():
    ws = _lib.lib().pna_tower_aggr_train_workspace_bytes
    for T, Fi, Fo, S, div, ed, names in ((5, 22, 16, 1, 1, 0, ("sum",)), (5, 22, 16, 1, 1, 40, ("max",)), (4, 6, 6, 3, 1, 0, ("mean", "min", "max", "std")),
                                         (1, 128, 8, 3, 0, 0, ("min", "std", "sum", "max")), (2, 12, 6, 2, 0, 64, ("sum", "var", "min"))):
        arr = _codes(*names)
        sizes = [ws(V, 4 * V, T, Fi, Fo, S, div, ed, len(names), arr) for V in (2, 15, 16, 17, 250, 400, 4096, 65536, 65537, 200000)]
        assert all(s > 0 and s % 256 == 0 for s in sizes)
        assert sizes == sorted(sizes) and sizes[0] < sizes[-1]
        by_e = [ws(400, E, T, Fi, Fo, S, div, ed, len(names), arr) for E in (0, 1, 4000, 400000)]
        assert by_e == sorted(by_e) and by_e[0] < by_e[-1]                        # (the per-edge message gradient lives there, with or without e)
    one = _codes("sum")
    assert ws(400, 10, 4, 6, 6, 3, 1, 0, 1, one) > 0
    for args in ((1, 0, 4, 6, 6, 3, 1, 0), (400, -1, 4, 6, 6, 3, 1, 0), (400, 10, 0, 6, 6, 3, 1, 0), (400, 10, 9, 6, 6, 3, 1, 0), (400, 10, 4, 3, 6, 3, 1, 0),
                 (400, 10, 4, 130, 6, 3, 1, 0), (400, 10, 1, 129, 6, 3, 0, 0), (400, 10, 4, 6, 0, 3, 1, 0), (400, 10, 4, 6, 33, 3, 1, 0), (400, 10, 4, 6, 6, 0, 1, 0),
                 (400, 10, 4, 6, 6, 4, 1, 0), (400, 10, 4, 6, 6, 3, 2, 0), (400, 10, 4, 6, 6, 3, 1, -1), (400, 10, 4, 6, 6, 3, 1, 65)):
        assert ws(*args, 1, one) == -1, args
    ok = (400, 10, 4, 6, 6, 3, 1, 0)
    assert ws(*ok, 0, one) == -1 and ws(*ok, 5, _codes("mean", "sum", "max", "min", "std")) == -1 and ws(*ok, 1, None) == -1
    assert ws(*ok, 2, _codes("sum", "sum")) == -1 and ws(*ok, 1, (ctypes.c_int32 * 1)(6)) == -1 and ws(*ok, 1, (ctypes.c_int32 * 1)(-1)) == -1
    # a shorter list never needs more than a longer one of the same shape
    assert ws(*ok, 1, one) <= ws(*ok, 2, _codes("sum", "var")) <= ws(*ok, 4, _codes("sum", "var", "max", "min"))
    for T in (0, 1, 5, 8, 9):
        for Fi in (3, 4, 22, 65, 128, 129):
            for Fo in (0, 1, 16, 26, 128, 129):
                for S in (0, 1, 3, 4):
                    for ed in (-1, 0, 1, 64, 65):
                        for codes in ((1,), (2, 5), (0, 3, 2, 4), (1, 1), (6,), (), (0, 1, 2, 3, 4)):
                            want = (1 <= T <= 8 and 4 <= Fi <= 128 and T * Fi <= 512 and 1 <= Fo and T * Fo <= 128 and 1 <= S <= 3 and 0 <= ed <= 64
                                    and 1 <= len(codes) <= 4 and len(set(codes)) == len(codes) and all(0 <= c <= 5 for c in codes))
                            arr = (ctypes.c_int32 * max(len(codes), 1))(*codes)
                            got = ws(400, 1000, T, Fi, Fo, S, 1, ed, len(codes), arr) >= 0
                            assert PF.small_tower_aggr_train_fits(T, Fi, Fo, S, ed, codes) == want == got, (T, Fi, Fo, S, ed, codes)


@pytest.mark.parametrize("name", list(C.RANDOM) + list(C.DROP))
def test_fp32_oracle_alone_is_inside_the_bars(name):
    """What the case seeds and keys were picked for: the two caps hold and the fp32 oracle, under the case's mask, passes the bars the GPU
    tests apply."""
    meta, a, sd, ref, key = C.case(name)
    assert float(ref.ill.sum()) / meta["N"] <= 0.15 and C.pmin_of(ref.out, a, meta) >= 1e-5
    r32 = ref.ref32
    C.check_step(meta, ref, r32["out"], r32["grad_h"], r32["grads"], r32["running"])
    if ref.grad_e is not None:
        C.check_grad_e(ref, r32["grad_e"])
    assert (key is None) == (ref.mask is None)


def test_the_oracle_step_without_a_mask_is_the_masked_one_under_ones():
    """masked_layer_forward with a mask of ones is oracle.dgl_layer_train_step for the case's list (float64), with and without edges."""
    for name in ("sum_var_min", "edge3_sum"):
        meta, a, sd, ref, _ = C.case(name)
        out, gh, ge, gp, run = C._step(sd, a, meta, torch.float64, torch.ones(meta["N"], meta["out_dim"], dtype=torch.float64))
        assert torch.equal(out, ref.out) and torch.equal(gh, ref.grad_h) and all(torch.equal(gp[k], ref.grads[k]) for k in gp)
        assert run.keys() == ref.running.keys() and all(torch.equal(run[k], ref.running[k]) for k in run)


def test_message_gradient_kernel_has_both_instantiations_and_no_scratch(tmp_path):
    """The recipe of tests/test_build_resources.py::test_no_kernel_uses_scratch on pna_tower_train.hip: the per-edge message gradient exists
    with and without the x_edge term, the pull and every other kernel of the file are there, and none uses scratch."""
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
    assert len(names) == len(scratch) and len(names) >= 23
    assert sum("k_tt_edge_dm" in n for n in names) == 2 and sum("k_tt_edge_pull" in n for n in names) == 1
    assert sum("k_tt_rows_fwd" in n for n in names) == 6 and sum("k_tt_rows_bwd" in n for n in names) == 3
    bad = [(n, s) for n, s in zip(names, scratch) if s != 0]
    assert not bad, f"kernels using scratch: {bad}"
