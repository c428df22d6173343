"""The binding of pna_pyg_conv_train_* (symbols, the args struct's size and offsets against the header compiled on the host, the
workspace query's scope, the ABI number) and PNAConv._one_call_path on CPU modules.  No GPU."""
import ctypes
import os
import shutil
import subprocess

import pytest
import torch

from pna_amd import _lib, functional as PF
from pna_amd.pytorch_geometric import PNAConv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["struct_size", "_abi_reserved", "aggr", "w_pre", "b_pre", "w_enc", "b_enc", "packed", "grad_w_pre", "grad_b_pre", "grad_w_enc", "grad_b_enc"]
A4 = [_lib.AGG_CODES[n] for n in ("mean", "min", "max", "std")]


def _bytes(V, E, T, Fi, Fo, S, div, ed, codes):
    arr = (ctypes.c_int32 * max(len(codes), 1))(*codes)
    return _lib.lib().pna_pyg_conv_train_workspace_bytes(V, E, T, Fi, Fo, S, div, ed, len(codes), arr)


def test_symbols_and_abi_version():
    L = _lib.lib()
    for name in ("pna_pyg_conv_train_workspace_bytes", "pna_pyg_conv_train_fwd_f32", "pna_pyg_conv_train_bwd_f32"):
        assert hasattr(L, name), name
    assert L.pna_abi_version() == 23


def test_struct_mirror_matches_the_header(tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not available")
    cls = _lib.PnaPygConvTrainArgs
    assert [n for n, *_ in cls._fields_] == FIELDS and cls._fields_[0][0] == "struct_size"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "pna_amd.h"', "int main(void) {",
             '  printf(". %zu 0\\n", sizeof(pna_pyg_conv_train_args));']
    for f in FIELDS:
        lines.append(f'  printf("{f} %zu %zu\\n", sizeof(((pna_pyg_conv_train_args*)0)->{f}), offsetof(pna_pyg_conv_train_args, {f}));')
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run([gcc, "-std=c11", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True)
    rows = {r.split()[0]: (int(r.split()[1]), int(r.split()[2])) for r in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()}
    assert ctypes.sizeof(cls) == rows["."][0]
    for f in FIELDS:
        d = getattr(cls, f)
        assert (d.size, d.offset) == rows[f], (f, (d.size, d.offset), rows[f])
    assert _lib.PnaPygConvTrainArgs().struct_size == ctypes.sizeof(cls)


def test_workspace_query_is_minus_one_outside_the_scope():
    assert _bytes(45, 100, 5, 75, 15, 3, 0, 50, A4) > _bytes(45, 100, 5, 75, 15, 3, 0, 0, A4) > 0
    tower = _lib.lib().pna_tower_aggr_train_workspace_bytes(45, 100, 5, 75, 15, 3, 0, 50, 4, (ctypes.c_int32 * 4)(*A4))
    assert _bytes(45, 100, 5, 75, 15, 3, 0, 50, A4) >= tower + 4 * 5 * 75 * (2 * 75 + 50 + 1)      # + the image's gradient
    assert _bytes(2, 0, 1, 4, 1, 1, 0, 0, [1]) > 0
    for bad in [(1, 0, 1, 4, 1, 1, 0, 0, A4), (45, 100, 9, 8, 8, 1, 0, 0, A4), (45, 100, 1, 3, 8, 1, 0, 0, A4), (45, 100, 1, 129, 8, 1, 0, 0, A4),
                (45, 100, 5, 128, 8, 1, 0, 0, A4), (45, 100, 2, 8, 65, 1, 0, 0, A4), (45, 100, 1, 8, 8, 4, 0, 0, A4), (45, 100, 1, 8, 8, 0, 0, 0, A4),
                (45, 100, 1, 8, 8, 1, 0, 65, A4), (45, 100, 1, 8, 8, 1, 0, -1, A4), (45, 100, 1, 8, 8, 1, 0, 0, []), (45, 100, 1, 8, 8, 1, 0, 0, [0, 0]),
                (45, 100, 1, 8, 8, 1, 0, 0, [0, 1, 2, 3, 4]), (45, 100, 1, 8, 8, 1, 0, 0, [6]), (45, 100, 1, 8, 8, 1, 2, 0, A4)]:
        assert _bytes(*bad) == -1, bad
    assert PF.pyg_conv_train_fits(5, 75, 15, 3, 50, A4) and not PF.pyg_conv_train_fits(5, 75, 15, 3, 65, A4)


def test_null_and_short_structs_are_refused_without_a_device():
    L = _lib.lib()
    assert L.pna_pyg_conv_train_fwd_f32(None, None) != 0
    y = _lib.PnaPygConvTrainArgs()
    y.struct_size -= 8
    assert L.pna_pyg_conv_train_fwd_f32(ctypes.byref(y), None) != 0 and L.pna_pyg_conv_train_bwd_f32(ctypes.byref(y), None) != 0
    y = _lib.PnaPygConvTrainArgs()                          # aggr == NULL
    assert L.pna_pyg_conv_train_bwd_f32(ctypes.byref(y), None) != 0
    assert b"pna_pyg_conv_train_bwd_f32" in L.pna_last_error()


def test_the_knob_is_off_by_default_and_the_predicate_declines_cpu_calls(monkeypatch):
    assert os.environ.get("PNA_AMD_PYG_TRAIN_ROWS") is not None or PF.PYG_TRAIN_ROWS == 0
    deg = torch.tensor([2, 5, 3])
    layer = PNAConv(8, 8, ["mean", "max"], ["identity"], deg, towers=2)
    x = torch.randn(10, 8)
    monkeypatch.setattr(PF, "PYG_TRAIN_ROWS", 0)
    assert layer._one_call_path(x) is False
    monkeypatch.setattr(PF, "PYG_TRAIN_ROWS", 4096)
    assert layer._one_call_path(x) is False                 # CPU tensors: the code the call took before (which refuses them itself)
    assert layer._one_call_path(x.to(torch.bfloat16)) is False
    assert PNAConv(8, 8, ["mean"], ["identity"], deg, edge_dim=4)._one_call_path(x, None) is False


def test_row_factors_are_memoised_on_the_graph_per_scaler_list_and_avg_deg():
    from pna_amd.graph import Graph
    from pna_amd.pytorch_geometric.pna import _row_factors
    g = Graph(torch.tensor([0, 1, 2, 2]), torch.tensor([1, 2, 0, 1]), 4)          # node 3 has no in-edge
    avg = {"lin": 1.0, "log": 0.5, "exp": 3.0}
    f1, d1 = _row_factors(g, ["identity", "attenuation", "inverse_linear"], avg)
    f2, d2 = _row_factors(g, ["identity", "attenuation", "inverse_linear"], dict(avg))
    assert f1[0] is None and f1[1] is f2[1] and f1[2] is f2[2] and d1 is d2        # layers 2..L of a net launch nothing
    assert d1.tolist() == [1.0, 2.0, 1.0, 0.0] and f1[1][3] == 1 and f1[2][3] == 1  # the deg == 0 rules (scalers.py:16-19, 26-29)
    f3, _ = _row_factors(g, ["identity", "attenuation", "inverse_linear"], dict(avg, lin=2.0))
    assert f3[2] is not f1[2] and torch.equal(f3[2][:3], 2 * f1[2][:3])
    f4, _ = _row_factors(g, ["linear"], avg)
    assert torch.equal(f4[0], d1)
