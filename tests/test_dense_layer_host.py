"""Host side of the one-call dense PNALayer (no GPU): the knob, the route predicate clause by clause, the exported symbols with the struct's
layout and the scope checks, the LDS and workspace formulas against their Python mirrors, the compiler's resource report of
pna_dense_layer.hip, and the cap that keeps the GPU tests' bar honest: for every case of tests/dense_layer_cases.py the fp32 oracle's own
bar stays under 1e-4 max|ref64| on every tensor."""
import ctypes
import importlib
import os
import re
import shutil
import subprocess

import pytest
import torch
import torch.nn as nn

import dense_layer_cases as C
from pna_amd import _lib
from pna_amd import functional as PF
from pna_amd.pytorch.pna.layer import PNALayer, PNATower

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pna_amd", "csrc")


# ---- the references and the bars ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.NAMES)
def test_the_fp32_oracle_alone_keeps_every_bar_under_the_cap(name):
    ref64, ref32, bars = C.references(name)
    cap = C.cap_of(ref64)
    assert all(torch.isfinite(v).all() for v in ref64.values()) and all(torch.isfinite(v).all() for v in ref32.values())
    worst = max(((bars[k] / cap[k]) if cap[k] > 0 else 0.0, k) for k in bars)
    print("DENSE_BAR_OVER_CAP", name, round(worst[0], 3), worst[1])
    assert set(ref64) == {"out", "x"} | set(C.dense_case(name)["sd"])
    for k in bars:
        assert bars[k] <= cap[k], (k, bars[k], cap[k])


def test_case_list_covers_what_it_promises():
    cases = [C.dense_case(n) for n in C.NAMES]
    assert {c["N"] for c in cases} >= {1, 2, 15, 16, 17, 64, 65, 128}
    slab = _lib.PNA_DENSE_MAX_SLABS
    assert {c["B"] for c in cases} >= {1, 3, slab + 1} and -(-(slab + 1) // slab) == 2 and -(-slab // slab) == 1   # graphs per slab
    assert {(c["T"], c["Fi"], c["Fo"]) for c in cases} >= {(1, 1, 1), (4, 2, 4), (4, 4, 4), (3, 5, 7), (8, 8, 8), (1, 64, 64)}
    assert {c["divide_input"] for c in cases} == {True, False} == {c["self_loop"] for c in cases}
    assert {" ".join(c["aggregators"]) for c in cases} == {"mean max min std", "std min", "max"}
    assert {len(c["scalers"]) for c in cases} == {1, 2, 3}
    assert any("linear" in c["scalers"] for c in cases) and any("inverse_linear" in c["scalers"] for c in cases)
    assert C.dense_case("n1")["self_loop"]
    w = C.dense_case("n65")["adj"]
    assert (w >= 0).all() and ((w != 0) & (w != w.round())).any()                  # positive, non-integer weights
    neg = C.dense_case("neg")["adj"]
    assert (neg < 0).sum() == neg.shape[0] and (neg.sum(-1) > 0.2).all()
    for c in cases:
        a = c["adj"] + torch.eye(c["N"]) if c["self_loop"] else c["adj"]
        assert (a != 0).any(dim=2).all() and (a > 0).any(dim=1).all(), c["name"]    # every row and every column has an entry
        assert PF.dense_layer_fits(c["N"], c["T"], c["Fi"], c["Fo"], len(c["aggregators"]), len(c["scalers"])), c["name"]
    big = C.dense_case("n128")
    assert PF.dense_layer_lds_bytes(128, 4, 4, 4, 4, 3) > 160 * 1024 - 1024 and big["N"] == 128   # the case at the LDS edge


def test_float64_reference_is_the_existing_cpu_restatement_of_the_goldens():
    """The reference the cases use is the function the repository's dense goldens were checked against (tests/test_oracle_golden.py)."""
    from conftest import load_golden
    from oracle import torch_oracle as TO
    meta, a, sd = load_golden("dense_self_loop")
    out = TO.dense_layer_forward(sd, a["x"], a["adj"], meta["aggregators"], meta["scalers"], {"log": a["avg_log"], "lin": a["avg_lin"]},
                                 meta["towers"], meta["divide_input"], meta["self_loop"])
    torch.testing.assert_close(out, a["out"], rtol=1e-4, atol=1e-5)


# ---- the knob and the predicate ----------------------------------------------------------------------------------------------------
def test_route_is_off_by_default_and_read_from_the_environment(monkeypatch):
    monkeypatch.delenv("PNA_AMD_DENSE_LAYER_ROWS", raising=False)
    try:
        assert importlib.reload(PF).DENSE_LAYER_ROWS == 0
        monkeypatch.setenv("PNA_AMD_DENSE_LAYER_ROWS", "4096")
        assert importlib.reload(PF).DENSE_LAYER_ROWS == 4096
    finally:
        monkeypatch.delenv("PNA_AMD_DENSE_LAYER_ROWS", raising=False)
        importlib.reload(PF)


class _OnGpu:
    """A stand-in for a tensor on the GPU (the predicate reads shape, dtype, is_cuda, device, dim, is_contiguous and requires_grad)."""

    def __init__(self, *shape, dtype=torch.float32, contiguous=True, requires_grad=False):
        self.shape, self.dtype, self.is_cuda, self.device = torch.Size(shape), dtype, True, torch.device("cpu")
        self._c, self.requires_grad = contiguous, requires_grad

    def dim(self):
        return len(self.shape)

    def is_contiguous(self):
        return self._c


def _layer(fin=16, fout=16, aggs="mean max min std", scalers="identity amplification attenuation", **kw):
    kw.setdefault("towers", 4)
    return PNALayer(fin, fout, aggs.split(), scalers.split(), C.AVG_D, **kw)


def test_one_call_path_clause_by_clause(monkeypatch):
    x, adj = _OnGpu(16, 15, 16), _OnGpu(16, 15, 15)
    monkeypatch.setattr(PF, "DENSE_LAYER_ROWS", 0)
    assert not _layer()._one_call_path(None, None)                                # the knob at 0: nothing is looked at
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))     # the parameters' residency without a GPU
    assert not _layer()._one_call_path(x, adj)
    monkeypatch.setattr(PF, "DENSE_LAYER_ROWS", 4096)
    assert _layer()._one_call_path(x, adj)
    assert _layer().eval()._one_call_path(x, adj)                                 # train and eval alike
    assert _layer(2, 16, divide_input=False)._one_call_path(_OnGpu(16, 15, 2), adj)          # the multitask first layer
    assert _layer(self_loop=True)._one_call_path(x, adj)
    assert _layer(aggs="std min", scalers="linear inverse_linear")._one_call_path(x, adj)
    assert _layer(aggs="max", scalers="identity", towers=1)._one_call_path(x, adj)
    # the rows
    monkeypatch.setattr(PF, "DENSE_LAYER_ROWS", 16 * 15 - 1)
    assert not _layer()._one_call_path(x, adj)                                    # more rows than the knob covers
    monkeypatch.setattr(PF, "DENSE_LAYER_ROWS", 16 * 15)
    assert _layer()._one_call_path(x, adj)
    monkeypatch.setattr(PF, "DENSE_LAYER_ROWS", 1 << 20)
    # the tensors
    assert not _layer()._one_call_path(_OnGpu(240, 16), adj) and not _layer()._one_call_path(x, _OnGpu(16, 225))
    assert not _layer()._one_call_path(x, _OnGpu(15, 15, 15)) and not _layer()._one_call_path(x, _OnGpu(16, 15, 14))
    assert not _layer()._one_call_path(x, _OnGpu(16, 14, 14)) and not _layer()._one_call_path(_OnGpu(16, 15, 8), adj)
    assert not _layer()._one_call_path(_OnGpu(16, 15, 16, dtype=torch.float64), adj)
    assert not _layer()._one_call_path(x, _OnGpu(16, 15, 15, dtype=torch.bfloat16))
    assert not _layer()._one_call_path(_OnGpu(16, 15, 16, contiguous=False), adj)
    assert not _layer()._one_call_path(x, _OnGpu(16, 15, 15, contiguous=False))
    assert not _layer()._one_call_path(x, _OnGpu(16, 15, 15, requires_grad=True))   # adj gets no gradient from the call
    assert _layer()._one_call_path(_OnGpu(16, 15, 16, requires_grad=True), adj)
    cpu = _OnGpu(16, 15, 16)
    cpu.is_cuda = False
    assert not _layer()._one_call_path(cpu, adj)
    other = _OnGpu(16, 15, 15)
    other.device = torch.device("meta")
    assert not _layer()._one_call_path(x, other)                                  # not on input's device
    # the towers
    assert not _layer(pretrans_layers=2)._one_call_path(x, adj) and not _layer(posttrans_layers=2)._one_call_path(x, adj)
    # aggregators and scalers
    assert not _layer(aggs="mean sum")._one_call_path(x, adj) and not _layer(aggs="mean var")._one_call_path(x, adj)
    assert not _layer(aggs="mean mean")._one_call_path(x, adj) and not _layer(aggs="softmax")._one_call_path(x, adj)
    assert not _layer(scalers="identity identity")._one_call_path(x, adj)
    assert not _layer(scalers="identity amplification attenuation linear")._one_call_path(x, adj)
    # the parameters
    assert not _layer().double()._one_call_path(x, adj)
    one = _layer()
    one.towers[2].posttrans.fully_connected[0].linear.bias.data = one.towers[2].posttrans.fully_connected[0].linear.bias.data.double()
    assert not one._one_call_path(x, adj)
    # the mixing network
    for attr, value in (("activation", nn.ReLU()), ("dropout", nn.Dropout(0.1)), ("b_norm", nn.BatchNorm1d(16))):
        odd = _layer()
        setattr(odd.mixing_network, attr, value)
        assert not odd._one_call_path(x, adj), attr
    nobias = _layer()
    nobias.mixing_network.linear = nn.Linear(16, 16, bias=False)
    assert not nobias._one_call_path(x, adj)
    # the shape's fit
    assert _layer()._one_call_path(_OnGpu(2, 128, 16), _OnGpu(2, 128, 128))
    assert not _layer()._one_call_path(_OnGpu(2, 129, 16), _OnGpu(2, 129, 129))
    assert not _layer(64, 64, towers=8)._one_call_path(_OnGpu(2, 64, 64), _OnGpu(2, 64, 64))   # 8 x 8 towers, four aggregators: over the LDS
    assert _layer(64, 64, towers=8, aggs="max", scalers="identity")._one_call_path(_OnGpu(2, 64, 64), _OnGpu(2, 64, 64))
    assert not _layer(128, 128, towers=8)._one_call_path(_OnGpu(2, 4, 128), _OnGpu(2, 4, 4))   # T Fi = 128
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: False))
    assert not _layer()._one_call_path(x, adj)                                    # parameters on the host


def test_a_bare_tower_has_no_one_call_route():
    assert not hasattr(PNATower, "_one_call_path")


def test_fits_and_lds_bytes_equal_the_kernels_own_check():
    L = _lib.lib()
    for N in (1, 2, 15, 16, 17, 64, 65, 97, 100, 127, 128):
        for T, Fi, Fo in ((1, 1, 1), (4, 2, 4), (4, 4, 4), (3, 5, 7), (8, 8, 8), (1, 64, 64), (2, 32, 1), (8, 1, 8)):
            for A in (1, 2, 4):
                for S in (1, 3):
                    TF, C2 = T * Fi, T * Fo                                         # (the test's own statement of layout())
                    want = 4 * N * ((N | 1) + 5 * TF + A * TF + 2 * C2 + 3 + S) + (2 * N * TF + 15) // 16 * 16
                    assert L.pna_dense_layer_lds_bytes(N, T, Fi, Fo, A, S) == want == PF.dense_layer_lds_bytes(N, T, Fi, Fo, A, S) > 0
                    fits = want <= 160 * 1024
                    assert PF.dense_layer_fits(N, T, Fi, Fo, A, S) == fits == (L.pna_dense_layer_workspace_bytes(1, N, T, Fi, Fo, A, S) > 0)
    for bad in ((0, 1, 1, 1, 1, 1), (129, 1, 1, 1, 1, 1), (8, 0, 1, 1, 1, 1), (8, 9, 1, 1, 1, 1), (8, 1, 0, 1, 1, 1), (8, 1, 65, 1, 1, 1),
                (8, 2, 33, 1, 1, 1), (8, 1, 1, 0, 1, 1), (8, 2, 1, 33, 1, 1), (8, 1, 1, 1, 0, 1), (8, 1, 1, 1, 5, 1), (8, 1, 1, 1, 1, 0),
                (8, 1, 1, 1, 1, 4)):
        assert L.pna_dense_layer_lds_bytes(*bad) == -1 == PF.dense_layer_lds_bytes(*bad) and not PF.dense_layer_fits(*bad), bad


def test_workspace_bytes_are_monotone_and_equal_the_mirror():
    L = _lib.lib()
    slab = _lib.PNA_DENSE_MAX_SLABS
    for N, T, Fi, Fo, A, S in ((15, 4, 2, 4, 4, 3), (25, 4, 4, 4, 4, 3), (17, 1, 64, 64, 4, 3), (2, 3, 5, 7, 2, 2), (128, 1, 1, 1, 1, 1)):
        last = 0
        for B in (1, 2, 3, slab - 1, slab, slab + 1, 2 * slab, 2 * slab + 1, 10 * slab + 7, 10 ** 6):
            n_slab = -(-B // -(-B // slab))                                         # ceil(B / slab) graphs per slab
            assert n_slab <= min(B, slab)                                           # the slabs in use never outnumber the images
            C2 = T * Fo
            want = min(B, slab) * (T * (2 * Fi * Fi + Fi + Fo * (1 + A * S) * Fi + Fo) + C2 * C2 + C2) * 4
            assert L.pna_dense_layer_workspace_bytes(B, N, T, Fi, Fo, A, S) == want == PF.dense_layer_workspace_bytes(B, N, T, Fi, Fo, A, S)
            assert want >= last                                                     # monotone in B
            last = want
    for args in ((0, 8, 1, 1, 1, 1, 1), (2 ** 24, 128, 1, 1, 1, 1, 1), (1, 129, 1, 1, 1, 1, 1), (1, 0, 1, 1, 1, 1, 1), (1, 8, 9, 1, 1, 1, 1),
                 (1, 8, 2, 33, 1, 1, 1), (1, 8, 1, 1, 65, 1, 1), (1, 8, 1, 1, 1, 5, 1), (1, 8, 1, 1, 1, 1, 4), (1, 64, 8, 8, 8, 4, 3)):
        assert L.pna_dense_layer_workspace_bytes(*args) == -1 == PF.dense_layer_workspace_bytes(*args), args


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_short_structs_are_refused():
    L = _lib.lib()
    for name in ("pna_dense_layer_fwd_f32", "pna_dense_layer_bwd_f32", "pna_dense_layer_workspace_bytes", "pna_dense_layer_lds_bytes"):
        assert hasattr(L, name), name
    assert L.pna_abi_version() == _lib.PNA_ABI_VERSION == 23
    header = open(os.path.join(ROOT, "include", "pna_amd.h")).read()
    assert "23, additive: + pna_dense_layer_fwd_f32" in header
    for cite in ("models/pytorch/pna/layer.py:33-49,99-109", "aggregators.py:17-73", "scalers.py:7-38"):
        assert cite in header, cite
    cls = _lib.PnaDenseLayerArgs
    for fn in (L.pna_dense_layer_fwd_f32, L.pna_dense_layer_bwd_f32):
        a = cls()
        assert a.struct_size == ctypes.sizeof(cls)
        for short in (0, ctypes.sizeof(cls) - 8):
            a.struct_size = short
            assert fn(ctypes.byref(a), None) == -1 and b"struct_size" in L.pna_last_error()
        a.struct_size = ctypes.sizeof(cls)
        assert fn(ctypes.byref(a), None) == -1 and b"struct_size" not in L.pna_last_error()              # all-zero: outside the scope
        assert fn(None, None) == -1
    assert re.search(r"class PnaDenseLayerArgs\(_PnaArgs\)", open(os.path.join(ROOT, "INTEGRATION.md")).read())


def test_the_struct_and_its_constants_have_gccs_layout(tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not available")
    cls = _lib.PnaDenseLayerArgs
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "pna_amd.h"', "int main(void) {",
             '  printf("PnaDenseLayerArgs . %zu 0\\n", sizeof(pna_dense_layer_args));']
    for f, *_ in cls._fields_:
        lines.append(f'  printf("PnaDenseLayerArgs {f} %zu %zu\\n", sizeof(((pna_dense_layer_args*)0)->{f}), offsetof(pna_dense_layer_args, {f}));')
    lines += ['  printf("consts %d %d %d\\n", PNA_DENSE_MAX_NODES, PNA_DENSE_MAX_SLABS, PNA_MAX_TOWER);',
              '  printf("scalers %d %d %d %d %d\\n", PNA_DENSE_SCALER_IDENTITY, PNA_DENSE_SCALER_AMPLIFICATION, PNA_DENSE_SCALER_ATTENUATION,'
              ' PNA_DENSE_SCALER_LINEAR, PNA_DENSE_SCALER_INVERSE_LINEAR);', "  return 0;", "}"]
    src, exe = tmp_path / "l.c", tmp_path / "l"
    src.write_text("\n".join(lines))
    subprocess.run([gcc, "-std=c11", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True)
    for row in (l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()):
        if row[0] == "consts":
            assert [int(v) for v in row[1:]] == [_lib.PNA_DENSE_MAX_NODES, _lib.PNA_DENSE_MAX_SLABS, _lib.PNA_MAX_TOWER]
        elif row[0] == "scalers":
            assert [int(v) for v in row[1:]] == [_lib.DENSE_SCALER_CODES[n] for n in ("identity", "amplification", "attenuation", "linear", "inverse_linear")]
        elif row[1] == ".":
            assert ctypes.sizeof(cls) == int(row[2])
        else:
            fld = getattr(cls, row[1])
            assert (fld.size, fld.offset) == (int(row[2]), int(row[3])), row


# ---- the compiler's report ---------------------------------------------------------------------------------------------------------------
def test_no_kernel_of_the_file_uses_scratch(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
           "-S", "--cuda-device-only", "-o", str(tmp_path / "out.s"), os.path.join(CSRC, "pna_dense_layer.hip"), "-Rpass-analysis=kernel-resource-usage"]
    out = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    names = re.findall(r"Function Name: (\S+)", out)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", out)]
    assert len(names) == len(scratch) == 3, names
    for k in ("k_dense_layer_fwd", "k_dense_layer_bwd", "k_dense_layer_final"):
        assert any(k in n for n in names), k
    assert not [(n, s) for n, s in zip(names, scratch) if s != 0]
    text = open(str(tmp_path / "out.s")).read()
    assert "atomic" not in text                                                      # no atomics of any kind


# ---- the avg_d scalars --------------------------------------------------------------------------------------------------------------------
def test_avg_d_scalars_are_passed_or_built_per_call_and_never_cached():
    """A 1-element fp32 tensor on the call's device is passed as it is; a Python number or another tensor becomes a fresh fp32 scalar
    that follows its source at once, and the route leaves no cached operand on the layer or on the tensor."""
    from pna_amd import autograd as AG
    dev = torch.device("cpu")
    here = torch.tensor(1.25)
    assert AG._dense_avg(here, dev).data_ptr() == here.data_ptr()
    a = AG._dense_avg(1.25, dev)
    assert a.dtype == torch.float32 and a.shape == (1,) and float(a) == 1.25 and AG._dense_avg(1.5, dev).item() == 1.5
    wide = torch.tensor(3.0, dtype=torch.float64)
    lin = AG._dense_avg(wide, dev)
    assert lin.dtype == torch.float32 and float(lin) == 3.0
    wide.mul_(2.0)
    assert float(AG._dense_avg(wide, dev)) == 6.0
    assert not [k for k in wide.__dict__ if str(k).startswith("_pna_amd")]
    src = open(os.path.join(ROOT, "pna_amd", "autograd.py")).read()
    body = src[src.index("def _dense_avg("):src.index("def dense_layer(")]
    assert "memo(" not in body and "__dict__" not in body
