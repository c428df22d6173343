"""Host side of the one-call MLP head route (no GPU): the float64 references of tests/mlp_head_cases.py against float64 autograd through
nn.Linear, F.relu and F.leaky_relu; the random cases' bars, caps and at-risk units; the exact cases' bound; the knob and the route
predicates clause by clause for nets.MLPReadout, layers.MLP and the superpixel net's embeddings; the exported symbols with the struct's
layout and the scope checks; the workspace formula; state_dict compatibility; and the compiler's resource report of pna_mlp_head.hip."""
import ctypes
import importlib
import os
import re
import shutil
import subprocess

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import mlp_head_cases as C
from pna_amd import _lib, layers, nets
from pna_amd import autograd as AG
from pna_amd import functional as PF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pna_amd", "csrc")


# ---- the references, the bars and the cases ------------------------------------------------------------------------------------------
def _autograd64(c):
    x = c["x"].double().requires_grad_(True)
    ws = [w.double().requires_grad_(True) for w in c["ws"]]
    bs = [None if b is None else b.double().requires_grad_(True) for b in c["bs"]]
    h = x
    for w, b, act in zip(ws, bs, c["acts"]):
        h = F.linear(h, w, b)
        kind, slope = C.act_parts(act)
        h = F.relu(h) if kind == "relu" else F.leaky_relu(h, slope) if kind == "leaky" else h
    leaves = [x] + ws + [b for b in bs if b is not None]
    grads = torch.autograd.grad(h, leaves, c["go"].double())
    L = len(ws)
    names = ["x"] + [f"w{l}" for l in range(L)] + [f"b{l}" for l in range(L) if bs[l] is not None]
    return h.detach(), dict(zip(names, grads))


@pytest.mark.parametrize("name", C.NAMES + C.EXACT_NAMES)
def test_float64_formulas_are_float64_autograd_through_nn_linear(name):
    c = C.mlp_case(name) if name in C.CASES else C.exact_case(name)
    y, grads = _autograd64(c)
    torch.testing.assert_close(c["ref"]["y"], y, rtol=1e-12, atol=1e-12)
    assert sorted(grads) == sorted(k for k in C.tensors_of(c) if k != "y")
    for k, g in grads.items():
        torch.testing.assert_close(c["ref"][k], g, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("name", C.NAMES)
def test_no_unit_is_at_risk_and_no_bar_exceeds_the_cap(name):
    c = C.mlp_case(name)
    assert C.at_risk(c) == 0
    for k in C.tensors_of(c):
        top = float(c["ref"][k].abs().max())
        assert 0 < c["bars"][k] <= C.CAP * top, (k, c["bars"][k], top)
    assert 0 <= C.CASES[name][5] < C.MAX_SEEDS


def test_the_bars_are_tight_enough_to_see_a_wrong_derivative_or_a_dropped_bias():
    c = C.mlp_case("mt")
    swapped = C.mlp_grad_ref(c["x"], c["ws"], c["bs"], [("leaky", 0.02)] * 3, c["go"])                # another slope
    assert C.worst_ratio(swapped["y"], c["ref"]["y"], c["bars"]["y"]) > 10 and C.worst_ratio(swapped["x"], c["ref"]["x"], c["bars"]["x"]) > 10
    c = C.mlp_case("zinc")
    nobias = C.mlp_grad_ref(c["x"], c["ws"], [None] * 3, c["acts"], c["go"])
    assert C.worst_ratio(nobias["y"], c["ref"]["y"], c["bars"]["y"]) > 1e3
    half = C.mlp_grad_ref(c["x"], [w.half().float() for w in c["ws"]], c["bs"], c["acts"], c["go"])
    assert C.worst_ratio(half["w0"], c["ref"]["w0"], c["bars"]["w0"]) > 10


def test_case_list_covers_what_it_promises():
    assert C.SLAB == _lib.PNA_MLP_SLAB_ROWS and C.MAX_SLABS == _lib.PNA_MLP_MAX_SLABS
    assert C.ACT_CODES == {"none": _lib.PNA_MLP_ACT_NONE, "relu": _lib.PNA_MLP_ACT_RELU, "leaky": _lib.PNA_MLP_ACT_LEAKY}
    rows = {n: C.CASES[n][0] for n in C.NAMES}
    widths = {n: C.CASES[n][1] for n in C.NAMES}
    assert 1 in rows.values() and any(v % 16 not in (0,) and v > 16 for v in rows.values())            # one row; a ragged last tile
    every = {w for ws in widths.values() for w in ws}
    assert {1, 127, 128} <= every
    assert {len(ws) - 1 for ws in widths.values()} >= {1, 3, 4}
    V = rows["slabs"]
    assert C.slab_rows(V) == 66 and -(-V // C.slab_rows(V)) == 64                                        # several slabs, above the 64-row floor
    assert any(not all(C.CASES[n][3]) for n in C.NAMES)                                                  # a NULL bias
    assert all(a == ("leaky", 0.01) for a in C.CASES["mt"][2]) and len(C.CASES["mt"][2]) == 3           # LeakyReLU on every layer, the last too
    assert any(C.CASES[n][4] is not None for n in C.NAMES)                                               # a strided x
    assert (128, (70, 35, 17, 1)) == C.CASES["zinc"][:2] and (128, (70, 35, 17, 10)) == C.CASES["cls10"][:2]
    for n in C.NAMES:
        c = C.mlp_case(n)
        for l, w in enumerate(c["ws"]):
            k = widths[n][l] ** -0.5
            assert float(w.abs().max()) <= k and (c["bs"][l] is None or float(c["bs"][l].abs().max()) <= k)


@pytest.mark.parametrize("name", C.EXACT_NAMES)
def test_exact_cases_are_exact_in_fp32_in_any_order(name):
    c = C.exact_case(name)
    V, widths = C.EXACT[name][:2]
    assert V <= 40 and max(widths) <= 16
    assert all(C.act_parts(a)[1] in (0.0, 0.25) for a in c["acts"])
    M, q = C.exact_bound(c)
    assert M < 2.0 ** 24 * q and q == 2.0 ** round(__import__("math").log2(q))
    for k in C.tensors_of(c):                                                     # every reference value is a multiple of q, below 2^24 q
        r = c["ref"][k] / q
        assert torch.equal(r, r.round()) and float(c["ref"][k].abs().max()) <= M
        assert torch.equal(c["ref"][k].float().double(), c["ref"][k])
    assert C.zero_preactivations(c) >= 5                                           # the kink itself is hit
    o32 = C.mlp_grad_ref(c["x"], c["ws"], c["bs"], c["acts"], c["go"], dtype=torch.float32)
    for k in C.tensors_of(c):                                                     # (the CPU's fp32 arithmetic agrees: exact)
        assert torch.equal(o32[k].double(), c["ref"][k]), k


# ---- the knob and the predicates ---------------------------------------------------------------------------------------------------
def test_route_is_off_by_default_and_read_from_the_environment(monkeypatch):
    monkeypatch.delenv("PNA_AMD_MLP_HEAD_ROWS", raising=False)
    try:
        assert importlib.reload(PF).MLP_HEAD_ROWS == 0
        monkeypatch.setenv("PNA_AMD_MLP_HEAD_ROWS", "4096")
        assert importlib.reload(PF).MLP_HEAD_ROWS == 4096
    finally:
        monkeypatch.delenv("PNA_AMD_MLP_HEAD_ROWS", raising=False)
        importlib.reload(PF)


class _OnGpu:
    """A stand-in for rows on the GPU (the predicate reads shape, dtype, is_cuda, dim, stride, is_contiguous, device and nothing else)."""

    def __init__(self, *shape, dtype=torch.float32, col_stride=1, contiguous=True):
        self.shape, self.dtype, self.is_cuda, self.device, self._cs, self._c = torch.Size(shape), dtype, True, torch.device("cpu"), col_stride, contiguous

    def dim(self):
        return len(self.shape)

    def stride(self, d):
        return self._cs if d == len(self.shape) - 1 else self.shape[-1] * self._cs

    def is_contiguous(self):
        return self._cs == 1 and self._c


def test_mlp_readout_path_clause_by_clause(monkeypatch):
    R = lambda i=70, o=1, L=2: nets.MLPReadout(i, o, L)                             # noqa: E731
    x = _OnGpu(128, 70)
    monkeypatch.setattr(PF, "MLP_HEAD_ROWS", 0)
    assert not R()._one_call_path(None)                                           # the knob at 0: nothing is looked at
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))     # the parameters' residency without a GPU
    assert not R()._one_call_path(x)
    monkeypatch.setattr(PF, "MLP_HEAD_ROWS", 4096)
    assert R()._one_call_path(x) and R().eval()._one_call_path(x) and R(70, 10)._one_call_path(x)
    assert R(128, 3, 3)._one_call_path(_OnGpu(5, 128)) and R(4, 1, 0)._one_call_path(_OnGpu(1, 4))      # four layers; one layer, one row
    # rows
    monkeypatch.setattr(PF, "MLP_HEAD_ROWS", 127)
    assert not R()._one_call_path(x)                                              # more rows than the knob covers
    monkeypatch.setattr(PF, "MLP_HEAD_ROWS", 128)
    assert R()._one_call_path(x)
    monkeypatch.setattr(PF, "MLP_HEAD_ROWS", 4096)
    assert not R()._one_call_path(_OnGpu(0, 70))
    # the tensor
    assert not R()._one_call_path(_OnGpu(2, 64, 70))                              # 3-D is layers.MLP's shape
    assert not R()._one_call_path(_OnGpu(128, 70, dtype=torch.float64)) and not R()._one_call_path(_OnGpu(128, 70, dtype=torch.bfloat16))
    assert not R()._one_call_path(_OnGpu(128, 70, col_stride=2))
    flat = _OnGpu(128, 70)
    flat.stride = lambda d: (0, 1)[d]
    assert not R()._one_call_path(flat)                                           # expanded rows: a row pitch below the width
    cpu = _OnGpu(128, 70)
    cpu.is_cuda = False
    assert not R()._one_call_path(cpu)
    other = _OnGpu(128, 70)
    other.device = torch.device("meta")
    assert not R()._one_call_path(other)                                          # not the parameters' device
    assert not R()._one_call_path(_OnGpu(128, 69))                                # not the first layer's width
    # the module
    assert not R().double()._one_call_path(x) and not R().to(torch.bfloat16)._one_call_path(x)
    one = R()
    one.FC_layers[1].bias.data = one.FC_layers[1].bias.data.double()
    assert not one._one_call_path(x)                                              # one fp64 parameter
    sub = R()

    class Lin(nn.Linear):
        pass
    sub.FC_layers[0] = Lin(70, 35)
    assert not sub._one_call_path(x)                                              # not a plain nn.Linear
    nob = R()
    nob.FC_layers[2] = nn.Linear(17, 1, bias=False)
    assert nob._one_call_path(x)                                                  # bias=False is inside the scope
    # the widths and the layer count
    assert not R(258, 1)._one_call_path(_OnGpu(128, 258))                         # width 129 inside
    assert not R(129, 1, 0)._one_call_path(_OnGpu(128, 129))
    assert not R(128, 1, 4)._one_call_path(_OnGpu(128, 128))                      # five layers
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: False))
    assert not R()._one_call_path(x)                                              # parameters on the host


def test_layers_mlp_path_clause_by_clause(monkeypatch):
    def M(i=16, h=16, o=3, n=3, **kw):
        kw.setdefault("mid_activation", "LeakyReLU")
        kw.setdefault("last_activation", "LeakyReLU")
        return layers.MLP(i, h, o, n, **kw)
    x = _OnGpu(16, 15, 16)
    monkeypatch.setattr(PF, "MLP_HEAD_ROWS", 0)
    assert not M()._one_call_path(None)
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    assert not M()._one_call_path(x)
    monkeypatch.setattr(PF, "MLP_HEAD_ROWS", 240)
    assert M()._one_call_path(x) and M().eval()._one_call_path(x) and M()._one_call_path(_OnGpu(240, 16))
    assert M(mid_activation="relu", last_activation="none")._one_call_path(x) and M(n=1)._one_call_path(x) and M(n=4)._one_call_path(x)
    monkeypatch.setattr(PF, "MLP_HEAD_ROWS", 239)
    assert not M()._one_call_path(x)                                              # B N = 240 rows
    monkeypatch.setattr(PF, "MLP_HEAD_ROWS", 4096)
    assert not M()._one_call_path(_OnGpu(16, 15, 16, contiguous=False))           # a reshape that would copy
    assert not M()._one_call_path(_OnGpu(2, 8, 15, 16))                           # 4-D (a pretrans over edges)
    assert not M()._one_call_path(_OnGpu(16, 15, 16, dtype=torch.float64)) and not M().double()._one_call_path(x)
    # activations, batch-norm, dropout
    assert not M(mid_activation="tanh")._one_call_path(x) and not M(last_activation="sigmoid")._one_call_path(x)

    class Leaky(nn.LeakyReLU):
        pass
    sub = M()
    sub.fully_connected[0].activation = Leaky()
    assert not sub._one_call_path(x)                                              # exact types only
    fn = M()
    fn.fully_connected[1] = layers.FCLayer(16, 16, activation=F.relu)
    assert not fn._one_call_path(x)                                               # a callable is not one of the three modules
    assert not M(mid_b_norm=True)._one_call_path(x) and not M(last_b_norm=True)._one_call_path(x)
    assert not layers.S2SReadout(16, 16, 3).mlp._one_call_path(_OnGpu(16, 32))     # the graph head keeps torch's ops
    drop = M(dropout=0.2)
    assert not drop.train()._one_call_path(x) and drop.eval()._one_call_path(x)   # a dropout counts where it is active
    # widths and layers
    assert not M(129, 16, 3)._one_call_path(_OnGpu(16, 15, 129)) and not M(16, 129, 3)._one_call_path(x) and not M(16, 16, 129)._one_call_path(x)
    assert M(128, 128, 128)._one_call_path(_OnGpu(16, 15, 128)) and not M(n=5)._one_call_path(x)
    # is_affine and tail are what they were
    assert M(n=1, last_activation="none").is_affine and not M().is_affine
    t = torch.randn(4, 16)
    m = M(n=2, mid_activation="relu", last_activation="none")
    assert torch.equal(m.tail(m.fully_connected[0].linear(t)), m.fully_connected[1](F.relu(m.fully_connected[0].linear(t))))


def test_superpixel_embeddings_go_through_the_same_predicate(monkeypatch):
    calls = []
    monkeypatch.setattr(AG, "mlp_head", lambda x, linears, acts: calls.append((x.shape, len(linears), acts)) or "routed")
    lin = nn.Linear(5, 60)
    x = torch.randn(7, 5)
    monkeypatch.setattr(PF, "MLP_HEAD_ROWS", 0)
    assert torch.equal(nets.linear_rows(lin, x), lin(x)) and not calls
    monkeypatch.setattr(PF, "MLP_HEAD_ROWS", 4096)
    assert torch.equal(nets.linear_rows(lin, x), lin(x)) and not calls            # rows on the host: torch's own
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    monkeypatch.setattr(PF, "MLP_HEAD_ROWS", 15168)
    assert nets.linear_rows(lin, _OnGpu(15168, 5)) == "routed"
    assert calls == [((15168, 5), 1, [(_lib.PNA_MLP_ACT_NONE, 0.0)])]
    monkeypatch.setattr(PF, "MLP_HEAD_ROWS", 15167)
    assert not PF.mlp_head_path(_OnGpu(15168, 5), [lin], [None])
    monkeypatch.setattr(PF, "MLP_HEAD_ROWS", 1 << 20)
    assert not PF.mlp_head_path(_OnGpu(100, 5, dtype=torch.float64), [lin], [None])
    assert not PF.mlp_head_path(_OnGpu(100, 5), [nn.Linear(5, 129)], [None])
    assert PF.mlp_head_path(_OnGpu(100, 1), [nn.Linear(1, 50)], [None])           # the edge embedding: in_dim_edge 1


def test_mlp_head_fits_and_act_codes_at_their_edges():
    assert PF.mlp_head_fits([1, 1], [0]) and PF.mlp_head_fits([128] * 5, [1, 2, 0, 1])
    assert not PF.mlp_head_fits([128] * 6, [0] * 5) and not PF.mlp_head_fits([4], [])
    assert not PF.mlp_head_fits([0, 4], [0]) and not PF.mlp_head_fits([4, 129], [0]) and not PF.mlp_head_fits([129, 4], [0])
    assert not PF.mlp_head_fits([4, 4], [3]) and not PF.mlp_head_fits([4, 4], [-1]) and not PF.mlp_head_fits([4, 4, 4], [0])
    assert PF.mlp_head_act(None) == (0, 0.0) and PF.mlp_head_act(nn.ReLU()) == (1, 0.0) and PF.mlp_head_act(nn.LeakyReLU(0.25)) == (2, 0.25)
    assert PF.mlp_head_act(nn.Tanh()) is None and PF.mlp_head_act(F.relu) is None


def test_knob_off_runs_the_old_lines_on_the_host():
    assert PF.MLP_HEAD_ROWS == 0
    torch.manual_seed(0)
    r = nets.MLPReadout(70, 10)
    x = torch.randn(9, 70)
    assert torch.equal(r(x), r.FC_layers[2](F.relu(r.FC_layers[1](F.relu(r.FC_layers[0](x))))))
    m = layers.MLP(16, 16, 3, 3, mid_activation="LeakyReLU", last_activation="LeakyReLU")
    xb = torch.randn(2, 5, 16)
    want = xb
    for fc in m.fully_connected:
        want = F.leaky_relu(fc.linear(want), 0.01)
    assert torch.equal(m(xb), want) and m(xb).shape == (2, 5, 3)


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_short_structs_are_refused():
    L = _lib.lib()
    for name in ("pna_mlp_head_fwd_f32", "pna_mlp_head_bwd_f32", "pna_mlp_head_workspace_bytes", "pna_mlp_head_in_scope"):
        assert hasattr(L, name), name
    assert L.pna_abi_version() == _lib.PNA_ABI_VERSION == 23
    assert "23, additive: + pna_mlp_head_fwd_f32 / pna_mlp_head_bwd_f32" in open(os.path.join(ROOT, "include", "pna_amd.h")).read()
    cls = _lib.PnaMlpHeadArgs
    for fn in (L.pna_mlp_head_fwd_f32, L.pna_mlp_head_bwd_f32):
        a = cls()
        assert a.struct_size == ctypes.sizeof(cls)
        for short in (0, ctypes.sizeof(cls) - 8):
            a.struct_size = short
            assert fn(ctypes.byref(a), None) == -1 and b"struct_size" in L.pna_last_error()
        a.struct_size = ctypes.sizeof(cls)
        assert fn(ctypes.byref(a), None) == -1 and b"struct_size" not in L.pna_last_error()              # all-zero: outside the scope
        assert fn(None, None) == -1
    assert re.search(r"class PnaMlpHeadArgs\(_PnaArgs\)", open(os.path.join(ROOT, "INTEGRATION.md")).read())


def test_the_struct_and_its_constants_have_gccs_layout(tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not available")
    cls = _lib.PnaMlpHeadArgs
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "pna_amd.h"', "int main(void) {",
             '  printf("PnaMlpHeadArgs . %zu 0\\n", sizeof(pna_mlp_head_args));']
    for f, *_ in cls._fields_:
        lines.append(f'  printf("PnaMlpHeadArgs {f} %zu %zu\\n", sizeof(((pna_mlp_head_args*)0)->{f}), offsetof(pna_mlp_head_args, {f}));')
    lines += ['  printf("consts %d %d %d %d %d %d %d %d\\n", PNA_MAX_MLP_LAYERS, PNA_MAX_MLP_WIDTHS, PNA_MLP_MAX_WIDTH, PNA_MLP_ACT_NONE, '
              'PNA_MLP_ACT_RELU, PNA_MLP_ACT_LEAKY, PNA_MLP_SLAB_ROWS, PNA_MLP_MAX_SLABS);', "  return 0;", "}"]
    src, exe = tmp_path / "l.c", tmp_path / "l"
    src.write_text("\n".join(lines))
    subprocess.run([gcc, "-std=c11", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True)
    for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
        parts = line.split()
        if parts[0] == "consts":
            assert [int(v) for v in parts[1:]] == [_lib.PNA_MAX_MLP_LAYERS, _lib.PNA_MAX_MLP_WIDTHS, _lib.PNA_MLP_MAX_WIDTH, _lib.PNA_MLP_ACT_NONE,
                                                   _lib.PNA_MLP_ACT_RELU, _lib.PNA_MLP_ACT_LEAKY, _lib.PNA_MLP_SLAB_ROWS, _lib.PNA_MLP_MAX_SLABS]
            continue
        _, f, size, off = parts
        if f == ".":
            assert ctypes.sizeof(cls) == int(size)
        else:
            fld = getattr(cls, f)
            assert (fld.size, fld.offset) == (int(size), int(off)), (f, fld.size, fld.offset, size, off)


def _scope_args(kw):
    """An args struct inside the scope except for `kw`; the pointers are non-null but never followed: every check precedes a launch."""
    a = _lib.PnaMlpHeadArgs()
    a.V, a.n_layers = 8, 2
    a.widths[0], a.widths[1], a.widths[2] = 16, 8, 3
    a.act[0], a.act[1] = _lib.PNA_MLP_ACT_RELU, _lib.PNA_MLP_ACT_NONE
    a.x, a.ldx, a.y, a.ldy = 4096, 16, 4096, 3
    for l, ld in enumerate((16, 8)):
        a.w[l], a.ldw[l], a.b[l] = 4096, ld, 4096
    for k, v in kw.items():
        if isinstance(k, tuple):
            getattr(a, k[0])[k[1]] = v
        else:
            setattr(a, k, v)
    return a


@pytest.mark.parametrize("kw,clause", [
    ({"n_layers": 0}, b"n_layers"), ({"n_layers": 5}, b"n_layers"), ({("widths", 0): 0}, b"every width"), ({("widths", 1): 129}, b"every width"),
    ({("widths", 2): -1}, b"every width"), ({"V": 0}, b"V >= 1"), ({"V": 2 ** 31}, b"V >= 1"), ({("act", 0): 3}, b"every act"),
    ({("act", 1): -1}, b"every act"), ({"x": None}, b"needs x"), ({"ldx": 15}, b"needs x"), ({("w", 1): None}, b"every w"),
    ({("ldw", 0): 15}, b"every w"), ({"y": None}, b"needs y"), ({"ldy": 2}, b"needs y")])
def test_forward_scope_clauses_are_named(kw, clause):
    L = _lib.lib()
    assert L.pna_mlp_head_fwd_f32(ctypes.byref(_scope_args(kw)), None) == -1
    assert clause in L.pna_last_error(), L.pna_last_error()


@pytest.mark.parametrize("kw,clause", [
    ({}, b"grad_out"), ({"grad_out": 4096, "ld_go": 2}, b"grad_out"), ({"grad_out": 4096, "ld_go": 3, "need_x": 1}, b"grad_x"),
    ({"grad_out": 4096, "ld_go": 3, "need_x": 1, "grad_x": 4096, "ld_gx": 15}, b"grad_x"),
    ({"grad_out": 4096, "ld_go": 3, ("need_w", 1): 1}, b"gradient buffer"), ({"grad_out": 4096, "ld_go": 3, ("need_b", 0): 1}, b"gradient buffer"),
    ({"grad_out": 4096, "ld_go": 3, ("need_w", 0): 1, ("grad_w", 0): 4096}, b"workspace"),
    ({"grad_out": 4096, "ld_go": 3, ("need_w", 0): 1, ("grad_w", 0): 4096, "workspace": 4096, "workspace_bytes": 64}, b"workspace"),
    ({"grad_out": 4096, "ld_go": 3, ("need_w", 0): 1, ("grad_w", 0): 4096, "workspace": 4100, "workspace_bytes": 1 << 20}, b"aligned"),
    ({"grad_out": 4096, "ld_go": 3, "n_layers": 5}, b"n_layers")])
def test_backward_scope_clauses_are_named(kw, clause):
    L = _lib.lib()
    assert L.pna_mlp_head_bwd_f32(ctypes.byref(_scope_args(kw)), None) == -1
    assert clause in L.pna_last_error(), L.pna_last_error()


def test_a_backward_that_wants_nothing_returns_without_a_launch():
    assert _lib.lib().pna_mlp_head_bwd_f32(ctypes.byref(_scope_args({"grad_out": 4096, "ld_go": 3})), None) == 0


def test_workspace_bytes_formula_and_scope():
    L = _lib.lib()
    ints = lambda v: (ctypes.c_int32 * len(v))(*v)                                  # noqa: E731
    for widths in ((70, 35, 17, 1), (70, 35, 17, 10), (16, 16, 16, 3), (1, 1), (128,) * 5, (5, 60), (127, 65, 33, 2)):
        n = len(widths) - 1
        for V in (1, 15, C.SLAB - 1, C.SLAB, C.SLAB + 1, 3 * C.SLAB + 17, 4200, C.SLAB * C.MAX_SLABS, C.SLAB * C.MAX_SLABS + 1, 52000, 10 ** 6):
            slab = max(C.SLAB, -(-V // C.MAX_SLABS))
            n_slab = -(-V // slab)
            assert n_slab <= C.MAX_SLABS and C.slab_rows(V) == slab == max(_lib.PNA_MLP_SLAB_ROWS, -(-V // _lib.PNA_MLP_MAX_SLABS))
            rows = 2 * sum(widths[1:]) - widths[-1]
            image = sum(widths[l] * (widths[l - 1] + 1) for l in range(1, n + 1))
            want = 4 * (V * rows + n_slab * image)
            assert L.pna_mlp_head_workspace_bytes(V, n, ints(widths)) == want == PF.mlp_head_workspace_bytes(V, widths), (V, widths)
    for V, widths in ((0, (4, 4)), (2 ** 31, (4, 4)), (8, (4,)), (8, (4,) * 6), (8, (0, 4)), (8, (4, 129)), (8, (129, 4))):
        assert PF.mlp_head_workspace_bytes(V, widths) == -1, (V, widths)
    assert L.pna_mlp_head_workspace_bytes(8, 1, None) == -1 and L.pna_mlp_head_in_scope(8, 1, None, None) == 0
    assert L.pna_mlp_head_in_scope(8, 1, ints((4, 4)), None) == 0 and L.pna_mlp_head_in_scope(8, 1, ints((4, 4)), ints((0,))) == 1


# ---- state_dict compatibility ----------------------------------------------------------------------------------------------------------
def test_state_dicts_are_what_they_were():
    r = nets.MLPReadout(70, 1)
    assert list(r.state_dict()) == [f"FC_layers.{l}.{p}" for l in range(3) for p in ("weight", "bias")]
    stock = nn.ModuleDict({"FC_layers": nn.ModuleList([nn.Linear(70, 35), nn.Linear(35, 17), nn.Linear(17, 1)])})
    r.load_state_dict(stock.state_dict(), strict=True)
    stock.load_state_dict(nets.MLPReadout(70, 1).state_dict(), strict=True)
    m = layers.MLP(16, 16, 3, 3, mid_activation="LeakyReLU", last_activation="LeakyReLU")
    assert list(m.state_dict()) == [f"fully_connected.{l}.linear.{p}" for l in range(3) for p in ("weight", "bias")]
    import tower_drop_train_cases as T
    net = nets.PNANetSuperpixels(T.net_params(0.0, True, torch.tensor(2.0)))
    keys = list(net.state_dict())
    assert keys[:4] == ["embedding_h.weight", "embedding_h.bias", "embedding_e.weight", "embedding_e.bias"]
    assert type(net.embedding_h) is nn.Linear and type(net.embedding_e) is nn.Linear
    assert [k for k in keys if k.startswith("MLP_layer")] == [f"MLP_layer.FC_layers.{l}.{p}" for l in range(3) for p in ("weight", "bias")]


# ---- the compiler's report ---------------------------------------------------------------------------------------------------------------
MAX_VGPR_ROWS = 96          # the two rows kernels stay at or under 96 VGPRs (5 wavefronts per SIMD: two 8-wavefront workgroups per CU)


def test_no_kernel_of_the_file_uses_scratch(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
           "-S", "--cuda-device-only", "-o", str(tmp_path / "out.s"), os.path.join(CSRC, "pna_mlp_head.hip"), "-Rpass-analysis=kernel-resource-usage"]
    out = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    names = re.findall(r"Function Name: (\S+)", out)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", out)]
    vgprs = [int(v) for v in re.findall(r" VGPRs: (\d+)", out)]
    assert len(names) == len(scratch) == len(vgprs) == 4, names
    for k in ("k_mlp_rows_fwd", "k_mlp_rows_bwd", "k_mlp_dw_slab", "k_mlp_dw_final"):
        assert any(k in n for n in names), k
    assert not [(n, s) for n, s in zip(names, scratch) if s != 0]
    assert not [(n, v) for n, v in zip(names, vgprs) if "k_mlp_rows" in n and v > MAX_VGPR_ROWS]
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert f"at or under {MAX_VGPR_ROWS} VGPRs" in design and "pna_mlp_head" in design
    text = open(str(tmp_path / "out.s")).read()
    assert "v_mfma_f32_16x16x4_f32" in text                                          # the exact-fp32 matrix instruction
