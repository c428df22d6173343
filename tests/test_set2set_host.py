"""Host side of the one-call Set2Set readout and of the GNN front end (no GPU): the cap that keeps the GPU tests' bars honest, the
restatement the references use against the loop over nn.LSTM, the reference's checkpoints loaded key for key into layers.Set2Set,
layers.S2SReadout and pytorch.gnn_framework.GNN with the GNN's golden outputs reproduced on the CPU, the knob and the route predicate, the
exported symbols with the struct's layout and every scope clause, the LDS and workspace formulas against their Python mirrors, and the
compiler's resource report of pna_set2set.hip."""
import ctypes
import importlib
import os
import re
import shutil
import subprocess
import types

import pytest
import torch
import torch.nn as nn

import set2set_cases as C
from conftest import golden_names, load_golden
from pna_amd import _lib, layers
from pna_amd import autograd as AG
from pna_amd import functional as PF
from pna_amd.pytorch.gnn_framework import GNN
from pna_amd.pytorch.pna.layer import PNALayer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pna_amd", "csrc")
TRACES = golden_names("c1_train_trace")


# ---- the references and the bars ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.NAMES)
def test_the_fp32_oracle_alone_keeps_every_bar_under_the_cap(name):
    ref64, ref32, bars = C.references(name)
    cap = C.cap_of(ref64)
    assert all(torch.isfinite(v).all() for v in ref64.values()) and all(torch.isfinite(v).all() for v in ref32.values())
    worst = max(((bars[k] / cap[k]) if cap[k] > 0 else 0.0, k) for k in bars)
    print("S2S_BAR_OVER_CAP", name, round(worst[0], 3), worst[1])
    assert set(ref64) == set(C.TENSORS)
    for k in bars:
        assert bars[k] <= cap[k], (k, bars[k], cap[k])
    assert torch.equal(ref64["b_ih"], ref64["b_hh"])                # independently drawn, equal gradients


def test_case_list_covers_what_it_promises():
    cases = [C.s2s_case(n) for n in C.NAMES]
    table = {(1, 1, 2, 1, 1.0), (2, 3, 2, 2, 1.0), (15, 16, 16, 15, 1.0), (17, 3, 32, 17, 1.0), (64, 2, 31, 64, 1.0), (128, 2, 32, 128, 1.0),
             (128, 1, 2, 128, 1.0), (97, 4, 16, 97, 1.0), (15, 3, 16, 3, 1.0), (5, 300, 16, 5, 1.0), (128, 2, 32, 128, 3.0)}
    have = {(c["N"], c["B"], c["D"], c["steps"], C.CASES[c["name"]][4]) for c in cases}
    assert table <= have
    assert C.SLABS == _lib.PNA_S2S_MAX_SLABS and any(c["B"] > C.SLABS for c in cases)
    assert any(c["D"] == 1 for c in cases) and C.CASES["sat"][5] == 4.0
    for c in cases:
        assert PF.set2set_fits(c["N"], c["D"], c["steps"]), c["name"]
        assert not torch.equal(c["b_ih"], c["b_hh"])
        k = c["D"] ** -0.5 * C.CASES[c["name"]][4]
        assert all(float(c[p].abs().max()) <= k for p in C.PARAMS)


def _loop_module(c, dtype=torch.float32):
    """layers.Set2Set carrying the case's parameters: on the CPU its forward is the loop over nn.LSTM."""
    m = layers.Set2Set(c["D"], steps=c["steps"])
    m.lstm.load_state_dict(C.lstm_state_dict(c), strict=True)
    return m.to(dtype)


@pytest.mark.parametrize("name", ["n1", "n2", "n15", "n17", "steps3", "d1", "sat"])
def test_restatement_equals_the_loop_over_nn_lstm(name):
    """set2set_ref in fp32 against the reference's formulation (a one-step nn.LSTM per round): 1e-6 of the largest output; in float64 the
    two and their gradients agree to 1e-12."""
    c = C.s2s_case(name)
    with torch.no_grad():
        want = _loop_module(c)(c["x"])
        got = C.set2set_ref(c["x"], *[c[k] for k in C.PARAMS], c["steps"])
    err = float((got - want).abs().max()) / float(want.abs().max())
    print("S2S_REF_VS_LSTM", name, f"{err:.2e}")
    assert got.shape == want.shape == (c["B"], 2 * c["D"]) and err <= 1e-6
    m = _loop_module(c, torch.float64)
    x = c["x"].double().requires_grad_(True)
    grads = torch.autograd.grad(m(x), [x, m.lstm.weight_ih_l0, m.lstm.weight_hh_l0, m.lstm.bias_ih_l0, m.lstm.bias_hh_l0], c["go"].double())
    ref64 = C.references(name)[0]
    for k, g in zip(("x",) + C.PARAMS, grads):
        torch.testing.assert_close(g, ref64[k], rtol=1e-10, atol=1e-12)


# ---- the modules and the reference's checkpoints ---------------------------------------------------------------------------------------
class OracleLayer(PNALayer):
    """PNALayer's parameters under oracle.torch_oracle's plain-torch forward: the convolution of the CPU runs below (the package's own
    PNALayer has no CPU path), so what they check is the assembly around it."""

    def forward(self, x, adj):
        from oracle import torch_oracle as TO
        t0 = self.towers[0]
        return TO.dense_layer_forward(dict(self.named_parameters()), x, adj, t0.aggregators, t0.scalers, t0.avg_d, len(self.towers),
                                      self.divide_input, t0.self_loop)


def _gnn(meta, avg_d, device="cpu", layer_type=OracleLayer):
    """The README model: hidden 16, 4 towers, fixed, variable N / 2 layers, shared GRU (multitask_benchmark's configuration)."""
    conv = dict(aggregators=meta["aggregators"], scalers=meta["scalers"], avg_d=avg_d, towers=meta["towers"], self_loop=False,
                pretrans_layers=1, posttrans_layers=1)
    first = dict(layer_type=layer_type, args=dict(conv, divide_input=False))
    middle = types.SimpleNamespace(layer_type=layer_type, args=dict(conv, divide_input=True))
    return GNN(nfeat=2, nhid=meta["hidden"], nodes_out=3, graph_out=3, dropout=meta.get("dropout", 0.0), conv_layers=lambda adj: adj.shape[1] // 2,
               fc_layers=3, first_conv_descr=first, middle_conv_descr=middle, final_activation="LeakyReLU", skip=False, gru=True, fixed=True,
               variable=True, device=device)


@pytest.mark.parametrize("name", ["c1_gnn_forward_n15"] + TRACES)
def test_gnn_readout_and_set2set_load_the_reference_checkpoints_strictly(name):
    meta, a, sd = load_golden(name)
    net = _gnn(meta, {"log": a["avg_log"], "lin": a["avg_lin"]})
    assert sum(p.numel() for p in net.parameters()) == meta["n_parameters"] == 8350
    net.load_state_dict(sd, strict=True)
    assert [n for n, _ in net.named_children()] == ["conv_layers", "gru", "nodes_read_out", "graph_read_out"]
    assert list(net.state_dict()) == list(sd)                       # ... and in the checkpoint's order
    assert len(net.conv_layers) == 2 and isinstance(net.gru, layers.GRU) and isinstance(net.graph_read_out, layers.S2SReadout)
    H = meta["hidden"]
    head = layers.S2SReadout(H, H, 3, fc_layers=3, final_activation="LeakyReLU")
    head.load_state_dict({k[len("graph_read_out."):]: v for k, v in sd.items() if k.startswith("graph_read_out.")}, strict=True)
    s2s = layers.Set2Set(H)
    s2s.load_state_dict({k[len("graph_read_out.set2set."):]: v for k, v in sd.items() if k.startswith("graph_read_out.set2set.")}, strict=True)
    assert isinstance(s2s.lstm, nn.LSTM) and s2s.lstm.batch_first and (s2s.lstm.input_size, s2s.lstm.hidden_size) == (2 * H, H)
    assert s2s.nhid == 2 * H and s2s.lstm_output_dim == H and head.mlp.fully_connected[0].b_norm is not None


def test_gnn_reproduces_the_reference_forward_on_the_cpu():
    meta, a, sd = load_golden("c1_gnn_forward_n15")
    net = _gnn(meta, {"log": a["avg_log"], "lin": a["avg_lin"]})
    net.load_state_dict(sd, strict=True)
    net.eval()
    with torch.no_grad():
        nodes, graph = net(a["x"], a["adj"])
    for got, want, what in ((nodes, a["out"], "out"), (graph, a["graph_out"], "graph_out")):
        err = float((got - want).abs().max()) / float(want.abs().max())
        print("S2S_GNN_CPU", what, f"{err:.2e}")
        assert got.shape == want.shape and err <= 1e-5, what


def test_constructors_keep_the_reference_contract():
    with pytest.raises(ValueError, match="hidden_dim should be larger than input_dim"):
        layers.Set2Set(8, nhid=8)
    m = layers.Set2Set(4, nhid=10, steps=3, num_layers=2)
    assert (m.lstm.input_size, m.lstm.hidden_size, m.lstm.num_layers, m.lstm_output_dim) == (10, 4, 2, 6)
    conv = dict(layer_type=PNALayer, args=dict(aggregators=["mean"], scalers=["identity"], avg_d={"log": 1.0, "lin": 1.0}))
    kw = dict(nfeat=2, nhid=4, nodes_out=1, graph_out=1, dropout=0.0)
    with pytest.raises(AssertionError, match="function from adjacency matrix"):
        GNN(conv_layers=2, first_conv_descr=dict(conv), middle_conv_descr=dict(conv), variable=True, fixed=True, **kw)
    with pytest.raises(AssertionError, match="they must be fixed"):
        GNN(conv_layers=lambda adj: 2, first_conv_descr=dict(conv), middle_conv_descr=dict(conv), variable=True, **kw)
    with pytest.raises(AssertionError, match="skip and fixed"):
        GNN(conv_layers=lambda adj: 2, first_conv_descr=dict(conv), middle_conv_descr=dict(conv), variable=True, fixed=True, skip=True, **kw)
    with pytest.raises(AssertionError, match="greater than 0"):
        GNN(conv_layers=0, first_conv_descr=dict(conv), middle_conv_descr=dict(conv), **kw)
    with pytest.raises(AssertionError, match="dict or SimpleNamespace"):
        GNN(conv_layers=2, first_conv_descr=None, middle_conv_descr=dict(conv), **kw)
    # skip: the heads read the input and every layer's output; three distinct layers when not fixed
    net = GNN(conv_layers=3, skip=True, first_conv_descr={"layer_type": OracleLayer, "args": dict(conv["args"])},
              middle_conv_descr={"layer_type": OracleLayer, "args": dict(conv["args"])}, **kw).eval()
    assert len(net.conv_layers) == 3 and net.gru is None and net.nodes_read_out.in_size == 2 + 3 * 4 == net.graph_read_out.set2set.nin
    adj = torch.ones(2, 5, 5) - torch.eye(5)
    nodes, graph = net(torch.randn(2, 5, 2), adj)
    assert nodes.shape == (2, 5, 1) and graph.shape == (2, 1)


# ---- the knob and the predicate ----------------------------------------------------------------------------------------------------
def test_route_is_off_by_default_and_read_from_the_environment(monkeypatch):
    monkeypatch.delenv("PNA_AMD_S2S_ROWS", raising=False)
    try:
        assert importlib.reload(PF).S2S_ROWS == 0
        monkeypatch.setenv("PNA_AMD_S2S_ROWS", "4096")
        assert importlib.reload(PF).S2S_ROWS == 4096
    finally:
        monkeypatch.delenv("PNA_AMD_S2S_ROWS", raising=False)
        importlib.reload(PF)


class _OnGpu:
    """A stand-in for a tensor on the GPU (the predicate reads shape, dtype, is_cuda, device, dim and is_contiguous)."""

    def __init__(self, *shape, dtype=torch.float32, contiguous=True):
        self.shape, self.dtype, self.is_cuda, self.device = torch.Size(shape), dtype, True, torch.device("cpu")
        self._c = contiguous

    def dim(self):
        return len(self.shape)

    def is_contiguous(self):
        return self._c


def test_one_call_path_clause_by_clause(monkeypatch):
    x = _OnGpu(16, 15, 16)
    monkeypatch.setattr(PF, "S2S_ROWS", 0)
    assert not layers.Set2Set(16)._one_call_path(None)                             # the knob at 0: nothing is looked at
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))      # the parameters' residency without a GPU
    assert not layers.Set2Set(16)._one_call_path(x)
    monkeypatch.setattr(PF, "S2S_ROWS", 16 * 15)
    assert layers.Set2Set(16)._one_call_path(x) and layers.Set2Set(16).eval()._one_call_path(x)
    assert layers.Set2Set(16, steps=3)._one_call_path(x) and layers.Set2Set(16, steps=128)._one_call_path(x)
    monkeypatch.setattr(PF, "S2S_ROWS", 16 * 15 - 1)
    assert not layers.Set2Set(16)._one_call_path(x)                                # more rows than the knob covers
    monkeypatch.setattr(PF, "S2S_ROWS", 1 << 20)
    assert not layers.Set2Set(16, steps=129)._one_call_path(x)
    assert not layers.Set2Set(16)._one_call_path(_OnGpu(240, 16)) and not layers.Set2Set(16)._one_call_path(_OnGpu(16, 15, 8))
    assert not layers.Set2Set(16)._one_call_path(_OnGpu(16, 15, 16, dtype=torch.float64))
    assert not layers.Set2Set(16)._one_call_path(_OnGpu(16, 15, 16, contiguous=False))
    cpu = _OnGpu(16, 15, 16)
    cpu.is_cuda = False
    assert not layers.Set2Set(16)._one_call_path(cpu)
    other = _OnGpu(16, 15, 16)
    other.device = torch.device("meta")
    assert not layers.Set2Set(16)._one_call_path(other)                            # the parameters are not on x's device
    assert not layers.Set2Set(16, num_layers=2)._one_call_path(x) and not layers.Set2Set(16, nhid=33)._one_call_path(x)
    assert not layers.Set2Set(16).double()._one_call_path(x)
    nobias = layers.Set2Set(16)
    nobias.lstm = nn.LSTM(32, 16, batch_first=True, bias=False)
    assert not nobias._one_call_path(x)
    assert layers.Set2Set(32)._one_call_path(_OnGpu(2, 128, 32)) and layers.Set2Set(1)._one_call_path(_OnGpu(1, 1, 1))
    assert not layers.Set2Set(32)._one_call_path(_OnGpu(2, 129, 32)) and not layers.Set2Set(33)._one_call_path(_OnGpu(2, 15, 33))
    assert layers.Set2Set(32, steps=5)._one_call_path(_OnGpu(2, 128, 32)) and not layers.Set2Set(32, steps=5)._one_call_path(_OnGpu(2, 129, 32))
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: False))
    assert not layers.Set2Set(16)._one_call_path(x)                                # parameters on the host


def test_knob_off_or_a_cpu_tensor_runs_the_loop(monkeypatch):
    calls = []
    monkeypatch.setattr(AG, "set2set", lambda *a: calls.append(1))
    c = C.s2s_case("steps3")
    m = _loop_module(c)
    assert PF.S2S_ROWS == 0
    with torch.no_grad():
        off = m(c["x"])
        monkeypatch.setattr(PF, "S2S_ROWS", 1 << 20)
        on = m(c["x"])                                                             # a CPU tensor: still the loop
        head = layers.S2SReadout(16, 16, 3).eval()
        assert head(c["x"]).shape == (c["B"], 3)
    assert not calls and torch.equal(off, on)
    assert not [k for k in list(m.__dict__) + list(m.lstm.__dict__) if str(k).startswith("_pna_amd")]
    src = open(os.path.join(ROOT, "pna_amd", "autograd.py")).read()
    body = src[src.index("_s2s_ws = {}"):]
    assert "memo(" not in body and "__dict__" not in body and "_pna_amd_" not in body


# ---- the formulas ------------------------------------------------------------------------------------------------------------------------
def test_lds_bytes_and_fits_equal_the_kernels_own_check():
    L = _lib.lib()
    for N in (1, 2, 15, 16, 17, 63, 64, 65, 97, 127, 128):
        for D in (1, 2, 3, 15, 16, 17, 31, 32):
            want = L.pna_set2set_lds_bytes(N, D)
            PI, PH = (2 * D) | 1, D | 1
            assert want == PF.set2set_lds_bytes(N, D) == -(-4 * (4 * D * (PI + PH) + N * PH + 12 * D * D + N * D + 26 * D + 2 * N + 4) // 16) * 16
            assert 0 < want <= 160 * 1024                                          # the whole scope fits: PNA_S2S_MAX_WIDTH stays 32
            for steps in (1, N, 128):
                assert PF.set2set_fits(N, D, steps) and L.pna_set2set_workspace_bytes(1, N, D, steps) > 0
            for steps in (0, 129):
                assert not PF.set2set_fits(N, D, steps) and L.pna_set2set_workspace_bytes(1, N, D, steps) == -1
    assert L.pna_set2set_lds_bytes(128, 32) == 136976
    for bad in ((0, 1), (129, 1), (1, 0), (1, 33), (-1, 16), (15, -1)):
        assert L.pna_set2set_lds_bytes(*bad) == -1 == PF.set2set_lds_bytes(*bad) and not PF.set2set_fits(*bad, 1), bad


def test_workspace_bytes_are_monotone_and_equal_the_mirror():
    L = _lib.lib()
    slab = _lib.PNA_S2S_MAX_SLABS
    for N, D, steps in ((15, 16, 15), (97, 16, 97), (128, 32, 128), (1, 1, 1), (5, 16, 5), (15, 16, 3), (64, 31, 128)):
        last = 0
        for B in (1, 2, 3, slab - 1, slab, slab + 1, 2 * slab, 2 * slab + 1, 10 * slab + 7, 10 ** 6):
            per = -(-B // slab)                                                    # graphs per slab
            assert -(-B // per) <= min(B, slab)                                    # the slabs in use never outnumber the images
            want = min(B, slab) * (12 * D * D + 4 * D + steps * (7 * D + N)) * 4
            assert L.pna_set2set_workspace_bytes(B, N, D, steps) == want == PF.set2set_workspace_bytes(B, N, D, steps)
            assert want >= last
            last = want
    assert -(-slab // slab) == 1 and -(-(slab + 1) // slab) == 2
    for args in ((0, 8, 4, 8), (-1, 8, 4, 8), (2 ** 24, 128, 4, 8), (2 ** 31, 1, 4, 1), (1, 129, 4, 8), (1, 0, 4, 8), (1, 8, 0, 8), (1, 8, 33, 8),
                 (1, 8, 4, 0), (1, 8, 4, 129)):
        assert L.pna_set2set_workspace_bytes(*args) == -1 == PF.set2set_workspace_bytes(*args), args
    assert L.pna_set2set_workspace_bytes(2 ** 24 - 1, 128, 4, 8) > 0 and PF.set2set_workspace_bytes(2 ** 24 - 1, 128, 4, 8) > 0


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_short_structs_are_refused():
    L = _lib.lib()
    for name in ("pna_set2set_fwd_f32", "pna_set2set_bwd_f32", "pna_set2set_workspace_bytes", "pna_set2set_lds_bytes"):
        assert hasattr(L, name), name
    assert L.pna_abi_version() == _lib.PNA_ABI_VERSION == 23
    header = open(os.path.join(ROOT, "include", "pna_amd.h")).read()
    assert "23, additive: + pna_set2set_fwd_f32" in header and "23, additive: + pna_tower_layer_bf16" in header
    for cite in ("models/layers.py:22-98", ":271-289", "models/pytorch/gnn_framework.py:83,108"):
        assert cite in header, cite
    cls = _lib.PnaSet2setArgs
    for fn in (L.pna_set2set_fwd_f32, L.pna_set2set_bwd_f32):
        a = cls()
        assert a.struct_size == ctypes.sizeof(cls)
        for short in (0, ctypes.sizeof(cls) - 8):
            a.struct_size = short
            assert fn(ctypes.byref(a), None) == -1 and b"struct_size" in L.pna_last_error()
        a.struct_size = ctypes.sizeof(cls)
        assert fn(ctypes.byref(a), None) == -1 and b"struct_size" not in L.pna_last_error()              # all-zero: outside the scope
        assert fn(None, None) == -1
    assert re.search(r"class PnaSet2setArgs\(_PnaArgs\)", open(os.path.join(ROOT, "INTEGRATION.md")).read())


def test_every_scope_clause_refuses_with_its_message():
    """No launch happens: every call below is refused on the host (the pointers are never dereferenced there)."""
    L = _lib.lib()
    buf = (ctypes.c_float * 64)()
    ptr = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16

    def args(**kw):
        a = _lib.PnaSet2setArgs()
        a.B, a.N, a.D, a.steps, a.dtype = 2, 15, 16, 15, _lib.PNA_S2S_F32
        for f in ("x", "w_ih", "w_hh", "b_ih", "b_hh", "out", "grad_out", "grad_x", "workspace"):
            setattr(a, f, ptr)
        a.workspace_bytes = 1 << 40
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    both = (L.pna_set2set_fwd_f32, L.pna_set2set_bwd_f32)
    for kw, text, fns in (
            (dict(dtype=1), b"fp32 only", both),
            (dict(D=0), b"1 <= D <= 32", both), (dict(D=33), b"1 <= D <= 32", both),
            (dict(N=0), b"1 <= N <= 128", both), (dict(N=129), b"1 <= N <= 128", both),
            (dict(steps=0), b"1 <= steps <= 128", both), (dict(steps=129), b"1 <= steps <= 128", both),
            (dict(B=0), b"B >= 1", both), (dict(B=2 ** 31 // 15 + 1), b"B N < 2^31", both),
            (dict(x=None), b"needs x", both), (dict(w_hh=None), b"needs w_ih (4D, 2D) and w_hh", both),
            (dict(b_ih=None), b"needs b_ih and b_hh", both),
            (dict(out=None), b"needs out", both[:1]), (dict(grad_out=None), b"needs grad_out", both[1:]),
            (dict(workspace=None), b"workspace", both[1:]), (dict(workspace=ptr + 4), b"16-byte aligned", both[1:]),
            (dict(workspace_bytes=PF.set2set_workspace_bytes(2, 15, 16, 15) - 4), b"pna_set2set_workspace_bytes", both[1:])):
        for fn in fns:
            assert fn(ctypes.byref(args(**kw)), None) == -1, kw
            msg = L.pna_last_error()
            assert text in msg and (b"pna_set2set_fwd_f32" if fn is both[0] else b"pna_set2set_bwd_f32") in msg, (kw, msg)


def test_the_struct_and_its_constants_have_gccs_layout(tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not available")
    cls = _lib.PnaSet2setArgs
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "pna_amd.h"', "int main(void) {",
             '  printf("PnaSet2setArgs . %zu 0\\n", sizeof(pna_set2set_args));']
    for f, *_ in cls._fields_:
        lines.append(f'  printf("PnaSet2setArgs {f} %zu %zu\\n", sizeof(((pna_set2set_args*)0)->{f}), offsetof(pna_set2set_args, {f}));')
    lines += ['  printf("consts %d %d %d %d %d\\n", PNA_S2S_F32, PNA_S2S_MAX_WIDTH, PNA_S2S_MAX_NODES, PNA_S2S_MAX_STEPS, PNA_S2S_MAX_SLABS);',
              "  return 0;", "}"]
    src, exe = tmp_path / "l.c", tmp_path / "l"
    src.write_text("\n".join(lines))
    subprocess.run([gcc, "-std=c11", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True)
    for row in (l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()):
        if row[0] == "consts":
            assert [int(v) for v in row[1:]] == [_lib.PNA_S2S_F32, _lib.PNA_S2S_MAX_WIDTH, _lib.PNA_S2S_MAX_NODES, _lib.PNA_S2S_MAX_STEPS,
                                                 _lib.PNA_S2S_MAX_SLABS] == [0, 32, 128, 128, 256]
        elif row[1] == ".":
            assert ctypes.sizeof(cls) == int(row[2])
        else:
            fld = getattr(cls, row[1])
            assert (fld.size, fld.offset) == (int(row[2]), int(row[3])), row
    assert _lib.PNA_S2S_MAX_NODES == _lib.PNA_DENSE_MAX_NODES                      # the dense layer's bound


# ---- the compiler's report ---------------------------------------------------------------------------------------------------------------
def test_no_kernel_of_the_file_uses_scratch(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
           "-S", "--cuda-device-only", "-o", str(tmp_path / "out.s"), os.path.join(CSRC, "pna_set2set.hip"), "-Rpass-analysis=kernel-resource-usage"]
    out = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    names = re.findall(r"Function Name: (\S+)", out)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", out)]
    assert len(names) == len(scratch) == 3, names
    for k in ("k_set2set_fwd", "k_set2set_bwd", "k_set2set_final"):
        assert any(k in n for n in names), k
    assert not [(n, s) for n, s in zip(names, scratch) if s != 0]
    text = open(str(tmp_path / "out.s")).read()
    assert "atomic" not in text and "v_mfma" not in text                            # no atomics of any kind; the vector ALU alone
    source = open(os.path.join(CSRC, "pna_set2set.hip")).read()
    assert "asm" not in re.sub(r"//.*", "", source)                                 # plain HIP C++
