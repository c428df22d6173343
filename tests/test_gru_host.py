"""Host side of the GRU cell route (no GPU): the float64 references of tests/gru_cases.py against float64 autograd through torch.nn.GRU,
torch's own fp32 CPU nn.GRU inside the derived bars (a check of the bars, not of the kernel), the route predicates clause by clause, the
exported symbols with the struct's layout and the scope checks, the workspace formula, state_dict compatibility, and the compiler's
resource report of pna_gru.hip."""
import ctypes
import importlib
import os
import re
import shutil
import subprocess

import pytest
import torch
import torch.nn as nn

import gru_cases as C
from pna_amd import _lib, layers, nets
from pna_amd import functional as PF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pna_amd", "csrc")
HOST_CASES = [("mt_first", 17), ("mt_later", 33), ("floor", 2), ("h75", 65), ("h128", 15), ("pad_x", 33), ("pad_h", 33), ("rect", 209)]


def _torch_gru(c, dtype):
    """nn.GRU carrying the case's parameters, and its length-1 run on the PADDED inputs with every leaf requiring a gradient."""
    IN, H = c["w_ih"].shape[1], c["w_hh"].shape[1]
    gru = nn.GRU(IN, H).to(dtype)
    for name in C.PARAMS:
        getattr(gru, C.NN_NAMES[name]).data.copy_(c[name].to(dtype))
    x = c["x"].to(dtype).requires_grad_(True)
    h = c["h"].to(dtype).requires_grad_(True)
    out = gru(C._pad(x, IN).unsqueeze(0), C._pad(h, H).unsqueeze(0))[1][0]
    leaves = [x, h] + [getattr(gru, C.NN_NAMES[name]) for name in C.PARAMS]
    return out, leaves


# ---- the references and the bars ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width,V", HOST_CASES)
def test_float64_formulas_are_float64_autograd_through_nn_gru(width, V):
    c = C.gru_case(width, V)
    f, g = C.gru_grad_ref64(*C.case_params(c), c["go"])
    out, leaves = _torch_gru(c, torch.float64)
    torch.testing.assert_close(f["out"], out.detach(), rtol=1e-12, atol=1e-12)
    grads = torch.autograd.grad(out, leaves, c["go"].double())
    for name, got in zip(("x", "h") + C.PARAMS, grads):
        torch.testing.assert_close(g[name], got, rtol=1e-12, atol=1e-12)


def _torch_fp32_inside_the_bars(width, V, scale):
    c = C.gru_case(width, V, scale=scale)
    f, g = C.gru_grad_ref64(*C.case_params(c), c["go"])
    bars = C.gru_bars(*C.case_params(c), c["go"])
    out, leaves = _torch_gru(c, torch.float32)
    grads = torch.autograd.grad(out, leaves, c["go"])
    assert torch.isfinite(out).all() and all(torch.isfinite(t).all() for t in grads)
    worst = {"out": C.worst_ratio(out.detach(), f["out"], bars["out"])}
    for name, got in zip(("x", "h") + C.PARAMS, grads):
        worst[name] = C.worst_ratio(got, g[name], bars[name])
    print("CPU_RATIO", width, V, scale, {k: round(v, 3) for k, v in worst.items()})
    assert all(v <= 1.0 for v in worst.values()), worst


@pytest.mark.parametrize("width,V", C.KERNEL_CASES, ids=[f"{w}-{v}" for w, v in C.KERNEL_CASES])
def test_torchs_fp32_cpu_gru_stays_inside_the_derived_bars(width, V):
    """Every case the GPU kernel tests walk: a check of the bars, not of the kernel."""
    _torch_fp32_inside_the_bars(width, V, None)


@pytest.mark.parametrize("scale", [30.0, 100.0])
@pytest.mark.parametrize("width,V", HOST_CASES + [("h110", 15)])
def test_torchs_fp32_cpu_gru_stays_inside_the_derived_bars_when_saturated(width, V, scale):
    _torch_fp32_inside_the_bars(width, V, scale)


def test_the_bars_are_tight_enough_to_see_a_wrong_gate():
    """A bar that admits everything checks nothing: r and z swapped, gi_n and gh_n merged under r, or fp16-rounded weights all leave
    the bars by orders of magnitude."""
    c = C.gru_case("h75", 65)
    f = C.gru_ref64(*C.case_params(c))
    bars = C.gru_bars(*C.case_params(c))
    H = 75
    merged = torch.tanh(f["r"] * (f["gi_n"] + f["gh_n"]))
    assert C.worst_ratio((1 - f["z"]) * merged + f["z"] * f["h"], f["out"], bars["out"]) > 1e3
    assert C.worst_ratio((1 - f["r"]) * f["n"] + f["r"] * f["h"], f["out"], bars["out"]) > 1e3
    half = C.gru_ref64(c["x"], c["h"], c["w_ih"].half().float(), c["w_hh"].half().float(), c["b_ih"], c["b_hh"])
    assert C.worst_ratio(half["out"], f["out"], bars["out"]) > 10
    assert float(bars["out"].max()) < 1e-3 and bars["out"].shape == (65, H)         # (outputs are O(1); the worst-case bar of a 152-term sum is ~1e-4)


def test_case_list_covers_what_it_promises():
    assert C.SLAB == _lib.PNA_GRU_SLAB_ROWS and C.MAX_SLABS == _lib.PNA_GRU_MAX_SLABS
    for w in C.WIDTHS:
        rows = [v for ww, v in C.KERNEL_CASES if ww == w]
        assert min(rows) < 16 and max(rows) >= 3 * C.SLAB                        # a sub-tile and a count spanning at least three slabs
    for w in ("mt_later", "h75"):
        assert {v for ww, v in C.KERNEL_CASES if ww == w} == set(C.ROWS)
    assert {2, 15, 16, 17, 33, C.SLAB - 1, C.SLAB, C.SLAB + 1} <= set(C.ROWS)
    assert len(set(C.KERNEL_CASES)) == len(C.KERNEL_CASES)
    for scale in (30.0, 100.0):
        c = C.gru_case("mt_later", 33, scale=scale)
        f = C.gru_ref64(*C.case_params(c))
        top = max(float(f["a_r"].abs().max()), float(f["a_z"].abs().max()), float((f["gi_n"] + f["r"] * f["gh_n"]).abs().max()))
        assert abs(top - scale) < 0.05 * scale


# ---- the knob and the predicates ---------------------------------------------------------------------------------------------------
def test_route_is_off_by_default_and_read_from_the_environment(monkeypatch):
    monkeypatch.delenv("PNA_AMD_GRU_ROWS", raising=False)
    try:
        assert importlib.reload(PF).GRU_ROWS == 0
        monkeypatch.setenv("PNA_AMD_GRU_ROWS", "4096")
        assert importlib.reload(PF).GRU_ROWS == 4096
    finally:
        monkeypatch.delenv("PNA_AMD_GRU_ROWS", raising=False)
        importlib.reload(PF)


class _OnGpu:
    """A stand-in for rows on the GPU (the predicate reads shape, dtype, is_cuda, dim, stride, device and nothing else)."""

    def __init__(self, *shape, dtype=torch.float32, col_stride=1):
        self.shape, self.dtype, self.is_cuda, self.device, self._cs = torch.Size(shape), dtype, True, torch.device("cpu"), col_stride

    def dim(self):
        return len(self.shape)

    def stride(self, d):
        return self._cs if d == len(self.shape) - 1 else self.shape[-1] * self._cs

    def is_contiguous(self):
        return self._cs == 1

    def reshape(self, *shape):
        n = 1
        for s in self.shape:
            n *= s
        return _OnGpu(shape[0], n // shape[0], dtype=self.dtype, col_stride=self._cs)


def test_one_call_path_clause_by_clause(monkeypatch):
    G = lambda i=16, h=16: nets.GRU(i, h, "cpu")                                   # noqa: E731
    x, y = _OnGpu(40, 16), _OnGpu(40, 16)
    monkeypatch.setattr(PF, "GRU_ROWS", 0)
    assert not G()._one_call_path(None, None)                                     # the knob at 0: nothing is looked at
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))     # the parameters' residency without a GPU
    assert not G()._one_call_path(x, y)
    monkeypatch.setattr(PF, "GRU_ROWS", 4096)
    assert G()._one_call_path(x, y)
    assert G()._one_call_path(_OnGpu(40, 2), y) and G()._one_call_path(x, _OnGpu(40, 5))     # padding on either side
    assert G().eval()._one_call_path(x, y)                                        # train and eval alike
    assert G(24, 40)._one_call_path(_OnGpu(40, 24), _OnGpu(40, 40))
    assert G(128, 128)._one_call_path(_OnGpu(40, 128), _OnGpu(40, 128))
    # rows
    monkeypatch.setattr(PF, "GRU_ROWS", 39)
    assert not G()._one_call_path(x, y)                                           # more rows than the knob covers
    monkeypatch.setattr(PF, "GRU_ROWS", 40)
    assert G()._one_call_path(x, y)
    monkeypatch.setattr(PF, "GRU_ROWS", 4096)
    assert not G()._one_call_path(_OnGpu(1, 16), _OnGpu(1, 16))                   # one row: .squeeze() drops the row dimension
    assert G()._one_call_path(_OnGpu(2, 16), _OnGpu(2, 16))
    assert not G()._one_call_path(x, _OnGpu(39, 16))
    # the tensors
    assert not G()._one_call_path(_OnGpu(2, 20, 16), y)                           # 3-D
    assert not G()._one_call_path(_OnGpu(40, 16, dtype=torch.float64), y) and not G()._one_call_path(x, _OnGpu(40, 16, dtype=torch.bfloat16))
    assert not G()._one_call_path(_OnGpu(40, 16, col_stride=2), y) and not G()._one_call_path(x, _OnGpu(40, 16, col_stride=2))
    flat = _OnGpu(40, 16)
    flat.stride = lambda d: (0, 1)[d]
    assert not G()._one_call_path(flat, y) and not G()._one_call_path(x, flat)      # expanded rows: a row pitch below the width
    cpu = _OnGpu(40, 16)
    cpu.is_cuda = False
    assert not G()._one_call_path(cpu, y) and not G()._one_call_path(x, cpu)
    other = _OnGpu(40, 16)
    other.device = torch.device("meta")
    assert not G()._one_call_path(other, y)                                       # not the parameters' device
    # the module
    for kw in ({"num_layers": 2}, {"bidirectional": True}, {"bias": False}, {"batch_first": True}):
        odd = G()
        odd.gru = nn.GRU(16, 16, **kw)
        assert not odd._one_call_path(x, y), kw
    assert not G().double()._one_call_path(x, y) and not G().to(torch.bfloat16)._one_call_path(x, y)
    one = G()
    one.gru.bias_hh_l0.data = one.gru.bias_hh_l0.data.double()
    assert not one._one_call_path(x, y)                                           # one fp64 parameter
    # the widths
    assert not G(130, 16)._one_call_path(_OnGpu(40, 130), y) and not G(16, 130)._one_call_path(x, _OnGpu(40, 130))
    assert not G(16, 1)._one_call_path(x, _OnGpu(40, 1))
    assert G(1, 2)._one_call_path(_OnGpu(40, 1), _OnGpu(40, 2))
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: False))
    assert not G()._one_call_path(x, y)                                           # parameters on the host


def test_dense_gru_path_looks_at_the_row_views(monkeypatch):
    L = lambda: layers.GRU(16, 16, "cpu")                                          # noqa: E731
    monkeypatch.setattr(PF, "GRU_ROWS", 0)
    assert not L()._one_call_path(None, None)
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    monkeypatch.setattr(PF, "GRU_ROWS", 64)
    assert L()._one_call_path(_OnGpu(4, 16, 2), _OnGpu(4, 16, 16))                # B N = 64 rows, a 2-column x
    assert not L()._one_call_path(_OnGpu(4, 17, 2), _OnGpu(4, 17, 16))            # 68 rows
    assert not L()._one_call_path(_OnGpu(64, 2), _OnGpu(64, 16))                  # 2-D is nets.GRU's shape
    assert not L()._one_call_path(_OnGpu(4, 16, 2, col_stride=2), _OnGpu(4, 16, 16))
    assert not L()._one_call_path(_OnGpu(1, 1, 2), _OnGpu(1, 1, 16))              # one row
    assert not L()._one_call_path(_OnGpu(4, 16, 2), _OnGpu(4, 16, 16, dtype=torch.float64))


def test_gru_cell_fits_at_its_edges():
    assert PF.gru_cell_fits(1, 1, 1, 2) and PF.gru_cell_fits(128, 128, 128, 128) and PF.gru_cell_fits(2, 16, 16, 16)
    assert not PF.gru_cell_fits(1, 1, 1, 1) and not PF.gru_cell_fits(1, 1, 0, 2)
    assert not PF.gru_cell_fits(1, 1, 129, 2) and not PF.gru_cell_fits(1, 1, 1, 129)
    assert not PF.gru_cell_fits(0, 1, 4, 4) and not PF.gru_cell_fits(5, 1, 4, 4)
    assert not PF.gru_cell_fits(1, 0, 4, 4) and not PF.gru_cell_fits(1, 5, 4, 4)
    assert PF.gru_cell_fits(4, 4, 4, 4)


def test_knob_off_runs_the_old_lines_on_the_host():
    """With PNA_AMD_GRU_ROWS unset nothing observable changes: both modules are nn.GRU on padded rows, as the reference's are."""
    assert PF.GRU_ROWS == 0
    torch.manual_seed(0)
    g = nets.GRU(12, 12, "cpu")
    x, y = torch.randn(5, 12), torch.randn(5, 12)
    assert torch.equal(g(x, y), g.gru(x.unsqueeze(0), y.unsqueeze(0))[1].squeeze())
    d = layers.GRU(16, 16, "cpu")
    xb, yb = torch.randn(2, 3, 2), torch.randn(2, 3, 16)
    want = d.gru(torch.nn.functional.pad(xb.reshape(1, 6, 2), [0, 14]), yb.reshape(1, 6, 16))[1].reshape(2, 3, 16)
    assert torch.equal(d(xb, yb), want) and d(xb, yb).shape == (2, 3, 16)


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_short_structs_are_refused():
    L = _lib.lib()
    for name in ("pna_gru_cell_fwd_f32", "pna_gru_cell_bwd_f32", "pna_gru_cell_workspace_bytes", "pna_gru_cell_in_scope"):
        assert hasattr(L, name), name
    assert L.pna_abi_version() == _lib.PNA_ABI_VERSION == 23
    assert "23, additive: + pna_gru_cell_fwd_f32" in open(os.path.join(ROOT, "include", "pna_amd.h")).read()
    cls = _lib.PnaGruCellArgs
    for fn in (L.pna_gru_cell_fwd_f32, L.pna_gru_cell_bwd_f32):
        a = cls()
        assert a.struct_size == ctypes.sizeof(cls)
        for short in (0, ctypes.sizeof(cls) - 8):
            a.struct_size = short
            assert fn(ctypes.byref(a), None) == -1 and b"struct_size" in L.pna_last_error()
        a.struct_size = ctypes.sizeof(cls)
        assert fn(ctypes.byref(a), None) == -1 and b"struct_size" not in L.pna_last_error()              # all-zero: outside the scope
        assert fn(None, None) == -1
    assert re.search(r"class PnaGruCellArgs\(_PnaArgs\)", open(os.path.join(ROOT, "INTEGRATION.md")).read())


def test_the_struct_and_its_constants_have_gccs_layout(tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not available")
    cls = _lib.PnaGruCellArgs
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "pna_amd.h"', "int main(void) {",
             '  printf("PnaGruCellArgs . %zu 0\\n", sizeof(pna_gru_cell_args));']
    for f, *_ in cls._fields_:
        lines.append(f'  printf("PnaGruCellArgs {f} %zu %zu\\n", sizeof(((pna_gru_cell_args*)0)->{f}), offsetof(pna_gru_cell_args, {f}));')
    lines += ['  printf("consts %d %d %d\\n", PNA_GRU_F32, PNA_GRU_SLAB_ROWS, PNA_GRU_MAX_SLABS);', "  return 0;", "}"]
    src, exe = tmp_path / "l.c", tmp_path / "l"
    src.write_text("\n".join(lines))
    subprocess.run([gcc, "-std=c11", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True)
    for c, f, size, off in (l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()):
        if c == "consts":
            assert (int(f), int(size), int(off)) == (_lib.PNA_GRU_F32, _lib.PNA_GRU_SLAB_ROWS, _lib.PNA_GRU_MAX_SLABS)
        elif f == ".":
            assert ctypes.sizeof(cls) == int(size)
        else:
            fld = getattr(cls, f)
            assert (fld.size, fld.offset) == (int(size), int(off)), (f, fld.size, fld.offset, size, off)


def _scope_args(**kw):
    """An args struct inside the scope except for `kw`; the pointers are non-null but never followed: every check precedes a launch."""
    a = _lib.PnaGruCellArgs()
    a.V, a.I, a.Hc, a.input_size, a.hidden_size, a.dtype = 8, 16, 16, 16, 16, _lib.PNA_GRU_F32
    for f in ("x", "h", "w_ih", "w_hh", "b_ih", "b_hh", "out"):
        setattr(a, f, 4096)
    a.ldx = a.ldh = a.ld_wih = a.ld_whh = a.ld_out = 16
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("kw,clause", [
    ({"dtype": 1}, b"fp32 only"), ({"input_size": 0, "I": 0}, b"input_size"), ({"input_size": 129}, b"input_size"),
    ({"hidden_size": 1, "Hc": 1}, b"hidden_size"), ({"hidden_size": 129}, b"hidden_size"), ({"V": 1}, b"V >= 2"), ({"V": 0}, b"V >= 2"),
    ({"I": 0}, b"I <= input_size"), ({"I": 17}, b"I <= input_size"), ({"Hc": 0}, b"Hc <= hidden_size"), ({"Hc": 17}, b"Hc <= hidden_size"),
    ({"x": None}, b"needs x"), ({"ldx": 15}, b"needs x"), ({"h": None}, b"needs h"), ({"w_ih": None}, b"w_ih"), ({"ld_whh": 15}, b"w_hh"),
    ({"b_hh": None}, b"b_hh"), ({"out": None}, b"needs out"), ({"ld_out": 15}, b"needs out")])
def test_forward_scope_clauses_are_named(kw, clause):
    L = _lib.lib()
    assert L.pna_gru_cell_fwd_f32(ctypes.byref(_scope_args(**kw)), None) == -1
    assert clause in L.pna_last_error(), L.pna_last_error()


def test_workspace_bytes_formula_and_scope():
    L = _lib.lib()
    for H, I, Hc in ((16, 2, 16), (2, 1, 2), (75, 75, 75), (128, 128, 128), (80, 37, 80), (40, 24, 40)):
        for V in (2, 15, C.SLAB - 1, C.SLAB, C.SLAB + 1, 3 * C.SLAB + 17, C.SLAB * C.MAX_SLABS, C.SLAB * C.MAX_SLABS + 1, 52000, 10 ** 6):
            slab = max(C.SLAB, -(-V // C.MAX_SLABS))
            n_slab = -(-V // slab)
            assert n_slab <= C.MAX_SLABS and C.slab_rows(V) == slab == max(_lib.PNA_GRU_SLAB_ROWS, -(-V // _lib.PNA_GRU_MAX_SLABS))
            want = 4 * (V * 4 * H + n_slab * 3 * H * (I + Hc + 2))
            assert L.pna_gru_cell_workspace_bytes(V, I, Hc, H) == want == PF.gru_cell_workspace_bytes(V, I, Hc, H), (V, H, I, Hc)
    for V, I, Hc, H in ((1, 4, 4, 4), (0, 4, 4, 4), (2 ** 31, 4, 4, 4), (8, 0, 4, 4), (8, 129, 4, 4), (8, 4, 0, 4), (8, 4, 5, 4), (8, 4, 1, 1), (8, 4, 4, 129)):
        assert L.pna_gru_cell_workspace_bytes(V, I, Hc, H) == -1 == PF.gru_cell_workspace_bytes(V, I, Hc, H), (V, I, Hc, H)


# ---- state_dict compatibility ----------------------------------------------------------------------------------------------------------
class _Stock(nn.Module):
    """The reference's wrapper as far as the state_dict sees it (models/layers.py:242-246, nets/gru.py)."""

    def __init__(self, H):
        super().__init__()
        self.gru = nn.GRU(input_size=H, hidden_size=H)


@pytest.mark.parametrize("cls", [layers.GRU, nets.GRU])
def test_state_dict_is_interchangeable_with_a_stock_wrapper(cls):
    stock, ours = _Stock(12), cls(12, 12, "cpu")
    keys = ["gru.weight_ih_l0", "gru.weight_hh_l0", "gru.bias_ih_l0", "gru.bias_hh_l0"]
    assert list(stock.state_dict()) == keys == list(ours.state_dict())
    ours.load_state_dict(stock.state_dict(), strict=True)
    assert all(torch.equal(a, b) for a, b in zip(ours.state_dict().values(), stock.state_dict().values()))
    fresh = cls(12, 12, "cpu")
    _Stock(12).load_state_dict(fresh.state_dict(), strict=True)


# ---- the compiler's report ---------------------------------------------------------------------------------------------------------------
MAX_VGPR_ROWS = 96          # the two rows kernels stay at or under 96 VGPRs (5 wavefronts per SIMD: two 8-wavefront workgroups per CU)


def test_no_kernel_of_the_file_uses_scratch(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
           "-S", "--cuda-device-only", "-o", str(tmp_path / "out.s"), os.path.join(CSRC, "pna_gru.hip"), "-Rpass-analysis=kernel-resource-usage"]
    out = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    names = re.findall(r"Function Name: (\S+)", out)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", out)]
    vgprs = [int(v) for v in re.findall(r" VGPRs: (\d+)", out)]
    assert len(names) == len(scratch) == len(vgprs) == 4, names
    for k in ("k_gru_rows_fwd", "k_gru_rows_bwd", "k_gru_dw_slab", "k_gru_dw_final"):
        assert any(k in n for n in names), k
    assert not [(n, s) for n, s in zip(names, scratch) if s != 0]
    assert not [(n, v) for n, v in zip(names, vgprs) if "k_gru_rows" in n and v > MAX_VGPR_ROWS]
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert f"at or under {MAX_VGPR_ROWS} VGPRs" in design
    text = open(str(tmp_path / "out.s")).read()
    assert "v_mfma_f32_16x16x4_f32" in text                                          # the exact-fp32 matrix instruction
