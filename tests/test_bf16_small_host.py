"""CPU-side checks of pna_tower_layer_bf16 (pna_bf16_small.hip), the bf16 tower layer of molecule batches as one C call: the symbol is
exported inside ABI 23, the entry point refuses a short args struct and bad shapes without a device, the file compiles for gfx950
without scratch, functional.bf16_small_applies picks the kernel clause by clause, and the cached images follow their source tensors."""
import ctypes
import importlib
import os
import re
import shutil
import subprocess
import sys
from types import SimpleNamespace

import pytest
import torch

from pna_amd import _lib
from pna_amd import functional as PF
from pna_amd import ops
from pna_amd.dgl.pna_layer import PNALayer, PNASimpleLayer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pna_amd", "csrc")
BF = torch.bfloat16


def test_symbol_is_exported_inside_abi_23():
    L = _lib.lib()
    assert L.pna_abi_version() == _lib.PNA_ABI_VERSION == 23
    assert hasattr(L, "pna_tower_layer_bf16")
    header = open(os.path.join(ROOT, "include", "pna_amd.h")).read()
    assert re.search(r"#define PNA_ABI_VERSION 23\b", header) and "23, additive: + pna_tower_layer_bf16" in header


def test_entry_point_refuses_a_short_args_struct():
    L = _lib.lib()
    a = _lib.PnaTowerLayerBf16Args()
    assert a.struct_size == ctypes.sizeof(_lib.PnaTowerLayerBf16Args)
    for short in (0, ctypes.sizeof(_lib.PnaTowerLayerBf16Args) - 8):
        a.struct_size = short
        assert L.pna_tower_layer_bf16(ctypes.byref(a), None) == -1
        assert b"struct_size" in L.pna_last_error(), L.pna_last_error()
    assert L.pna_tower_layer_bf16(None, None) == -1 and b"null" in L.pna_last_error()


def _args(**kw):
    a = _lib.PnaTowerLayerBf16Args()
    a.V, a.n_tower, a.Fi, a.Fo, a.n_scaler, a.n_aggr, a.mix_slope = 100, 5, 75, 15, 3, 4, 0.01
    for i, code in enumerate((0, 2, 3, 4)):
        a.aggr[i] = code
    p = ctypes.c_void_p(64)
    a.rowptr = a.col = a.h = a.x_cat = a.proj_img = a.post_img = a.y = p
    a.ldh, a.ldx, a.ldy = 75, 800, 75
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_entry_point_refuses_bad_shapes_without_a_gpu():
    L = _lib.lib()
    bad = [dict(V=-1), dict(n_tower=0), dict(Fi=0), dict(Fo=0), dict(n_scaler=4), dict(n_scaler=0), dict(n_aggr=0), dict(n_aggr=9),
           dict(mix_slope=1.5), dict(col_scale=ctypes.c_void_p(64)), dict(mix_img=ctypes.c_void_p(64), No=0),
           dict(no_self_panel=1),                                                   # the simple form has one tower
           dict(rowptr=None), dict(h=None), dict(post_img=None), dict(y=None), dict(x_cat=None), dict(proj_img=None),
           dict(ldh=74), dict(ldy=74), dict(ldx=792), dict(ldx=804), dict(x_cat=ctypes.c_void_p(66)), dict(post_img=ctypes.c_void_p(72)),
           dict(residual=ctypes.c_void_p(64), ld_res=74),
           dict(edge_type=ctypes.c_void_p(64)),                                     # edge types without a table
           dict(edge_type=ctypes.c_void_p(64), edge_table=ctypes.c_void_p(64), ld_edge_table=400, n_edge_types=5),
           dict(edge_type=ctypes.c_void_p(64), edge_table=ctypes.c_void_p(64), ld_edge_table=399, n_edge_types=4)]
    for kw in bad:
        assert L.pna_tower_layer_bf16(ctypes.byref(_args(**kw)), None) == -1, kw
        assert b"pna_tower_layer_bf16" in L.pna_last_error(), (kw, L.pna_last_error())
    a = _args()
    a.aggr[2] = 99
    assert L.pna_tower_layer_bf16(ctypes.byref(a), None) == -1 and b"aggregator" in L.pna_last_error()
    # a tile beyond 160 KiB of LDS: refused by the entry point and by its host mirror alike
    assert L.pna_tower_layer_bf16(ctypes.byref(_args(Fi=300, ldh=300, ldx=3040)), None) == -1 and b"LDS" in L.pna_last_error()
    assert ops.tower_layer_bf16_lds_bytes(5, 300, 15, 4, False, No=75) > 160 * 1024
    assert ops.tower_layer_bf16_lds_bytes(5, 75, 15, 4, False, No=75) == 16 * 2 * ((5 * 320 + 8) + (96 + 8) + (96 + 8))
    assert L.pna_tower_layer_bf16(ctypes.byref(_args(V=0)), None) == 0               # nothing to do: no launch, no device needed


def test_new_kernels_use_no_scratch_and_report_their_registers(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out_s = str(tmp_path / "bf16_small.s")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
           "-S", "--cuda-device-only", "-o", out_s, os.path.join(CSRC, "pna_bf16_small.hip"), "-Rpass-analysis=kernel-resource-usage"]
    err = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    names = re.findall(r"Function Name: (\S+)", err)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", err)]
    vgprs = [int(v) for v in re.findall(r" VGPRs: (\d+)", err)]
    agprs = [int(v) for v in re.findall(r" AGPRs: (\d+)", err)]
    assert names and len(names) == len(scratch) == len(vgprs) == len(agprs)
    for n, v, a, s in zip(names, vgprs, agprs, scratch):
        print(f"{n}: {v} VGPRs + {a} AGPRs, {s} bytes of scratch")
    assert sum("k_tower_rows_bf16" in n for n in names) == 6 == len(names), names       # 3 scaler counts x {16-byte, 2-byte gather}
    assert not [(n, s) for n, s in zip(names, scratch) if s], "kernels using scratch"
    assert all(v + a <= 168 for v, a in zip(vgprs, agprs)), list(zip(names, vgprs, agprs))  # 3 wavefronts per SIMD, as compiled today
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_audit
    for n in names:
        kl = isa_audit.kernel_lines(out_s, n)
        assert not isa_audit.sgpr_hazards(kl), n
        assert not isa_audit.pk_src1_hi_selects(kl), n


def _graph(n_heavy=0):
    return SimpleNamespace(heavy_schedule=lambda: SimpleNamespace(n_heavy=n_heavy))


ZINC = dict(T=5, Fi=75, Fo=15, A=4, divide_input=False, posttrans_affine=True, No=75)


def test_bf16_small_applies_clause_by_clause(monkeypatch):
    monkeypatch.setattr(PF, "BF16_SMALL_ROWS", 4096)
    assert PF.bf16_small_applies(_graph(), 3000, **ZINC)
    assert PF.bf16_small_applies(_graph(), 4096, **ZINC)
    assert not PF.bf16_small_applies(_graph(), 4097, **ZINC)                          # above the threshold
    assert not PF.bf16_small_applies(_graph(), 0, **ZINC)                             # no rows
    assert not PF.bf16_small_applies(_graph(n_heavy=1), 3000, **ZINC)                 # a hub row
    assert not PF.bf16_small_applies(_graph(), 3000, **dict(ZINC, posttrans_affine=False))   # a deeper posttrans
    table = (torch.zeros(8, dtype=torch.int32), torch.zeros(3, 50))
    assert PF.bf16_small_applies(_graph(), 3000, edge_features=True, etab=table, **ZINC)
    assert not PF.bf16_small_applies(_graph(), 3000, edge_features=True, etab=None, **ZINC)   # per-edge rows
    assert not PF.bf16_small_applies(_graph(), 3000, **dict(ZINC, Fi=300))            # the tile does not fit the LDS
    assert PF.bf16_small_applies(_graph(), 3000, T=1, Fi=80, Fo=80, A=4, divide_input=False, posttrans_affine=True, no_self_panel=True)
    monkeypatch.setattr(PF, "BF16_SMALL_ROWS", 0)
    assert not PF.bf16_small_applies(_graph(), 3000, **ZINC)                          # the path turned off


def test_threshold_is_read_from_the_environment(monkeypatch):
    try:
        monkeypatch.setenv("PNA_AMD_BF16_SMALL_ROWS", "0")
        assert importlib.reload(PF).BF16_SMALL_ROWS == 0 and not PF.bf16_small_applies(_graph(), 100, **ZINC)
        monkeypatch.setenv("PNA_AMD_BF16_SMALL_ROWS", "123")
        assert importlib.reload(PF).BF16_SMALL_ROWS == 123
    finally:
        monkeypatch.delenv("PNA_AMD_BF16_SMALL_ROWS")
        importlib.reload(PF)


def _layer(**kw):
    args = dict(towers=2, edge_features=True, edge_dim=3)
    args.update(kw)
    return PNALayer(8, 8, "mean max min std", "identity amplification", {"log": torch.tensor(1.5)}, 0.0, True, True, **args).eval().to(BF)


def test_small_images_follow_every_tensor_they_are_built_from():
    layer = _layer()
    towers, mix = list(layer.towers), layer.mixing_network
    first = PF._small_images_bf16(towers, mix, True)
    assert PF._small_images_bf16(towers, mix, True) is first
    t1 = towers[1]
    for tensor, image in [(t1.pretrans.fully_connected[0].linear.weight, "proj"), (t1.pretrans.fully_connected[0].linear.bias, "proj_bias"),
                          (t1.pretrans.fully_connected[0].linear.weight, "edge"),
                          (t1.posttrans.fully_connected[0].linear.weight, "post"), (t1.posttrans.fully_connected[0].linear.bias, "post_bias"),
                          (t1.batchnorm_h.running_mean, "ct"), (t1.batchnorm_h.weight, "cs"),
                          (mix.linear.weight, "mix"), (mix.linear.bias, "mix_bias")]:
        before = PF._small_images_bf16(towers, mix, True)
        kept = before[image].clone()
        with torch.no_grad():
            tensor.add_(1.0)
        after = PF._small_images_bf16(towers, mix, True)
        assert after is not before and not torch.equal(after[image], kept), image
    # PNATower on its own has images of its own (no mixing network)
    alone = PF._small_images_bf16([towers[0]], None, False)
    assert alone["mix"] is None and alone is not PF._small_images_bf16(towers, mix, True)
    # layout: Fi = Fo = 4, Fp = 8, Fop = 16, Kp = 32, Khp = 32; tower 1 of the divided layer reads the second half of the input
    im = PF._small_images_bf16(towers, mix, True)
    assert im["proj"].shape == (1, 32, 32) and im["proj_bias"].shape == (32,) and im["edge"].shape == (1, 32, 32) and im["mix"].shape == (16, 32)
    assert im["post"].numel() == 2 * 2 * 16 * 32 + 2 * 16 * 32
    post, own = im["post"][:2 * 2 * 16 * 32].view(2, 2, 16, 32), im["post"][2 * 2 * 16 * 32:].view(2, 16, 32)
    W = t1.posttrans.fully_connected[0].linear.weight
    Wpre = t1.pretrans.fully_connected[0].linear.weight
    assert torch.equal(own[1, :4, :4], W[:, :4]) and torch.count_nonzero(own[1]) == torch.count_nonzero(W[:, :4])
    for s in range(2):
        for a in range(4):
            assert torch.equal(post[1, s, :4, a * 8:a * 8 + 4], W[:, 4 + (s * 4 + a) * 4:4 + (s * 4 + a + 1) * 4])
            assert torch.count_nonzero(post[1, s, :4, a * 8 + 4:a * 8 + 8]) == 0
        assert torch.count_nonzero(post[1, s, 4:]) == 0
    assert torch.equal(im["proj"][0, 8:12, 4:8], Wpre[:, :4]) and torch.equal(im["proj"][0, 24:28, 4:8], Wpre[:, 4:8])
    assert torch.count_nonzero(im["proj"][0, 8:12, :4]) == 0 and torch.count_nonzero(im["proj"][0, 12:16]) == 0
    assert torch.equal(im["proj_bias"][24:28], t1.pretrans.fully_connected[0].linear.bias) and torch.count_nonzero(im["proj_bias"][:16]) == 0
    assert torch.equal(im["edge"][0, 8:12, :3], Wpre[:, 8:])
    # the multi-launch images of the same layer are untouched by all of this
    assert PF._tower_images_bf16(towers, True) is PF._tower_images_bf16(towers, True)


def test_simple_layer_images_follow_their_tensors():
    layer = PNASimpleLayer(12, 10, "mean sum max", "identity attenuation", {"log": torch.tensor(1.5)}, 0.0, True, False).eval().to(BF)
    first = PF._small_simple_images_bf16(layer)
    assert PF._small_simple_images_bf16(layer) is first and first["post"].shape == (1, 2, 16, 64)
    lin = layer.posttrans.fully_connected[0].linear
    W = lin.weight.clone()
    for s in range(2):
        for a in range(3):
            assert torch.equal(first["post"][0, s, :10, a * 16:a * 16 + 12], W[:, (s * 3 + a) * 12:(s * 3 + a + 1) * 12])
    for tensor, image in [(lin.weight, "post"), (layer.batchnorm_h.running_var, "cs"), (layer.batchnorm_h.bias, "ct")]:
        before = PF._small_simple_images_bf16(layer)
        kept = before[image].clone()
        with torch.no_grad():
            tensor.add_(1.0)
        after = PF._small_simple_images_bf16(layer)
        assert after is not before and not torch.equal(after[image], kept), image


def test_predicate_no_longer_refuses_a_capturing_stream():
    """_bf16_towers_path does not look at the stream any more (nothing here can capture: the source is the witness)."""
    import inspect
    from pna_amd.dgl import pna_layer
    assert "is_current_stream_capturing" not in inspect.getsource(pna_layer._bf16_towers_path)
