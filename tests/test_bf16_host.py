"""CPU-side checks of the bf16 inference path of PNASimpleLayer: the C entry points refuse a short args struct, its kernels
(pna_bf16_gather.hip, pna_bf16_contract.hip) compile without scratch and inside their register budget, and the layer's dispatch predicate picks the bf16 kernels exactly for
bf16 inference on a whole graph on the GPU -- never for an fp32 call."""
import copy
import ctypes
import os
import re
import shutil
import subprocess
import sys
from types import SimpleNamespace

import pytest
import torch

from pna_amd import _lib
from pna_amd.dgl.pna_layer import PNASimpleLayer
from pna_amd.graph import Graph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pna_amd", "csrc")


def test_bf16_entry_points_refuse_a_short_args_struct():
    L = _lib.lib()
    for cls, fn in [(_lib.PnaSegreduceBf16Args, L.pna_segreduce_fwd_bf16), (_lib.PnaPosttransBf16Args, L.pna_posttrans_bf16)]:
        a = cls()
        assert a.struct_size == ctypes.sizeof(cls)
        for short in (0, ctypes.sizeof(cls) - 8):
            a.struct_size = short
            assert fn(ctypes.byref(a), None) == -1, (cls.__name__, short)
            assert b"struct_size" in L.pna_last_error(), L.pna_last_error()


def test_bf16_entry_points_refuse_bad_shapes_without_a_gpu():
    L = _lib.lib()
    a = _lib.PnaPosttransBf16Args()
    a.M, a.K, a.N, a.n_scaler = 10, 300, 75, 4                  # four scaler blocks: more than the kernel keeps
    assert L.pna_posttrans_bf16(ctypes.byref(a), None) == -1
    a.n_scaler, a.N = 3, 129                                     # out_dim beyond 128
    assert L.pna_posttrans_bf16(ctypes.byref(a), None) == -1
    a.N, a.K = 75, 75                                            # K not a multiple of 8
    assert L.pna_posttrans_bf16(ctypes.byref(a), None) == -1
    assert [L.pna_posttrans_bf16_tiles(n) for n in (0, 1, 32, 33, 64, 75, 80, 96, 128, 129)] == [-1, 2, 2, 4, 4, 5, 5, 8, 8, -1]
    s = _lib.PnaSegreduceBf16Args()
    s.V, s.F = 10, 513
    assert L.pna_segreduce_fwd_bf16(ctypes.byref(s), None) == -1
    assert L.pna_segreduce_bf16_partials_bytes(3, 75) == 3 * 4 * 80 * 4


def test_bf16_kernels_use_no_scratch_and_fit_their_register_budget(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_audit
    count = {}
    for src in ("pna_bf16_gather.hip", "pna_bf16_contract.hip"):
        out_s = str(tmp_path / (src + ".s"))
        cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
               "-S", "--cuda-device-only", "-o", out_s, os.path.join(CSRC, src), "-Rpass-analysis=kernel-resource-usage"]
        err = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
        names = re.findall(r"Function Name: (\S+)", err)
        scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", err)]
        vgprs = [int(v) for v in re.findall(r" VGPRs: (\d+)", err)]
        assert names and len(names) == len(scratch) == len(vgprs)
        assert not [(n, s) for n, s in zip(names, scratch) if s], "kernels using scratch"
        # the plain gather (MSG = false: pna_segreduce_fwd_bf16) keeps >= 5 wavefronts per SIMD (<= 96 registers); the contractions
        # stay in the 256 architectural VGPRs
        plain = re.compile(r"k_gather_bf16I(Lb[01]E){2}Lb0EEE|k_gather_bf16_segILb[01]ELb0EEE|k_gather_bf16_fin")
        for n, v in zip(names, vgprs):
            assert v <= (96 if plain.search(n) else 256), (n, v)
            kind = "plain" if plain.search(n) else "msg" if "k_gather_bf16" in n else "posttrans" if "k_posttrans_bf16" in n else "contract"
            count[kind] = count.get(kind, 0) + 1
        for n in names:
            kl = isa_audit.kernel_lines(out_s, n)
            assert not isa_audit.sgpr_hazards(kl), n
            assert not isa_audit.pk_src1_hi_selects(kl), n
    # gather: 4 light-row and 2 segment instantiations with and without message terms, 2 finalize; posttrans: 3 scaler counts x 4
    # column-tile counts; contraction: those x {self in block 0, self in its own set}
    assert count == {"plain": 8, "msg": 6, "posttrans": 12, "contract": 24}, count


def _layer(dtype):
    layer = PNASimpleLayer(8, 8, "mean max min std", "identity amplification", {"log": torch.tensor(1.5)}, 0.0, True, True)
    return layer.eval().to(dtype)


def _feat(dtype, is_cuda=True, requires_grad=False):
    return SimpleNamespace(dtype=dtype, is_cuda=is_cuda, requires_grad=requires_grad)


def test_dispatch_predicate_takes_bf16_inference_only():
    g = Graph(torch.tensor([0, 1, 2]), torch.tensor([1, 2, 0]), 3)
    bf = _layer(torch.bfloat16)
    with torch.no_grad():
        assert bf._bf16_path(g, _feat(torch.bfloat16))
        # fp32 / fp16 features, or an fp32 layer: never
        assert not bf._bf16_path(g, _feat(torch.float32))
        assert not bf._bf16_path(g, _feat(torch.float16))
        assert not _layer(torch.float32)._bf16_path(g, _feat(torch.float32))
        assert not _layer(torch.float32)._bf16_path(g, _feat(torch.bfloat16))
        # one parameter or buffer left in fp32
        mixed = copy.deepcopy(bf)
        mixed.batchnorm_h.running_var.data = mixed.batchnorm_h.running_var.data.float()
        assert not mixed._bf16_path(g, _feat(torch.bfloat16))
        mixed = copy.deepcopy(bf)
        mixed.posttrans.fully_connected[0].linear.bias.data = mixed.posttrans.fully_connected[0].linear.bias.data.float()
        assert not mixed._bf16_path(g, _feat(torch.bfloat16))
        # features on the host
        assert not bf._bf16_path(g, _feat(torch.bfloat16, is_cuda=False))
        # training mode
        bf.train()
        assert not bf._bf16_path(g, _feat(torch.bfloat16))
        bf.eval()
        # something other than a whole Graph (a sharded graph is a Graph subclass)
        sub = type("ShardLike", (Graph,), {})(torch.tensor([0, 1]), torch.tensor([1, 0]), 2)
        assert not bf._bf16_path(sub, _feat(torch.bfloat16))
    # a gradient is required: features that require grad, or grad mode with trainable parameters
    with torch.enable_grad():
        assert not bf._bf16_path(g, _feat(torch.bfloat16))
        for p in bf.parameters():
            p.requires_grad_(False)
        assert bf._bf16_path(g, _feat(torch.bfloat16))
        assert not bf._bf16_path(g, _feat(torch.bfloat16, requires_grad=True))


def test_bf16_call_outside_the_predicate_keeps_todays_type_error():
    """bf16 training (and every other case the predicate refuses) reaches the fp32 code, which refuses bf16 as before."""
    g = Graph(torch.tensor([0, 1, 2]), torch.tensor([1, 2, 0]), 3)
    bf = _layer(torch.bfloat16).train()
    with pytest.raises((TypeError, RuntimeError)):
        bf(g, torch.zeros(3, 8, dtype=torch.bfloat16))
