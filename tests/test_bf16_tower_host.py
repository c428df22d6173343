"""CPU-side checks of the bf16 inference path of PNALayer / PNATower: the C entry points of pna_bf16_gather.hip and pna_bf16_contract.hip refuse a short args
struct and bad shapes, the files compile for gfx950 without scratch (register counts pinned at what the compiler gives), and the
layers' dispatch predicate picks the bf16 kernels exactly for bf16 inference with an affine pretrans on a whole graph on the GPU."""
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
from pna_amd.dgl.pna_layer import PNALayer, PNATower
from pna_amd.graph import Graph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pna_amd", "csrc")


def test_tower_entry_points_refuse_a_short_args_struct():
    L = _lib.lib()
    assert L.pna_abi_version() == 23
    for cls, fn in [(_lib.PnaGatherBf16Args, L.pna_gather_bf16), (_lib.PnaContractBf16Args, L.pna_contract_bf16)]:
        a = cls()
        assert a.struct_size == ctypes.sizeof(cls)
        for short in (0, ctypes.sizeof(cls) - 8):
            a.struct_size = short
            assert fn(ctypes.byref(a), None) == -1, (cls.__name__, short)
            assert b"struct_size" in L.pna_last_error(), L.pna_last_error()


def test_tower_entry_points_refuse_bad_shapes_without_a_gpu():
    L = _lib.lib()
    c = _lib.PnaContractBf16Args()
    c.M, c.K, c.N, c.n_scaler, c.slope = 10, 300, 75, 4, 1.0    # four scaler blocks: more than the kernel keeps
    assert L.pna_contract_bf16(ctypes.byref(c), None) == -1
    c.n_scaler, c.N = 3, 129                                     # beyond 128 columns with scaler blocks
    assert L.pna_contract_bf16(ctypes.byref(c), None) == -1 and b"N > 128" in L.pna_last_error()
    c.n_scaler, c.N = 1, 4097
    assert L.pna_contract_bf16(ctypes.byref(c), None) == -1
    c.N, c.K = 75, 0
    assert L.pna_contract_bf16(ctypes.byref(c), None) == -1
    c.K = 300
    c.h_self, c.Kh = ctypes.c_void_p(64), 75                     # a self operand without its weight image
    assert L.pna_contract_bf16(ctypes.byref(c), None) == -1 and b"h_self" in L.pna_last_error()
    c.h_self, c.Kh, c.slope = None, 0, 1.5                       # a slope that is no (leaky) ReLU
    c.a, c.w_img, c.y, c.lda, c.ldy = ctypes.c_void_p(64), ctypes.c_void_p(64), ctypes.c_void_p(64), 304, 80
    assert L.pna_contract_bf16(ctypes.byref(c), None) == -1 and b"slope" in L.pna_last_error()
    c.slope, c.lda = 0.01, 299                                   # rows shorter than K
    assert L.pna_contract_bf16(ctypes.byref(c), None) == -1
    assert [L.pna_contract_bf16_tiles(n) for n in (0, 1, 32, 33, 64, 75, 80, 96, 128, 129, 4096, 4097)] == \
        [-1, 2, 2, 4, 4, 5, 5, 8, 8, 8, 8, -1]
    g = _lib.PnaGatherBf16Args()
    g.V, g.F = 10, 513
    assert L.pna_gather_bf16(ctypes.byref(g), None) == -1
    g.F, g.n_aggr = 75, 1
    g.rowptr = g.col = g.x = g.out = ctypes.c_void_p(64)
    g.ldx, g.ldo = 80, 80
    g.aggr[0] = 99                                               # no such aggregator
    assert L.pna_gather_bf16(ctypes.byref(g), None) == -1
    g.aggr[0] = _lib.AGG_CODES["mean"]
    g.dst_term, g.ld_dst = ctypes.c_void_p(64), 74               # destination rows shorter than F
    assert L.pna_gather_bf16(ctypes.byref(g), None) == -1 and b"ld_dst" in L.pna_last_error()
    g.ld_dst = 80
    g.edge_type = ctypes.c_void_p(64)                            # edge types without a table
    assert L.pna_gather_bf16(ctypes.byref(g), None) == -1 and b"edge_type" in L.pna_last_error()
    g.edge_type, g.ldo = None, 75                                # an output pitch that is not 16-byte aligned
    assert L.pna_gather_bf16(ctypes.byref(g), None) == -1


# the largest VGPR count of the gather kernels and the largest VGPR + AGPR sum of the contraction kernels, as compiled today: a
# change of code that costs registers shows up here (the test prints every kernel's counts)
GATHER_VGPR_MAX = 145
CONTRACT_VGPR_MAX = 372


def test_tower_kernels_use_no_scratch_and_report_their_registers(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_audit
    seen = []
    for src in ("pna_bf16_gather.hip", "pna_bf16_contract.hip"):
        out_s = str(tmp_path / (src + ".s"))
        cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
               "-S", "--cuda-device-only", "-o", out_s, os.path.join(CSRC, src), "-Rpass-analysis=kernel-resource-usage"]
        err = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
        names = re.findall(r"Function Name: (\S+)", err)
        scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", err)]
        vgprs = [int(v) for v in re.findall(r" VGPRs: (\d+)", err)]
        agprs = [int(v) for v in re.findall(r" AGPRs: (\d+)", err)]
        assert names and len(names) == len(scratch) == len(vgprs) == len(agprs)
        # (k_posttrans_bf16 of the simple layer shares the file: its budget is tests/test_bf16_host.py's)
        keep = [i for i, n in enumerate(names) if "k_posttrans_bf16" not in n]
        names, scratch, vgprs, agprs = ([x[i] for i in keep] for x in (names, scratch, vgprs, agprs))
        for n, v, a, s in zip(names, vgprs, agprs, scratch):
            print(f"{n}: {v} VGPRs + {a} AGPRs, {s} bytes of scratch")
        assert not [(n, s) for n, s in zip(names, scratch) if s], "kernels using scratch"
        for n, v, a in zip(names, vgprs, agprs):
            lim = GATHER_VGPR_MAX if "k_gather_bf16" in n else CONTRACT_VGPR_MAX
            assert v + a <= lim and v <= 256 and a <= 256, (n, v, a)
        for n in names:
            kl = isa_audit.kernel_lines(out_s, n)
            assert not isa_audit.sgpr_hazards(kl), n
            assert not isa_audit.pk_src1_hi_selects(kl), n
        seen += names
    # 3 scaler counts x {self in block 0, self in its own set} x 4 column-tile counts; gather: 4 light-row and 2 segment instantiations
    # with and without message terms, 2 finalize
    assert sum("k_contract_bf16" in n for n in seen) == 24 and sum("k_gather_bf16" in n for n in seen) == 14, seen


def _layer(dtype, **kw):
    args = dict(towers=2, edge_features=False, edge_dim=0)
    args.update(kw)
    in_dim, out_dim = args.pop("in_dim", 8), args.pop("out_dim", 8)
    layer = PNALayer(in_dim, out_dim, "mean max min std", "identity amplification", {"log": torch.tensor(1.5)}, 0.0, True, True, **args)
    return layer.eval().to(dtype)


def _feat(dtype, is_cuda=True, requires_grad=False):
    return SimpleNamespace(dtype=dtype, is_cuda=is_cuda, requires_grad=requires_grad)


BF, F32 = torch.bfloat16, torch.float32


def test_dispatch_predicate_takes_bf16_inference_only():
    g = Graph(torch.tensor([0, 1, 2]), torch.tensor([1, 2, 0]), 3)
    bf = _layer(BF)
    with torch.no_grad():
        assert bf._bf16_path(g, _feat(BF))
        assert bf.towers[0]._bf16_path(g, _feat(BF))
        # fp32 / fp16 features, or an fp32 layer: never
        assert not bf._bf16_path(g, _feat(F32))
        assert not bf._bf16_path(g, _feat(torch.float16))
        assert not _layer(F32)._bf16_path(g, _feat(F32))
        assert not _layer(F32)._bf16_path(g, _feat(BF))
        assert not _layer(F32).towers[0]._bf16_path(g, _feat(BF))
        # one parameter or buffer left in fp32
        mixed = copy.deepcopy(bf)
        mixed.towers[1].batchnorm_h.running_var.data = mixed.towers[1].batchnorm_h.running_var.data.float()
        assert not mixed._bf16_path(g, _feat(BF))
        mixed = copy.deepcopy(bf)
        mixed.mixing_network.linear.bias.data = mixed.mixing_network.linear.bias.data.float()
        assert not mixed._bf16_path(g, _feat(BF))
        mixed = copy.deepcopy(bf)
        mixed.towers[0].pretrans.fully_connected[0].linear.weight.data = mixed.towers[0].pretrans.fully_connected[0].linear.weight.data.float()
        assert not mixed._bf16_path(g, _feat(BF))
        # features on the host
        assert not bf._bf16_path(g, _feat(BF, is_cuda=False))
        # training mode, of the layer or of one tower
        bf.train()
        assert not bf._bf16_path(g, _feat(BF))
        bf.eval()
        bf.towers[1].train()
        assert not bf._bf16_path(g, _feat(BF))
        bf.eval()
        assert bf._bf16_path(g, _feat(BF))
        # something other than a whole Graph (a sharded graph is a Graph subclass)
        sub = type("ShardLike", (Graph,), {})(torch.tensor([0, 1]), torch.tensor([1, 0]), 2)
        assert not bf._bf16_path(sub, _feat(BF))
        # a pretrans MLP with a hidden layer; a deeper posttrans is served (its first Linear on the kernel)
        assert not _layer(BF, pretrans_layers=2)._bf16_path(g, _feat(BF))
        assert _layer(BF, posttrans_layers=2)._bf16_path(g, _feat(BF))
        # edge features: bf16 rows on the GPU, nothing else
        ef = _layer(BF, edge_features=True, edge_dim=3)
        assert ef._bf16_path(g, _feat(BF), _feat(BF))
        assert not ef._bf16_path(g, _feat(BF), _feat(F32))
        assert not ef._bf16_path(g, _feat(BF), _feat(BF, is_cuda=False))
        assert not ef._bf16_path(g, _feat(BF), None)
        assert bf._bf16_path(g, _feat(BF), _feat(F32))            # a layer that does not read them does not look at them
        # more output columns than the contraction holds
        assert _layer(BF, in_dim=128, out_dim=128)._bf16_path(g, _feat(BF))
        assert not _layer(BF, in_dim=8, out_dim=130)._bf16_path(g, _feat(BF))
        assert not _layer(BF, in_dim=132, out_dim=132)._bf16_path(g, _feat(BF))
    # a gradient is required: features that require grad, or grad mode with trainable parameters
    with torch.enable_grad():
        assert not bf._bf16_path(g, _feat(BF))
        for p in bf.parameters():
            p.requires_grad_(False)
        assert bf._bf16_path(g, _feat(BF))
        assert not bf._bf16_path(g, _feat(BF, requires_grad=True))


def test_bf16_calls_outside_the_predicate_keep_todays_error():
    """bf16 training and a bf16 layer with a deep pretrans reach the fp32 code, which refuses bf16 as before."""
    g = Graph(torch.tensor([0, 1, 2]), torch.tensor([1, 2, 0]), 3)
    h, sn = torch.zeros(3, 8, dtype=BF), torch.ones(3, 1, dtype=BF)
    with pytest.raises((TypeError, RuntimeError)):
        _layer(BF).train()(g, h, None, sn)
    with torch.no_grad(), pytest.raises((TypeError, RuntimeError)):
        _layer(BF, pretrans_layers=2)(g, h, None, sn)


def test_weight_images_follow_every_tensor_they_are_built_from():
    """The cached images are rebuilt when ANY of their source tensors changes in place: pretrans and posttrans weights and biases
    of a later tower and the BatchNorm statistics (on the host: the images are plain tensor code)."""
    from pna_amd import functional as PF
    layer = _layer(BF, towers=2, edge_features=True, edge_dim=3)
    towers = list(layer.towers)
    first = PF._tower_images_bf16(towers, True)
    assert PF._tower_images_bf16(towers, True) is first
    t1 = towers[1]
    for tensor, image in [(t1.pretrans.fully_connected[0].linear.weight, "proj"), (t1.pretrans.fully_connected[0].linear.bias, "proj_bias"),
                          (t1.posttrans.fully_connected[0].linear.weight, "post"), (t1.posttrans.fully_connected[0].linear.bias, "post_bias"),
                          (t1.batchnorm_h.running_mean, "ct"), (t1.batchnorm_h.weight, "cs")]:
        before = PF._tower_images_bf16(towers, True)
        with torch.no_grad():
            tensor.add_(1.0)
        after = PF._tower_images_bf16(towers, True)
        assert after is not before and not torch.equal(after[image], before[image]), image
    # layout: tower 1 of a divide_input layer reads the second half of the input and writes the second half of the output
    im = PF._tower_images_bf16(towers, True)
    Fi, No, P = 4, 4, im["P"]
    assert P == 8 and im["proj"].shape == (1, 32, 32) and im["post"].shape == (2, 32, 32) and im["self"].shape == (1, 32, 32)
    assert torch.count_nonzero(im["proj"][0, :Fi, Fi:]) == 0 and torch.count_nonzero(im["proj"][0, Fi:2 * Fi, :Fi]) == 0
    W = t1.posttrans.fully_connected[0].linear.weight
    assert torch.equal(im["self"][0, No:2 * No, Fi:2 * Fi], W[:, :Fi])
    A = 4
    for s in range(2):
        for a in range(A):
            assert torch.equal(im["post"][s, No:2 * No, a * P + Fi:a * P + 2 * Fi], W[:, Fi + (s * A + a) * Fi:Fi + (s * A + a + 1) * Fi])
            assert torch.count_nonzero(im["post"][s, No:2 * No, a * P:a * P + Fi]) == 0
