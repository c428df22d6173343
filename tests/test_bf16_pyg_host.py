"""CPU-side checks of the bf16 inference path of the PyG front end (PNAConv, PNAConvSimple): the dispatch predicates clause by clause,
the weight images (cached per state of every source tensor; the PyG column order [x_i | x_j | enc] of a pre_nn weight lands in the
destination and source halves), the refusals of pna_edge_mlp_bf16 and of the aggregator codes, and the compiled resources of
pna_bf16_edge_mlp.hip.  None of this needs a GPU."""
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

from pna_amd import _lib, functional as PF, ops
from pna_amd.pytorch_geometric import PNAConv, PNAConvSimple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pna_amd", "csrc")
BF, F32 = torch.bfloat16, torch.float32
HIST = torch.tensor([1, 4, 3, 2])
AGGS, SCALERS = ["mean", "min", "max", "std"], ["identity", "amplification", "attenuation"]


def _conv(dtype=BF, in_c=8, out_c=8, aggs=AGGS, scalers=SCALERS, seed=0, **kw):
    torch.manual_seed(seed)
    return PNAConv(in_c, out_c, aggs, scalers, HIST, **kw).eval().to(dtype)


def _simple(dtype=BF, F=8, out=8, aggs=AGGS, scalers=SCALERS, **kw):
    torch.manual_seed(1)
    return PNAConvSimple(F, out, aggs, scalers, HIST, **kw).eval().to(dtype)


def _feat(dtype, is_cuda=True, requires_grad=False):
    return SimpleNamespace(dtype=dtype, is_cuda=is_cuda, requires_grad=requires_grad)


def test_dispatch_predicates_take_bf16_inference_only():
    conv, simple = _conv(towers=2), _simple()
    with torch.no_grad():
        assert conv._bf16_path(_feat(BF)) and simple._bf16_path(_feat(BF))
        for layer, make in ((conv, _conv), (simple, _simple)):
            # fp32 / fp16 features, an fp32 layer, features on the host
            assert not layer._bf16_path(_feat(F32)) and not layer._bf16_path(_feat(torch.float16))
            assert not make(F32)._bf16_path(_feat(F32)) and not make(F32)._bf16_path(_feat(BF))
            assert not layer._bf16_path(_feat(BF, is_cuda=False))
            # training mode
            layer.train()
            assert not layer._bf16_path(_feat(BF))
            layer.eval()
            assert layer._bf16_path(_feat(BF))
        # one parameter or buffer left in fp32
        for name in ("lin.bias", "pre_nns.1.0.weight", "post_nns.0.0.bias"):
            mixed = copy.deepcopy(conv)
            p = mixed.get_parameter(name)
            p.data = p.data.float()
            assert not mixed._bf16_path(_feat(BF)), name
        mixed = copy.deepcopy(simple)
        mixed.post_nn[0].weight.data = mixed.post_nn[0].weight.data.float()
        assert not mixed._bf16_path(_feat(BF))
        mixed = copy.deepcopy(simple)
        mixed.register_buffer("stat", torch.zeros(2))
        assert not mixed._bf16_path(_feat(BF))
        # edge features: bf16 rows on the GPU exactly when the layer was built with edge_dim
        ef = _conv(edge_dim=3)
        assert ef._bf16_path(_feat(BF), _feat(BF))
        assert not ef._bf16_path(_feat(BF), _feat(F32))
        assert not ef._bf16_path(_feat(BF), _feat(BF, is_cuda=False))
        assert ef._bf16_path(_feat(BF), _feat(BF, requires_grad=True))          # (no gradient is REQUIRED while grad mode is off)
        assert not ef._bf16_path(_feat(BF), None)
        assert not conv._bf16_path(_feat(BF), _feat(BF))             # the fp32 code refuses edge_attr without edge_dim: so does this call
        # at most 128 output columns
        assert _conv(in_c=128, out_c=128)._bf16_path(_feat(BF)) and not _conv(in_c=8, out_c=130)._bf16_path(_feat(BF))
        assert _simple(F=8, out=128)._bf16_path(_feat(BF)) and not _simple(F=8, out=129)._bf16_path(_feat(BF))
        # towers * round8(F_in) <= 512: one gathered row
        assert _conv(in_c=64, out_c=8, towers=8)._bf16_path(_feat(BF))                       # 8 * 64 = 512
        assert not _conv(in_c=65, out_c=8, towers=8)._bf16_path(_feat(BF))                   # 8 * 72
        assert not _conv(in_c=520, out_c=8, towers=8, divide_input=True)._bf16_path(_feat(BF))   # F_in = 65: 8 * round8(65) = 576
        assert _simple(F=512)._bf16_path(_feat(BF)) and not _simple(F=513)._bf16_path(_feat(BF))
        # at most 3 scalers, any of the five; all six aggregators
        five = ["identity", "amplification", "attenuation", "linear", "inverse_linear"]
        assert _conv(scalers=five[2:])._bf16_path(_feat(BF)) and _simple(scalers=five[2:])._bf16_path(_feat(BF))
        assert not _conv(scalers=five[:4])._bf16_path(_feat(BF)) and not _simple(scalers=five)._bf16_path(_feat(BF))
        six = ["sum", "mean", "min", "max", "var", "std"]
        assert _conv(aggs=six)._bf16_path(_feat(BF)) and _simple(aggs=six)._bf16_path(_feat(BF))
        # a deeper post_nn is served (its first Linear on the kernel); a deeper pre_nn while pna_edge_mlp_bf16 holds its hidden layers
        assert _conv(post_layers=3)._bf16_path(_feat(BF)) and _simple(post_layers=2)._bf16_path(_feat(BF))
        assert _conv(pre_layers=2)._bf16_path(_feat(BF)) and _conv(pre_layers=3, towers=2, edge_dim=3)._bf16_path(_feat(BF), _feat(BF))
        assert _conv(in_c=128, out_c=8, pre_layers=4)._bf16_path(_feat(BF))
        assert not _conv(in_c=129, out_c=8, pre_layers=2)._bf16_path(_feat(BF))              # F > 128
        assert _conv(in_c=129, out_c=8, pre_layers=1)._bf16_path(_feat(BF))
        assert not _conv(in_c=128, out_c=8, pre_layers=5)._bf16_path(_feat(BF))              # four hidden 128 x 128 layers: 161 KiB of LDS
    # a gradient is required: grad mode with trainable parameters, or features that require grad
    with torch.enable_grad():
        assert not conv._bf16_path(_feat(BF)) and not simple._bf16_path(_feat(BF))
        for layer in (conv, simple):
            for p in layer.parameters():
                p.requires_grad_(False)
            assert layer._bf16_path(_feat(BF)) and not layer._bf16_path(_feat(BF, requires_grad=True))
        ef = _conv(edge_dim=3)
        for p in ef.parameters():
            p.requires_grad_(False)
        assert ef._bf16_path(_feat(BF), _feat(BF)) and not ef._bf16_path(_feat(BF), _feat(BF, requires_grad=True))


def test_the_lds_mirror_is_the_librarys():
    L = _lib.lib()
    r = lambda x, m: (x + m - 1) // m * m   # noqa: E731
    for F in (1, 5, 16, 75, 80, 128):
        for nh in (1, 2, 5, 64):
            Kp = r(r(F, 8), 32)                                                    # (the test's own statement of the kernel's tile)
            want = 2 * (nh * r(F, 16) * (Kp + 16) + 64 * (Kp + 8))
            assert L.pna_edge_mlp_bf16_lds_bytes(F, nh) == want == ops.edge_mlp_bf16_lds_bytes(F, nh), (F, nh)
    assert L.pna_edge_mlp_bf16_lds_bytes(129, 1) == -1 and L.pna_edge_mlp_bf16_lds_bytes(0, 1) == -1 and L.pna_edge_mlp_bf16_lds_bytes(8, 0) == -1
    assert ops.edge_mlp_bf16_lds_bytes(128, 3) <= 160 * 1024 < ops.edge_mlp_bf16_lds_bytes(128, 4)
    assert ops.LDS_BUDGET == 160 * 1024


def test_a_pre_nn_deeper_than_the_edge_mlp_serves_takes_the_fp32_code():
    """pna_edge_mlp_bf16 refuses more than 64 hidden layers, whatever their bytes: the answer is the library's -1 (a formula of the tile
    alone gives 104 960 bytes, which would pass for a fit), and the predicate built on it sends the layer to the fp32 code."""
    assert ops.edge_mlp_bf16_lds_bytes(8, 64) == 103424 and ops.edge_mlp_bf16_lds_bytes(8, 65) == -1
    assert ops.edge_mlp_bf16_lds_bytes(129, 1) == -1 and ops.edge_mlp_bf16_lds_bytes(0, 1) == -1 and ops.edge_mlp_bf16_lds_bytes(8, 0) == -1
    with torch.no_grad():
        assert _conv(pre_layers=65)._bf16_path(_feat(BF)) and not _conv(pre_layers=66)._bf16_path(_feat(BF))


def test_bf16_calls_outside_the_predicate_keep_todays_error():
    """bf16 training, more than 3 scalers and a bf16 call on the host reach the fp32 code, which refuses as before."""
    x, ei = torch.zeros(4, 8, dtype=BF), torch.tensor([[0, 1, 2, 3], [1, 2, 3, 0]])
    with pytest.raises((TypeError, RuntimeError)):
        _conv().train()(x, ei)
    with torch.no_grad():
        for layer in (_conv(), _simple(), _simple(scalers=["identity", "amplification", "attenuation", "linear"])):
            with pytest.raises((TypeError, RuntimeError)):
                layer(x, ei)


def _changed(before, after):
    return [k for k in before if torch.is_tensor(before[k]) and not torch.equal(before[k], after[k])]


@pytest.mark.parametrize("pre_layers", [1, 3])
def test_conv_images_follow_every_tensor_they_are_built_from(pre_layers):
    """The images of both routes are rebuilt when ANY source tensor changes in place: edge_encoder, the first and every hidden pre_nn
    Linear of a later tower, the first post_nn Linear, lin."""
    conv = _conv(in_c=10, out_c=6, towers=2, divide_input=True, edge_dim=3, pre_layers=pre_layers)
    builders = [PF._pyg_conv_images_bf16] + ([PF._pyg_conv_small_images_bf16] if pre_layers == 1 else [])
    cases = [("edge_encoder.weight", "enc"), ("edge_encoder.bias", None), ("pre_nns.1.0.weight", "proj"), ("pre_nns.1.0.bias", "proj_bias"),
             ("post_nns.1.0.weight", "post"), ("post_nns.1.0.bias", "post_bias"), ("lin.weight", "mix"), ("lin.bias", None)]
    if pre_layers > 1:
        cases += [("pre_nns.1.2.weight", "mlp"), ("pre_nns.0.4.weight", "mlp"), ("pre_nns.1.4.bias", "mlp_bias")]
    for build in builders:
        first = build(conv)
        assert build(conv) is first
        for name, image in cases:
            before = build(conv)
            with torch.no_grad():
                conv.get_parameter(name).add_(1.0)
            after = build(conv)
            assert after is not before, (build.__name__, name)
            if image is not None:
                assert image in _changed(before, after), (build.__name__, name, _changed(before, after))
    # ... and a conversion drops them (DropsCachesOnConversion)
    assert "_pna_amd_bf16_images" in conv.__dict__
    conv.to(BF)
    assert "_pna_amd_bf16_images" not in conv.__dict__ and "_pna_amd_bf16_small" not in conv.__dict__


def _simple_small_images(simple, monkeypatch):
    """The images pyg_simple_bf16 hands pna_tower_layer_bf16 on its one-call route (the kernel call itself replaced by a recorder)."""
    from pna_amd.graph import Graph
    seen = []
    monkeypatch.setattr(PF, "bf16_small_applies", lambda *a, **k: True)
    monkeypatch.setattr(ops, "tower_layer_bf16", lambda *a, **k: seen.append(k) or "out")
    g = Graph(torch.tensor([0, 1, 2]), torch.tensor([1, 2, 0]), 3)
    g._csr = SimpleNamespace(rowptr=None, col=None)
    monkeypatch.setattr(PF, "pyg_row_factors", lambda *a, **k: [None] * 3)
    assert PF.pyg_simple_bf16(simple, g, torch.zeros(3, simple.F_in, dtype=BF)) == "out"
    return seen[0]["post_img"], seen[0]["post_bias"]


def test_simple_images_follow_their_tensors(monkeypatch):
    """Both routes of PNAConvSimple: the one-call image (memo on the module) and the multi-launch image (memo on the weight) are
    rebuilt when post_nn[0].weight or .bias changes in place, and a conversion drops them."""
    simple = _simple(F=5, out=6)
    lin = simple.post_nn[0]
    post, bias = _simple_small_images(simple, monkeypatch)
    assert _simple_small_images(simple, monkeypatch)[0] is post and bias is lin.bias
    assert post.shape == (1, 3, 16, 32)
    W = lin.weight.reshape(6, 3, 4, 5)
    for s in range(3):
        for a in range(4):
            assert torch.equal(post[0, s, :6, a * 8:a * 8 + 5], W[:, s, a]) and torch.count_nonzero(post[0, s, :, a * 8 + 5:a * 8 + 8]) == 0
    for t in (lin.weight, lin.bias):
        before = simple.__dict__["_pna_amd_bf16_small"]
        with torch.no_grad():
            t.add_(1.0)
        after, _ = _simple_small_images(simple, monkeypatch)
        assert simple.__dict__["_pna_amd_bf16_small"] is not before and after is not before[1]["post"], "stale one-call image"
        assert torch.equal(after[0, :, :6].reshape(3, 6, 4, 8)[..., :5], lin.weight.reshape(6, 3, 4, 5).permute(1, 0, 2, 3))
    simple.to(BF)
    assert "_pna_amd_bf16_small" not in simple.__dict__
    img = ops.pack_posttrans_weight_bf16(lin.weight, 3, 4, 5, 8)
    assert ops.pack_posttrans_weight_bf16(lin.weight, 3, 4, 5, 8) is img
    with torch.no_grad():
        lin.weight.add_(1.0)
    assert ops.pack_posttrans_weight_bf16(lin.weight, 3, 4, 5, 8) is not img
    # layout: scaler block s, aggregator a at columns a * 8, padding columns zero
    img = ops.pack_posttrans_weight_bf16(lin.weight, 3, 4, 5, 8)
    W = lin.weight.reshape(6, 3, 4, 5)
    for s in range(3):
        for a in range(4):
            assert torch.equal(img[s, :6, a * 8:a * 8 + 5], W[:, s, a]) and torch.count_nonzero(img[s, :, a * 8 + 5:a * 8 + 8]) == 0


def test_pyg_column_order_lands_in_the_source_and_destination_halves():
    """pre_nns[t][0].weight is [x_i (destination) | x_j (source) | enc]: W_j fills the x_src rows, W_i (with the bias) the x_dst rows --
    the opposite of the DGL order the same builder serves -- in the packed, the padded and the one-call layout."""
    Fi, T = 5, 2
    for pre_layers in (1, 2):
        conv = _conv(in_c=Fi, out_c=6, towers=T, edge_dim=3, pre_layers=pre_layers)
        im = PF._pyg_conv_images_bf16(conv)
        Fs = 8 if pre_layers > 1 else Fi                              # per-tower padded layout for pna_edge_mlp_bf16
        P = im["P"]
        assert P == 16 == (T * Fs + 7) // 8 * 8
        for t in range(T):
            W, b = conv.pre_nns[t][0].weight, conv.pre_nns[t][0].bias
            assert torch.equal(im["proj"][0, t * Fs:t * Fs + Fi, :Fi], W[:, Fi:2 * Fi])             # source half: W_j
            assert torch.equal(im["proj"][0, P + t * Fs:P + t * Fs + Fi, :Fi], W[:, :Fi])           # destination half: W_i
            assert torch.equal(im["proj_bias"][P + t * Fs:P + t * Fs + Fi], b) and torch.count_nonzero(im["proj_bias"][:P]) == 0
            assert torch.equal(im["edge"][0, t * Fs:t * Fs + Fi, :Fi], W[:, 2 * Fi:])
            Wp = conv.post_nns[t][0].weight
            assert torch.equal(im["self"][0, 3 * t:3 * t + 3, :Fi], Wp[:, :Fi])
            for s in range(3):                                        # identity is the first scaler: perm is the identity
                for a in range(4):
                    c = a * P + t * Fs
                    assert torch.equal(im["post"][s, 3 * t:3 * t + 3, c:c + Fi], Wp[:, Fi + (s * 4 + a) * Fi:Fi + (s * 4 + a + 1) * Fi])
                    assert torch.count_nonzero(im["post"][s, 3 * t:3 * t + 3, c + Fi:c + Fs]) == 0  # padding columns meet zero weights
        if pre_layers > 1:
            assert torch.count_nonzero(im["proj"][0, Fi:8]) == 0 and torch.count_nonzero(im["proj"][0, P + Fi:P + 8]) == 0
            assert im["mlp"].shape == (T, 1, 16, 32) and im["mlp_bias"].shape == (T, 1, Fi)
            for t in range(T):
                assert torch.equal(im["mlp"][t, 0, :Fi, :Fi], conv.pre_nns[t][2].weight) and torch.equal(im["mlp_bias"][t, 0], conv.pre_nns[t][2].bias)
            assert int(torch.count_nonzero(im["mlp"])) == int(sum(torch.count_nonzero(conv.pre_nns[t][2].weight) for t in range(T)))
    conv = _conv(in_c=Fi, out_c=6, towers=T, edge_dim=3)
    sm = PF._pyg_conv_small_images_bf16(conv)
    rows = torch.zeros(2 * T * 8, Fi, dtype=BF)
    for t in range(T):
        W = conv.pre_nns[t][0].weight
        rows[t * 8:t * 8 + Fi], rows[(T + t) * 8:(T + t) * 8 + Fi] = W[:, Fi:2 * Fi], W[:, :Fi]
    assert torch.equal(sm["proj"][0, :2 * T * 8, :Fi], rows)
    assert torch.equal(sm["mix"][:6, :6], conv.lin.weight) and sm["mix_bias"] is conv.lin.bias


def test_row_factors_are_cached_per_graph_scaler_and_avg_deg():
    from pna_amd.graph import Graph
    g = Graph(torch.tensor([0, 1, 2, 2]), torch.tensor([1, 2, 0, 1]), 4)           # node 3 has no in-edges
    avg = {"lin": 1.5, "log": 0.9, "exp": 3.0}
    f = PF.pyg_row_factors(g, ["identity", "attenuation", "inverse_linear"], avg)
    assert f[0] is None and f[1][3] == 1.0 and f[2][3] == 1.0 and f[1].dtype == torch.float32
    again = PF.pyg_row_factors(g, ["attenuation", "linear"], avg)
    assert again[0] is f[1]
    assert PF.pyg_row_factors(g, ["attenuation"], dict(avg, log=1.0))[0] is not f[1]
    assert PF._edge_ids(g) is PF._edge_ids(g) and PF._edge_ids(g).tolist() == [0, 1, 2, 3] and PF._edge_ids(g).dtype == torch.int32


def _edge_mlp_args():
    a = _lib.PnaEdgeMlpBf16Args()
    a.E, a.T, a.F, a.n_hidden = 100, 2, 75, 1
    for f in ("col", "row", "x_src", "x_dst", "w_img", "bias", "out"):
        setattr(a, f, ctypes.c_void_p(4096))
    a.ld_src = a.ld_dst = a.ld_out = 160
    return a


def test_edge_mlp_entry_point_refuses_what_it_cannot_run():
    L = _lib.lib()
    fn = L.pna_edge_mlp_bf16
    a = _edge_mlp_args()
    assert a.struct_size == ctypes.sizeof(_lib.PnaEdgeMlpBf16Args)
    for short in (0, ctypes.sizeof(_lib.PnaEdgeMlpBf16Args) - 8):
        a.struct_size = short
        assert fn(ctypes.byref(a), None) == -1 and b"struct_size" in L.pna_last_error()
    a = _edge_mlp_args()
    a.F = 129
    assert fn(ctypes.byref(a), None) == -1 and b"F <= 128" in L.pna_last_error()
    a = _edge_mlp_args()
    a.F, a.n_hidden = 128, 4                                       # the hidden weights of one tower beyond the LDS
    assert fn(ctypes.byref(a), None) == -1 and b"LDS" in L.pna_last_error()
    a = _edge_mlp_args()
    a.bias = None
    assert fn(ctypes.byref(a), None) == -1 and b"bias" in L.pna_last_error()
    a = _edge_mlp_args()
    a.out = ctypes.c_void_p(4096 + 2)                              # not 16-byte aligned
    assert fn(ctypes.byref(a), None) == -1 and b"out" in L.pna_last_error()
    a = _edge_mlp_args()
    a.ld_out = 156                                                 # a pitch that is no multiple of 8 / shorter than T round8(F)
    assert fn(ctypes.byref(a), None) == -1 and b"out" in L.pna_last_error()
    a = _edge_mlp_args()
    a.ld_src = 152
    assert fn(ctypes.byref(a), None) == -1 and b"x_src" in L.pna_last_error()
    a = _edge_mlp_args()
    a.edge_type = ctypes.c_void_p(4096)                            # edge types without a table
    assert fn(ctypes.byref(a), None) == -1 and b"edge_type" in L.pna_last_error()
    a = _edge_mlp_args()
    a.E = 0                                                        # nothing to do: no launch, no pointer is looked at
    a.out = None
    assert fn(ctypes.byref(a), None) == 0


def test_aggregator_codes_of_the_pyg_rules():
    """var_raw (6) and std_pyg (7) are codes of the three bf16 statistics entry points only: they refuse 8, an fp32 entry point 7."""
    L = _lib.lib()
    assert _lib.AGG_CODES["var_raw"] == 6 and _lib.AGG_CODES["std_pyg"] == 7
    assert "var_raw" not in ops._BF16_AGGS and "std_pyg" not in ops._BF16_AGGS          # the DGL predicate's set is what it was
    header = open(os.path.join(ROOT, "include", "pna_amd.h")).read()
    assert re.search(r"PNA_AGG_VAR_RAW = 6,", header) and re.search(r"PNA_AGG_STD_PYG = 7\b", header)
    p = ctypes.c_void_p(4096)

    def gather(cls, code):
        g = cls()
        g.V, g.F, g.n_aggr, g.ldx, g.ldo = 10, 75, 1, 80, 80
        g.rowptr = g.col = g.x = g.out = p
        g.aggr[0] = code
        g.ldo = 75                                                  # (the NEXT refusal, after the codes: nothing is ever launched)
        return g

    for cls, fn in ((_lib.PnaSegreduceBf16Args, L.pna_segreduce_fwd_bf16), (_lib.PnaGatherBf16Args, L.pna_gather_bf16)):
        for code, refused_for_code in ((6, False), (7, False), (8, True), (-1, True)):
            assert fn(ctypes.byref(gather(cls, code)), None) == -1
            assert (b"aggregator code" in L.pna_last_error()) == refused_for_code, (cls.__name__, code, L.pna_last_error())
    for code, refused_for_code in ((6, False), (7, False), (8, True)):
        t = _lib.PnaTowerLayerBf16Args()
        t.V, t.n_tower, t.Fi, t.Fo, t.n_scaler, t.n_aggr, t.mix_slope = 10, 1, 8, 8, 1, 1, 2.0     # (the next refusal: the slope)
        t.aggr[0] = code
        assert L.pna_tower_layer_bf16(ctypes.byref(t), None) == -1
        assert (b"aggregator code" in L.pna_last_error()) == refused_for_code, (code, L.pna_last_error())
    s = _lib.PnaSegreduceArgs()
    s.V, s.F, s.n_tower, s.n_aggr, s.n_scaler = 10, 8, 1, 1, 1
    s.rowptr = s.col = s.x = s.out = p
    s.ldx = s.ldo = s.tower_stride_in = s.tower_stride_out = 8
    for code, ok_code in ((6, True), (7, False)):
        s.aggr[0] = code
        s.ldo = 4                                                   # too short: refused after the codes
        assert L.pna_segreduce_fwd_f32(ctypes.byref(s), None) == -1
        assert (b"unknown aggregator code" in L.pna_last_error()) == (not ok_code), (code, L.pna_last_error())
        assert ok_code == (b"leading dimensions" in L.pna_last_error())
    assert ops._BF16_KERNEL_AGGS == ops._BF16_AGGS + ("var_raw", "std_pyg")


def _compile(src, tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out_s = str(tmp_path / (src + ".s"))
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
           "-S", "--cuda-device-only", "-o", out_s, os.path.join(CSRC, src), "-Rpass-analysis=kernel-resource-usage"]
    err = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    names = re.findall(r"Function Name: (\S+)", err)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", err)]
    vgprs = [int(v) for v in re.findall(r" VGPRs: (\d+)", err)]
    agprs = [int(v) for v in re.findall(r" AGPRs: (\d+)", err)]
    assert names and len(names) == len(scratch) == len(vgprs) == len(agprs)
    return out_s, names, scratch, vgprs, agprs


def test_edge_mlp_kernels_use_no_scratch_and_stay_within_256_registers(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_audit
    out_s, names, scratch, vgprs, agprs = _compile("pna_bf16_edge_mlp.hip", tmp_path)
    for n, v, a, s in zip(names, vgprs, agprs, scratch):
        print(f"{n}: {v} VGPRs + {a} AGPRs, {s} bytes of scratch")
    assert sum("k_edge_mlp_bf16" in n for n in names) == 4 == len(names)                 # 1..4 column chunks of 32
    assert not [n for n, s in zip(names, scratch) if s], "kernels using scratch"
    assert all(v + a <= 256 for v, a in zip(vgprs, agprs))
    text = open(out_s).read()
    assert "v_mfma_f32_16x16x32_bf16" in text and "ds_read_b128" in text
    for n in names:
        kl = isa_audit.kernel_lines(out_s, n)
        assert not isa_audit.sgpr_hazards(kl), n
        assert not isa_audit.pk_src1_hi_selects(kl), n


def test_the_statistics_codes_cost_the_pinned_files_no_instantiation(tmp_path):
    """var_raw and std_pyg are run-time codes: pna_bf16_gather.hip and pna_bf16_small.hip compile to the kernels they had (the
    counts and register caps of test_bf16_host.py, test_bf16_tower_host.py and test_build_resources.py)."""
    _, names, scratch, vgprs, _ = _compile("pna_bf16_gather.hip", tmp_path)
    assert sum("k_gather_bf16" in n for n in names) == 14 == len(names) and not any(scratch)
    # the plain gather: MSG, the LAST template argument of k_gather_bf16 / k_gather_bf16_seg, is false (4 light-row + 2 segment kernels)
    plain = [v for n, v in zip(names, vgprs) if re.search(r"k_gather_bf16(_seg)?I(Lb[01]E)*Lb0EEE", n)]
    assert len(plain) == 6, names
    assert max(plain) <= 96
    assert max(vgprs) <= 168
    _, names, scratch, vgprs, _ = _compile("pna_bf16_small.hip", tmp_path)
    assert sum("k_tower_rows_bf16" in n for n in names) == 6 == len(names) and not any(scratch) and max(vgprs) <= 168
