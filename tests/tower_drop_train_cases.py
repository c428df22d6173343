"""Shared inputs, references and the host restatement of the mask rule for the one-call PNALayer training tests WITH DROPOUT
(test_tower_drop_train_host.py, test_gpu_tower_drop_train_kernels.py, test_gpu_tower_drop_train_layers.py): pna_tower_drop_train_fwd_f32 /
_bwd_f32 and pna_dropout_mask_f32 against

* a numpy restatement of Philox4x32-10 and of the mask rule of include/pna_amd.h (known answers: the Random123 vectors), and
* the float64 oracle WITH A MASK, restated here from oracle.torch_oracle's public pieces: tower_forward per tower (train mode), times the
  mask, then the mixing Linear, LeakyReLU and the residual (models/dgl/pna_layer.py:71-75, 134-144).

The inputs, the ill-conditioned lists and the bars (check_step, close, check_grad_e) are those of tower_train_cases /
tower_edge_train_cases, unchanged: the lists depend on what lies in front of the BatchNorms, which the mask does not touch, so their
caps (at most 15 % of the nodes) hold as those modules assert them.  What the mask does change is which mixing pre-activations lie near
zero: a case asserts that none lies within 1e-5 of the largest UNDER ITS MASK.  The dropout keys below were picked on the CPU so that
this holds and the fp32 oracle under the same mask passes the bars on its own (test_tower_drop_train_host.py runs exactly that).
Every reference is computed once per session and never modified."""
import functools
import types

import numpy as np
import torch
import torch.nn.functional as Fnn

import tower_edge_train_cases as TE
import tower_train_cases as TT
from oracle import torch_oracle as O
from tower_train_cases import AGGS, SLOPE, check_step, close, post_w, pre_w  # noqa: F401  (re-exported to the tests)
from tower_edge_train_cases import check_grad_e  # noqa: F401

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF

# (counter, key, output): Random123's known answers for philox4x32-10
KNOWN_ANSWERS = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((MASK32,) * 4, (MASK32,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]

#        name: (base cases module, p, seed, offset) -- the kernel tests' cases
CASES = {
    "tower_train_t4_div": (TT, 0.3, 1237, 0),
    "zinc_first": (TT, 0.1, 7, 4096),
    "zinc_edge_first": (TE, 0.3, (5 << 32) | 13, (1 << 33) + 8),
}


def philox4x32_10(counter, key):
    """counter: 4 arrays (or ints) of 32-bit words, key: 2 -> the 4 output words as uint64 arrays holding 32-bit values."""
    c = [np.asarray(x, dtype=np.uint64) & np.uint64(MASK32) for x in counter]
    k0, k1 = (int(k) & MASK32 for k in key)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]                       # 32 x 32 -> 64 bits: no overflow in uint64
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & np.uint64(MASK32), p1 >> np.uint64(32), p1 & np.uint64(MASK32)
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return c


def thr_of(p):
    """(uint32) min(floor((double)(float) p 2^32), 2^32 - 1)."""
    return min(int(np.floor(float(np.float32(p)) * 4294967296.0)), MASK32)


def scale_of(p):
    """1.0f / (1.0f - p), every step in fp32."""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def host_words(n, seed, offset, first=0):
    """The random words of elements first .. first + n - 1: word e & 3 of philox(counter = (lo(e >> 2), hi(e >> 2), lo(offset), hi(offset)),
    key = (lo(seed), hi(seed)))."""
    e = np.arange(first, first + n, dtype=np.uint64)
    q = e >> np.uint64(2)
    w = philox4x32_10((q & np.uint64(MASK32), q >> np.uint64(32), np.full(n, offset & MASK32, np.uint64), np.full(n, (offset >> 32) & MASK32, np.uint64)),
                      (seed & MASK32, (seed >> 32) & MASK32))
    return np.stack(w, axis=1)[np.arange(n), (e & np.uint64(3)).astype(np.int64)]


def host_mask(V, C, p, seed, offset):
    """(V, C) float32: 0 at a dropped element, 1 / (1 - p) at a kept one (kept iff word >= thr)."""
    keep = host_words(V * C, seed, offset) >= np.uint64(thr_of(p))
    return np.where(keep, scale_of(p), np.float32(0.0)).astype(np.float32).reshape(V, C)


def masked_layer_forward(sd, src, dst, N, h, e, snorm_n, scalers, avg_log, towers, divide_input, edge_features, residual, mask, running=None):
    """PNALayer.forward in TRAIN mode with the towers' dropout as a given mask of factors (V, towers Fo): oracle.tower_forward per tower
    (graph norm, batch-statistics BatchNorm; `running` receives the running statistics), times the mask (models/dgl/pna_layer.py:75),
    cat, the mixing Linear + LeakyReLU (:141), the residual (:143-144)."""
    running = {} if running is None else running
    in_dim = h.shape[1]
    it = in_dim // towers if divide_input else in_dim
    outs = [O.tower_forward(sd, f"towers.{t}", src, dst, N, h[:, t * it:(t + 1) * it] if divide_input else h, e, snorm_n, AGGS, scalers, avg_log,
                            True, True, edge_features, running=running) for t in range(towers)]
    h_cat = torch.cat(outs, dim=1) * mask
    out = Fnn.leaky_relu(Fnn.linear(h_cat, sd["mixing_network.linear.weight"], sd["mixing_network.linear.bias"]), SLOPE)
    return h + out if (residual and in_dim == out.shape[1]) else out


def masked_step(sd, a, meta, dtype, mask):
    """One training step under `mask` in `dtype` and the gradients of (out * R).sum() -> (out, grad_h, grad_e or None, {parameter:
    gradient}, {running statistic: value after the step})."""
    cast = lambda t: t.to(dtype) if t.is_floating_point() else t   # noqa: E731
    edge = meta["edge_dim"] > 0
    params = {k: cast(v).clone().requires_grad_(True) for k, v in sd.items() if v.is_floating_point() and "running" not in k}
    live = {k: cast(v) for k, v in sd.items()}
    live.update(params)
    h = cast(a["h"]).clone().requires_grad_(True)
    e = cast(a["e"]).clone().requires_grad_(True) if edge else cast(a["e"])
    running = {}
    out = masked_layer_forward(live, a["src"], a["dst"], meta["N"], h, e, cast(a["snorm_n"]), meta["scalers"].split(), cast(a["avg_log"]), meta["towers"],
                               meta["divide_input"], edge, meta["residual"], mask.to(dtype), running)
    (out * cast(a["R"])).sum().backward()
    grads = {k: (torch.zeros_like(v) if v.grad is None else v.grad) for k, v in params.items()}
    ge = (torch.zeros_like(e) if e.grad is None else e.grad) if edge else None
    return out.detach(), h.grad, ge, grads, running


def pmin_of(out64, a, meta):
    """Smallest |p| / largest |p| of the float64 mixing pre-activation behind `out64`."""
    y = out64 - a["h"].double() if (meta["residual"] and meta["in_dim"] == meta["out_dim"]) else out64
    p = torch.where(y > 0, y, y / SLOPE)
    return (p.abs().min() / p.abs().max()).item()


@functools.lru_cache(maxsize=None)
def case(name, p=None, seed=None, offset=None):
    """-> (meta, arrays, state_dict, ref, key): the base case's inputs; ref = the float64 step under the mask of key = (p, seed, offset)
    (CASES[name]'s unless given) in the shape tower_train_cases.check_step reads, + grad_e, the fp32 step under the same mask (ref32: the
    bars' own-error term) and the mask."""
    base, p0, seed0, offset0 = CASES[name]
    p, seed, offset = (p0 if p is None else p), (seed0 if seed is None else seed), (offset0 if offset is None else offset)
    meta, a, sd, bref = base.case(name)
    mask = torch.from_numpy(host_mask(meta["N"], meta["out_dim"], p, seed, offset))
    out64, gh64, ge64, gp64, run64 = masked_step(sd, a, meta, torch.float64, mask)
    o32, gh32, ge32, gp32, run32 = masked_step(sd, a, meta, torch.float32, mask)
    pmin = pmin_of(out64, a, meta)
    assert pmin >= 1e-5, (name, p, seed, offset, pmin)
    ref = types.SimpleNamespace(out=out64, grad_h=gh64, grad_e=ge64, grads=gp64, running=run64, mask=mask, ill=bref.ill, touched=bref.touched,
                                touched_edges=getattr(bref, "touched_edges", None), z=bref.z, mass=bref.mass, mean=bref.mean, invstd=bref.invstd,
                                ref32=dict(out=o32, grad_h=gh32, grad_e=ge32, grads=gp32, running=run32))
    return meta, a, sd, ref, (p, seed, offset)


# ---- the two-layer PNANetSuperpixels of the layer tests (realworld_benchmark/README.md:65-100: hidden = out of the towers' layers, 5 towers,
# divide_input_first True, divide_input_last True) ---------------------------------------------------------------------------------------
NET_SEED = 3


def net_params(dropout, edge_feat, avg_log):
    return dict(in_dim=5, in_dim_edge=1, hidden_dim=60, out_dim=60, n_classes=10, L=2, readout="sum", edge_feat=edge_feat, edge_dim=50 if edge_feat else 0,
                gru=False, dropout=dropout, in_feat_dropout=0.0, graph_norm=True, batch_norm=True, residual=True, aggregators="mean max min std",
                scalers="identity amplification attenuation", avg_d={"log": avg_log}, towers=5, divide_input_first=True, divide_input_last=True,
                pretrans_layers=1, posttrans_layers=1, device="cpu")


@functools.lru_cache(maxsize=None)
def net_batch(seed=NET_SEED):
    """Four graphs of 20 to 30 nodes, every node with 8 in-edges from 8 distinct other nodes of its graph; 5 node features, 1 edge
    feature, labels."""
    gen = torch.Generator().manual_seed(seed)
    sizes = [int(s) for s in torch.randint(20, 31, (4,), generator=gen)]
    src, dst, o = [], [], 0
    for n in sizes:
        for v in range(n):
            others = torch.tensor([u for u in range(n) if u != v])
            src += [int(o + u) for u in others[torch.randperm(n - 1, generator=gen)[:8]]]
            dst += [o + v] * 8
        o += n
    src, dst = torch.tensor(src), torch.tensor(dst)
    order = torch.randperm(src.numel(), generator=gen)
    src, dst = src[order].contiguous(), dst[order].contiguous()
    V = sum(sizes)
    x = torch.randn(V, 5, generator=gen)
    ef = torch.rand(src.numel(), 1, generator=gen)
    snorm = torch.cat([torch.full((n, 1), float(n) ** -0.5) for n in sizes])
    labels = torch.randint(0, 10, (4,), generator=gen)
    avg_log = torch.log(torch.bincount(dst, minlength=V).double() + 1).mean().float()
    return dict(sizes=sizes, src=src, dst=dst, x=x, e=ef, snorm_n=snorm, labels=labels, avg_log=avg_log, N=V)


def net_masked_loss(sd, params, b, masks, dtype):
    """PNANetSuperpixels in TRAIN mode under one mask per layer -> (loss, live state dict with .grad after backward, the layers' inputs):
    nets/superpixels_graph_classification/pna_net.py:72-98 -- Linear embeddings, L x PNALayer (masked_layer_forward), the sum readout,
    MLPReadout, cross-entropy."""
    live = {k: (v.to(dtype).clone().requires_grad_("running" not in k) if v.is_floating_point() else v) for k, v in sd.items()}
    h = Fnn.linear(b["x"].to(dtype), live["embedding_h.weight"], live["embedding_h.bias"])
    ef = Fnn.linear(b["e"].to(dtype), live["embedding_e.weight"], live["embedding_e.bias"]) if params["edge_feat"] else torch.zeros(b["src"].numel(), 0, dtype=dtype)
    xs, scalers = [], params["scalers"].split()
    for i in range(params["L"]):
        lsd = {k[len(f"layers.{i}."):]: v for k, v in live.items() if k.startswith(f"layers.{i}.")}
        xs.append((h.detach(), ef.detach()))
        h = masked_layer_forward(lsd, b["src"], b["dst"], b["N"], h, ef, b["snorm_n"].to(dtype), scalers, b["avg_log"].to(dtype), params["towers"], True,
                                 params["edge_feat"], True, masks[i].to(dtype))
    y = torch.stack([p.sum(0) for p in torch.split(h, b["sizes"])])                      # readout="sum"
    k = 0
    while f"MLP_layer.FC_layers.{k + 1}.weight" in live:
        y = torch.relu(Fnn.linear(y, live[f"MLP_layer.FC_layers.{k}.weight"], live[f"MLP_layer.FC_layers.{k}.bias"]))
        k += 1
    y = Fnn.linear(y, live[f"MLP_layer.FC_layers.{k}.weight"], live[f"MLP_layer.FC_layers.{k}.bias"])
    loss = Fnn.cross_entropy(y, b["labels"])
    loss.backward()
    return loss.detach(), live, xs


#        name: (dropout, edge_feat, the seed torch.manual_seed gets before the step: the masks' key, offset 0)
NETS = {"cifar_p01": (0.1, False, 11), "cifar_edge_p03": (0.3, True, 15)}


def net_model(name):
    """The two-layer PNANetSuperpixels of NETS[name] on the CPU, in train mode, initialised under NET_SEED."""
    from pna_amd.nets import PNANetSuperpixels
    dropout, edge_feat, _ = NETS[name]
    b = net_batch()
    keep = torch.random.get_rng_state()
    torch.manual_seed(NET_SEED)
    net = PNANetSuperpixels(net_params(dropout, edge_feat, b["avg_log"])).train()
    torch.random.set_rng_state(keep)
    return net


def net_masks(name, seed, offset):
    """The layers' masks under the key rule of functional.tower_dropout_key: one key per layer call, in call order, the offset moved by
    4 ceil(V C / 4) each."""
    p = NETS[name][0]
    b, params = net_batch(), net_params(NETS[name][0], NETS[name][1], 1.0)
    masks = []
    for _ in range(params["L"]):
        masks.append(torch.from_numpy(host_mask(b["N"], params["out_dim"], p, seed, offset)))
        offset += 4 * ((b["N"] * params["out_dim"] + 3) // 4)
    return masks


@functools.lru_cache(maxsize=None)
def net_reference(name):
    """-> namespace: the float64 and fp32 training steps of NETS[name] under the masks of key (p, seed = NETS[name][2], offset 0) (loss, the
    live state dicts with gradients), the ill-conditioned destinations of either layer, the smallest |p| / largest |p| over the layers."""
    dropout, edge_feat, seed = NETS[name]
    b = net_batch()
    params = net_params(dropout, edge_feat, b["avg_log"])
    sd = {k: v.detach().clone() for k, v in net_model(name).state_dict().items()}
    masks = net_masks(name, seed, 0)
    loss64, live64, xs64 = net_masked_loss(sd, params, b, masks, torch.float64)
    loss32, live32, _ = net_masked_loss(sd, params, b, masks, torch.float32)
    base = TE if edge_feat else TT
    ill, pmin = torch.zeros(b["N"], dtype=torch.bool), 1.0
    for i, (x, ef) in enumerate(xs64):
        lsd = {k[len(f"layers.{i}."):]: v.detach() for k, v in live64.items() if k.startswith(f"layers.{i}.")}
        meta = dict(N=b["N"], towers=params["towers"], divide_input=True, in_dim=x.shape[1], out_dim=params["out_dim"], residual=True)
        ill |= base.ill_conditioned(meta, dict(src=b["src"], dst=b["dst"], h=x, e=ef), lsd)[0]
        with torch.no_grad():
            y = masked_layer_forward(lsd, b["src"], b["dst"], b["N"], x, ef, b["snorm_n"].double(), params["scalers"].split(), b["avg_log"].double(),
                                     params["towers"], True, edge_feat, True, masks[i].double())
        pmin = min(pmin, pmin_of(y, dict(h=x), meta))
    return types.SimpleNamespace(loss=loss64, live=live64, loss32=loss32, live32=live32, ill=ill, pmin=pmin, masks=masks, params=params, seed=seed)
