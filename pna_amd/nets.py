"""Network assembly of the realworld (sparse) benchmarks -- SURVEY.md 8f row N2.

`PNANet` mirrors realworld_benchmark/nets/molecules_graph_regression/pna_net.py:16-96 (same `net_params`
dict, forward signature and state_dict keys): atom/bond embeddings -> L x PNALayer -> per-graph readout ->
MLPReadout.  `PNANetHIV` mirrors nets/HIV_graph_classification/pna_net.py:9-64 with an in-tree stand-in for
ogb's AtomEncoder (a sum of per-feature embeddings; ogb is not available offline).  `PNANetSuperpixels` mirrors
nets/superpixels_graph_classification/pna_net.py:17-104 (CIFAR10 / MNIST: Linear embeddings of float node / edge features,
MLPReadout to n_classes, cross-entropy).

The per-graph readout (`dgl.sum_nodes` / `mean_nodes` / `max_nodes`, pna_net.py:83-90) is the same HIP
segment-reduce kernel as the message passing: segments = batch_num_nodes, messages = the node rows themselves.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import functional as PF
from .dgl.pna_layer import PNALayer, PNASimpleLayer, as_graph
from .graph import Graph


class MLPReadout(nn.Module):
    """nets/mlp_readout_layer.py:14-29: L halving Linear+ReLU layers, then Linear to output_dim."""

    def __init__(self, input_dim, output_dim, L=2):
        super().__init__()
        dims = [input_dim // 2 ** l for l in range(L + 1)]
        self.FC_layers = nn.ModuleList([nn.Linear(dims[l], dims[l + 1], bias=True) for l in range(L)] +
                                       [nn.Linear(dims[L], output_dim, bias=True)])
        self.L = L

    def _one_call_path(self, x):
        """Whether this head is served by pna_mlp_head_fwd_f32 / _bwd_f32 (functional.mlp_head_path: the knob PNA_AMD_MLP_HEAD_ROWS on
        and covering the rows, fp32 rows and plain nn.Linear parameters on one GPU, L + 1 <= 4 layers of widths <= 128).  The knob at
        0 answers before anything is looked at."""
        if not PF.MLP_HEAD_ROWS > 0:
            return False
        return x.dim() == 2 and PF.mlp_head_path(x, list(self.FC_layers), [_RELU] * self.L + [None])

    def forward(self, x):
        if PF.MLP_HEAD_ROWS > 0 and self._one_call_path(x):
            from . import autograd as AG
            return AG.mlp_head(x, list(self.FC_layers), [PF.mlp_head_act(_RELU)] * self.L + [PF.mlp_head_act(None)])
        for l in range(self.L):
            x = F.relu(self.FC_layers[l](x))
        return self.FC_layers[self.L](x)


_RELU = nn.ReLU()           # MLPReadout's F.relu as the activation module the head route's predicate reads


def linear_rows(lin, x):
    """lin(x) for an nn.Linear over rows (the superpixel net's embeddings): a one-layer call without activation of the head route under
    the same knob and predicate, else torch's own."""
    if PF.MLP_HEAD_ROWS > 0 and x.dim() == 2 and PF.mlp_head_path(x, [lin], [None]):
        from . import autograd as AG
        return AG.mlp_head(x, [lin], [PF.mlp_head_act(None)])
    return lin(x)


class GRU(nn.Module):
    """nets/gru.py:5-30: nn.GRU over a length-1 sequence with the previous features as hidden state."""

    def __init__(self, input_size, hidden_size, device):
        super().__init__()
        self.input_size, self.hidden_size = input_size, hidden_size
        self.gru = nn.GRU(input_size=input_size, hidden_size=hidden_size).to(device)

    def _one_call_path(self, x, y):
        """Whether this update is served by pna_gru_cell_fwd_f32 / _bwd_f32 (autograd.GruCellFn: one C call each way, train and eval,
        with and without grad): the knob PNA_AMD_GRU_ROWS is on and covers the rows (2 <= V: one row's `.squeeze()` has another shape),
        x and y are 2-D fp32 on the GPU with unit column stride and a row pitch of at least the width, the nn.GRU is one layer, one
        direction, bias=True, batch_first=False with its four parameters fp32 on that GPU, and the widths fit the call
        (functional.gru_cell_fits).  No float is read."""
        return gru_one_call_path(self.gru, x, y)

    def forward(self, x, y):
        assert x.shape[-1] <= self.input_size and y.shape[-1] <= self.hidden_size
        if PF.GRU_ROWS > 0 and self._one_call_path(x, y):
            from . import autograd as AG
            return AG.gru_cell(x, y, self.gru)
        return self.gru(x.unsqueeze(0), y.unsqueeze(0).contiguous())[1].squeeze()      # (MIOpen refuses a hidden state that is not contiguous)


def gru_one_call_path(gru, x, y):
    """nets.GRU._one_call_path for an nn.GRU and (V, I) / (V, Hc) rows (layers.GRU asks for its (B N, D) views)."""
    if not PF.GRU_ROWS > 0:
        return False
    if not (x.dim() == 2 and y.dim() == 2 and x.shape[0] == y.shape[0] and 2 <= x.shape[0] <= PF.GRU_ROWS):
        return False
    for t in (x, y):
        if not (t.is_cuda and t.dtype == torch.float32 and t.stride(1) == 1 and t.stride(0) >= t.shape[1]):
            return False
    if not (type(gru) is nn.GRU and gru.num_layers == 1 and not gru.bidirectional and gru.bias and not gru.batch_first and
            getattr(gru, "proj_size", 0) == 0 and gru.dropout == 0):
        return False
    for name in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0"):
        p = getattr(gru, name, None)
        if p is None or not (p.is_cuda and p.dtype == torch.float32 and p.device == x.device and p.device == y.device):
            return False
    return PF.gru_cell_fits(x.shape[1], y.shape[1], gru.input_size, gru.hidden_size)


def _readout_path(graph, h):
    """Whether this readout is served by pna_readout_fwd_f32 / _bwd_f32 (autograd.ReadoutFn: one C call each way): the knob
    PNA_AMD_NET_ENDS_ROWS is on and covers the batch, fp32 rows on the GPU inside the call's width, one row per node, and no graph of the
    batch is empty (the call's segments are non-empty node ranges).  No float is read and the device is not waited for."""
    V = h.shape[0]
    if not (PF.NET_ENDS_ROWS > 0 and 0 < V <= PF.NET_ENDS_ROWS):
        return False
    if not (h.is_cuda and h.dtype == torch.float32 and h.dim() == 2 and 1 <= h.shape[1] <= 512):
        return False
    if not (type(graph) is Graph and graph.num_nodes == V):
        return False
    return _readout_offsets(graph, h.device) is not None


def _readout_offsets(graph, dev):
    """int32 [n_graphs + 1] on `dev`: the node range of every graph of the batch (the readout graph's rowptr, without building that
    graph), or None when a graph of the batch is empty or the sizes do not add up to the node count.  From the host-side size list,
    kept with the graph's other derived arrays."""
    key = ("readout_offsets", dev)
    if key not in graph._heavy:
        sizes = torch.tensor([0] + list(graph.batch_num_nodes), dtype=torch.int64)
        ok = sizes.numel() >= 2 and int(sizes[1:].min()) >= 1 and int(sizes.sum()) == graph.num_nodes
        graph._heavy[key] = sizes.cumsum(0).to(torch.int32).to(dev) if ok else None
    return graph._heavy[key]


def readout_nodes(g, h, op):
    """(n_graphs, F): sum / mean / max of the node rows of every graph of the batch -- one segment-reduce launch."""
    graph = as_graph(g)
    if PF.NET_ENDS_ROWS > 0 and _readout_path(graph, h):
        # a molecule batch: the graphs are contiguous node ranges, one C call each way (autograd.ReadoutFn)
        from . import autograd as AG
        return AG.readout(h, _readout_offsets(graph, h.device), op)
    key = ("readout", h.device)
    rg = graph._heavy.get(key)
    if rg is None:
        sizes = torch.tensor(graph.batch_num_nodes, dtype=torch.long, device=h.device)
        owner = torch.repeat_interleave(torch.arange(sizes.numel(), device=h.device), sizes)
        rg = Graph(torch.arange(graph.num_nodes, device=h.device), owner, sizes.numel())   # node v -> its graph
        graph._heavy[key] = rg
    if h.dtype == torch.bfloat16:
        # bf16 rows (the bf16 inference path of the layers): fp32 statistics rounded once, pna_segreduce_fwd_bf16
        if h.stride(-1) != 1:
            h = h.contiguous()
        csr = rg.csr
        return PF.ops.segreduce_bf16(csr.rowptr, csr.col, h, h.shape[1], [op], heavy=rg.heavy_schedule(), workspace=rg.workspace)
    return PF.aggregate(rg, h, h.shape[1], [op], edge_resident=True)


class PNANet(PF.DropsCachesOnConversion, nn.Module):
    def __init__(self, net_params):
        super().__init__()
        p = net_params
        hidden_dim, out_dim, n_layers = p["hidden_dim"], p["out_dim"], p["L"]
        self.readout = p["readout"]
        self.edge_feat = p["edge_feat"]
        self.gru_enable = p["gru"]
        self.in_feat_dropout = nn.Dropout(p["in_feat_dropout"])
        self.embedding_h = nn.Embedding(p["num_atom_type"], hidden_dim)
        if self.edge_feat:
            self.embedding_e = nn.Embedding(p["num_bond_type"], p["edge_dim"])
        common = dict(dropout=p["dropout"], graph_norm=p["graph_norm"], batch_norm=p["batch_norm"], residual=p["residual"],
                      aggregators=p["aggregators"], scalers=p["scalers"], avg_d=p["avg_d"], towers=p["towers"],
                      edge_features=self.edge_feat, edge_dim=p["edge_dim"], pretrans_layers=p["pretrans_layers"],
                      posttrans_layers=p["posttrans_layers"])
        self.layers = nn.ModuleList([PNALayer(in_dim=hidden_dim, out_dim=hidden_dim, divide_input=p["divide_input_first"],
                                              **common) for _ in range(n_layers - 1)])
        self.layers.append(PNALayer(in_dim=hidden_dim, out_dim=out_dim, divide_input=p["divide_input_last"], **common))
        if self.gru_enable:
            self.gru = GRU(hidden_dim, hidden_dim, p["device"])
        self.MLP_layer = MLPReadout(out_dim, 1)

    def forward(self, g, h, e, snorm_n, snorm_e=None):
        graph = as_graph(g)
        h = self.in_feat_dropout(embed(self.embedding_h, h) if isinstance(self.embedding_h, nn.Embedding) else self.embedding_h(h))
        if self.edge_feat:
            e_idx = e
            e = embed(self.embedding_e, e)
            if e_idx.dim() == 1 and not torch.is_floating_point(e_idx) and hasattr(graph, "register_edge_types"):
                # the layers' edge-type fast paths (<= 4 bond types: ZINC) get the types they would otherwise have to FIND in e's rows
                graph.register_edge_types(e, e_idx, self.embedding_e.weight)
        for i, conv in enumerate(self.layers):
            h_t = conv(graph, h, e, snorm_n)
            if self.gru_enable and i != len(self.layers) - 1:
                h_t = self.gru(h, h_t)
            h = h_t
        hg = readout_nodes(graph, h, self.readout if self.readout in ("sum", "max", "mean") else "mean")
        return self.MLP_layer(hg)

    def loss(self, scores, targets):
        return nn.L1Loss()(scores, targets)


class PNANetSuperpixels(PF.DropsCachesOnConversion, nn.Module):
    """nets/superpixels_graph_classification/pna_net.py:17-104: the same stack as the molecules net behind LINEAR embeddings of the
    float node features (mean colour | position: in_dim 3 for MNIST, 5 for CIFAR10) and edge features, `n_classes` outputs and a
    cross-entropy loss.  (Like the reference's forward :72-98, `in_feat_dropout` is read from the params and never applied.)
    Same `net_params` keys, forward signature and state_dict keys."""

    def __init__(self, net_params):
        super().__init__()
        p = net_params
        hidden_dim, out_dim, n_layers = p["hidden_dim"], p["out_dim"], p["L"]
        self.readout = p["readout"]
        self.edge_feat = p["edge_feat"]
        self.gru_enable = p["gru"]
        self.embedding_h = nn.Linear(p["in_dim"], hidden_dim)
        if self.edge_feat:
            self.embedding_e = nn.Linear(p["in_dim_edge"], p["edge_dim"])
        common = dict(dropout=p["dropout"], graph_norm=p["graph_norm"], batch_norm=p["batch_norm"], residual=p["residual"],
                      aggregators=p["aggregators"], scalers=p["scalers"], avg_d=p["avg_d"], towers=p["towers"],
                      edge_features=self.edge_feat, edge_dim=p["edge_dim"], pretrans_layers=p["pretrans_layers"],
                      posttrans_layers=p["posttrans_layers"])
        self.layers = nn.ModuleList([PNALayer(in_dim=hidden_dim, out_dim=hidden_dim, divide_input=p["divide_input_first"],
                                              **common) for _ in range(n_layers - 1)])
        self.layers.append(PNALayer(in_dim=hidden_dim, out_dim=out_dim, divide_input=p["divide_input_last"], **common))
        if self.gru_enable:
            self.gru = GRU(hidden_dim, hidden_dim, p["device"])
        self.MLP_layer = MLPReadout(out_dim, p["n_classes"])

    def forward(self, g, h, e, snorm_n, snorm_e=None):
        graph = as_graph(g)
        h = linear_rows(self.embedding_h, h)
        if self.edge_feat:
            e = linear_rows(self.embedding_e, e)
        for i, conv in enumerate(self.layers):
            h_t = conv(graph, h, e, snorm_n)
            if self.gru_enable and i != len(self.layers) - 1:
                h_t = self.gru(h, h_t)
            h = h_t
        hg = readout_nodes(graph, h, self.readout if self.readout in ("sum", "max", "mean") else "mean")
        return self.MLP_layer(hg)

    def loss(self, pred, label):
        return nn.CrossEntropyLoss()(pred, label)


class _SmallTableEmbedding(torch.autograd.Function):
    """weight[idx] whose backward is a one-hot GEMM, grad_w = onehot(idx)^T @ grad.  torch's embedding backward sorts the
    indices and runs a segmented scatter (0.4 ms per table for 52 k atoms -- with the nine tables of the atom encoder
    that was 44 % of a MolHIV training step) and `index_add_` into a table of 2..119 rows is one long chain of
    contended atomics (0.3 ms per table); the GEMM is ~0.03 ms."""

    @staticmethod
    def forward(ctx, weight, idx):
        ctx.save_for_backward(idx)
        ctx.rows = weight.shape[0]
        return weight.index_select(0, idx)

    @staticmethod
    def backward(ctx, grad):
        (idx,) = ctx.saved_tensors
        if ctx.rows <= 1024:
            gw = F.one_hot(idx, ctx.rows).to(grad.dtype).t() @ grad
        else:
            gw = torch.zeros(ctx.rows, grad.shape[1], dtype=grad.dtype, device=grad.device).index_add_(0, idx, grad.contiguous())
        return gw, None


def _embed_sum_path(embs, idx):
    """Whether sum_j embs[j](idx[:, j]) is served by pna_embed_sum_fwd_f32 / _bwd_f32 (autograd.EmbedSumFn: one C call each way, train
    or eval, with or without grad): the knob PNA_AMD_NET_ENDS_ROWS is on and covers the rows, the index is int64 on the GPU with one
    column per table (1-D for a single table), every table is a plain fp32 nn.Embedding on the same GPU (no padding_idx, no max_norm)
    of one width, and the tables fit the call's scope (functional.embed_sum_fits).  Indices are not looked at: the calls clamp them."""
    V = idx.shape[0] if idx.dim() >= 1 else 0
    if not (PF.NET_ENDS_ROWS > 0 and 0 < V <= PF.NET_ENDS_ROWS):
        return False
    if not (idx.dtype == torch.int64 and idx.is_cuda):
        return False
    if not ((idx.dim() == 1 and len(embs) == 1) or (idx.dim() == 2 and idx.shape[1] == len(embs))):
        return False
    if any(type(e) is not nn.Embedding or e.padding_idx is not None or e.max_norm is not None for e in embs):
        return False
    ws = [e.weight for e in embs]
    if any(w.dtype != torch.float32 or w.device != idx.device or w.shape[1] != ws[0].shape[1] for w in ws):
        return False
    return PF.embed_sum_fits([w.shape[0] for w in ws], ws[0].shape[1])


def embed(emb: nn.Embedding, idx):
    """emb(idx) for the small categorical vocabularies of the molecule nets (same values, faster backward)."""
    if emb.padding_idx is not None or emb.max_norm is not None or idx.dim() != 1:
        return emb(idx)
    if PF.NET_ENDS_ROWS > 0 and _embed_sum_path([emb], idx):
        from . import autograd as AG
        return AG.embed_sum(idx, [emb.weight])
    return _SmallTableEmbedding.apply(emb.weight, idx)


class AtomEncoderStandIn(nn.Module):
    """Sum of one embedding per categorical atom feature -- what ogb.graphproppred.mol_encoder.AtomEncoder computes
    (ogb 1.2.2 is pinned by the reference but not installable offline; dims are the OGB molecule vocabulary sizes)."""
    DIMS = (119, 4, 12, 12, 10, 6, 6, 2, 2)

    def __init__(self, emb_dim, dims=DIMS):
        super().__init__()
        self.atom_embedding_list = nn.ModuleList(nn.Embedding(d, emb_dim) for d in dims)
        for emb in self.atom_embedding_list:
            nn.init.xavier_uniform_(emb.weight.data)

    def forward(self, x):
        if PF.NET_ENDS_ROWS > 0 and _embed_sum_path(list(self.atom_embedding_list), x):
            # a molecule batch: the nine lookups and their sum as one C call, the nine table gradients as another (autograd.EmbedSumFn)
            from . import autograd as AG
            return AG.embed_sum(x, [emb.weight for emb in self.atom_embedding_list])
        out = 0
        for i, emb in enumerate(self.atom_embedding_list):
            out = out + embed(emb, x[:, i])
        return out


class PNANetHIV(PF.DropsCachesOnConversion, nn.Module):
    """nets/HIV_graph_classification/pna_net.py:9-64 (PNASimpleLayer stack, mean readout by default)."""

    def __init__(self, net_params):
        super().__init__()
        p = net_params
        hidden_dim, out_dim, n_layers = p["hidden_dim"], p["out_dim"], p["L"]
        self.readout = p["readout"]
        self.in_feat_dropout = nn.Dropout(p["in_feat_dropout"])
        self.embedding_h = AtomEncoderStandIn(emb_dim=hidden_dim)
        common = dict(dropout=p["dropout"], batch_norm=p["batch_norm"], residual=p["residual"], aggregators=p["aggregators"],
                      scalers=p["scalers"], avg_d=p["avg_d"], posttrans_layers=p["posttrans_layers"])
        self.layers = nn.ModuleList([PNASimpleLayer(in_dim=hidden_dim, out_dim=hidden_dim, **common)
                                     for _ in range(n_layers - 1)])
        self.layers.append(PNASimpleLayer(in_dim=hidden_dim, out_dim=out_dim, **common))
        self.MLP_layer = MLPReadout(out_dim, 1)

    def forward(self, g, h):
        graph = as_graph(g)
        h = self.in_feat_dropout(embed(self.embedding_h, h) if isinstance(self.embedding_h, nn.Embedding) else self.embedding_h(h))
        for conv in self.layers:
            h = conv(graph, h)
        hg = readout_nodes(graph, h, self.readout if self.readout in ("sum", "max", "mean") else "mean")
        return self.MLP_layer(hg)

    def loss(self, scores, labels):
        return nn.BCEWithLogitsLoss()(scores, labels.float().to(scores.device).unsqueeze(-1))
