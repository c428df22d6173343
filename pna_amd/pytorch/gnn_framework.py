"""The multitask benchmark's network (models/pytorch/gnn_framework.py:8-108): a stack of graph convolutions on a dense adjacency, an
optional GRU shared by all of them, and two heads -- an MLP per node and a Set2Set readout per graph.  Same constructor arguments,
assertions, attribute names (`conv_layers`, `gru`, `nodes_read_out`, `graph_read_out`) and forward as the reference, so its checkpoints load
with strict=True.  The pieces are this package's: a `layer_type` such as pna_amd.pytorch.pna.layer.PNALayer, layers.GRU, layers.MLP and
layers.S2SReadout, each with its one-call route behind its own knob (PNA_AMD_DENSE_LAYER_ROWS, PNA_AMD_GRU_ROWS, PNA_AMD_MLP_HEAD_ROWS,
PNA_AMD_S2S_ROWS).
Nothing in the forward reads a float from the device, so an eval forward can be captured (capture.GraphedForward)."""
import types

import torch
import torch.nn as nn
import torch.nn.functional as F

from ..layers import GRU, MLP, S2SReadout


def _namespace(descr, what):
    """A convolution's description as a SimpleNamespace with a SimpleNamespace of arguments (either may arrive as a dict)."""
    if type(descr) == dict:
        descr = types.SimpleNamespace(**descr)
    assert type(descr) == types.SimpleNamespace, f"{what} should be dict or SimpleNamespace"
    if type(descr.args) == dict:
        descr.args = types.SimpleNamespace(**descr.args)
    assert type(descr.args) == types.SimpleNamespace, f"{what}.args should be either a dict or a SimpleNamespace"
    return descr


class GNN(nn.Module):
    """nfeat -> nhid through `conv_layers` convolutions -> (nodes_out per node, graph_out per graph).

    conv_layers: an int, or with `variable` a function adj -> int; `fixed` reuses ONE middle convolution for every layer after the first
    (required by `variable`, excluded by `skip`); `skip` feeds the input and every layer's output to the heads; `gru` updates the features
    with a shared GRU after each convolution; dropout follows every layer but the last.  first_conv_descr / middle_conv_descr: `layer_type`
    and `args`; in_features, out_features and device are filled in here."""

    def __init__(self, nfeat, nhid, nodes_out, graph_out, dropout, conv_layers=2, fc_layers=3, first_conv_descr=None,
                 middle_conv_descr=None, final_activation='LeakyReLU', skip=False, gru=False, fixed=False, variable=False, device='cpu'):
        super().__init__()
        if variable:
            assert callable(conv_layers), "conv_layers should be a function from adjacency matrix to int"
            assert fixed, "With a variable number of layers they must be fixed"
            assert not skip, "cannot have skip and fixed at the same time"
        else:
            assert type(conv_layers) == int, "conv_layers should be an int"
            assert conv_layers > 0, "conv_layers should be greater than 0"
        first_conv_descr = _namespace(first_conv_descr, "first_conv_descr")
        middle_conv_descr = _namespace(middle_conv_descr, "middle_conv_descr")

        self.dropout = dropout
        self.skip, self.fixed, self.variable = skip, fixed, variable
        self.n_fixed_conv = conv_layers
        self.conv_layers = nn.ModuleList()                           # (registered first: parameters() in the reference's order)
        self.gru = GRU(input_size=nhid, hidden_size=nhid, device=device) if gru else None

        first_conv_descr.args.in_features, first_conv_descr.args.out_features, first_conv_descr.args.device = nfeat, nhid, device
        self.conv_layers.append(first_conv_descr.layer_type(**vars(first_conv_descr.args)))
        middle_conv_descr.args.in_features, middle_conv_descr.args.out_features, middle_conv_descr.args.device = nhid, nhid, device
        for _ in range(1 if fixed else conv_layers - 1):
            self.conv_layers.append(middle_conv_descr.layer_type(**vars(middle_conv_descr.args)))

        n_conv_out = nfeat + conv_layers * nhid if skip else nhid
        self.nodes_read_out = MLP(in_size=n_conv_out, hidden_size=n_conv_out, out_size=nodes_out, layers=fc_layers,
                                  mid_activation="LeakyReLU", last_activation=final_activation, device=device)
        self.graph_read_out = S2SReadout(n_conv_out, n_conv_out, graph_out, fc_layers=fc_layers, device=device,
                                         final_activation=final_activation)

    def forward(self, x, adj):
        n_layers = self.n_fixed_conv(adj) if self.variable else self.n_fixed_conv
        convs = [self.conv_layers[0]] + [self.conv_layers[1]] * (n_layers - 1) if self.fixed else self.conv_layers
        kept = [x] if self.skip else None
        for k, conv in enumerate(convs):
            y = conv(x, adj)
            x = y if self.gru is None else self.gru(x, y)
            if self.skip:
                kept.append(x)
            if k != n_layers - 1:                                    # dropout on all layers but the last
                x = F.dropout(x, self.dropout, training=self.training)
        if self.skip:
            x = torch.cat(kept, dim=2)
        return self.nodes_read_out(x), self.graph_read_out(x)
