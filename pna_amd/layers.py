"""Dense blocks the PNA layers and the multitask GNN are assembled from: `FCLayer`, `MLP`, `GRU`, `Set2Set` and `S2SReadout`.

Same constructor arguments, forward order (linear -> activation -> dropout -> batch-norm), weight
initialisation and state_dict keys (`fully_connected.{k}.linear.{weight,bias}`) as the reference's
models/layers.py:101-234, so checkpoints are interchangeable.  These are the plain library GEMMs
of the path (torch.nn.Linear -> rocBLAS/hipBLASLt); the hot contraction after the aggregation goes
through pna_amd.ops.posttrans instead.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

_ACTIVATIONS = {
    "relu": nn.ReLU, "sigmoid": nn.Sigmoid, "tanh": nn.Tanh, "elu": nn.ELU, "selu": nn.SELU, "glu": nn.GLU,
    "leakyrelu": nn.LeakyReLU, "softplus": nn.Softplus,
}


def get_activation(activation):
    """String -> module, case-insensitive; None / 'none' -> None; callables pass through (models/layers.py:8-19)."""
    if activation is None or callable(activation):
        return activation
    key = str(activation).lower()
    if key == "none":
        return None
    assert key in _ACTIVATIONS, 'Unhandled activation function'   # same failure mode as the reference
    return _ACTIVATIONS[key]()


class FCLayer(nn.Module):
    def __init__(self, in_size, out_size, activation="relu", dropout=0., b_norm=False, bias=True, init_fn=None,
                 device="cpu"):
        super().__init__()
        self.in_size, self.out_size, self.bias = in_size, out_size, bias
        self.linear = nn.Linear(in_size, out_size, bias=bias).to(device)
        self.dropout = nn.Dropout(p=dropout) if dropout else None
        self.b_norm = nn.BatchNorm1d(out_size).to(device) if b_norm else None
        self.activation = get_activation(activation)
        self.init_fn = init_fn or nn.init.xavier_uniform_
        self.reset_parameters()

    def reset_parameters(self, init_fn=None):
        (init_fn or self.init_fn)(self.linear.weight, 1 / self.in_size)     # gain = 1/in_size (:170-179)
        if self.bias:
            self.linear.bias.data.zero_()

    def forward(self, x):
        h = self.linear(x)
        if self.activation is not None:
            h = self.activation(h)
        if self.dropout is not None:
            h = self.dropout(h)
        if self.b_norm is not None:
            h = self.b_norm(h.transpose(1, 2)).transpose(1, 2) if h.shape[1] != self.out_size else self.b_norm(h)
        return h

    def __repr__(self):
        return f"{self.__class__.__name__} ({self.in_size} -> {self.out_size})"


class MLP(nn.Module):
    """`layers` FCLayers; a single layer uses `last_activation` (models/layers.py:214-216).  With PNA_AMD_MLP_HEAD_ROWS on and the call
    in scope (`_one_call_path`) all layers run as one C call each way (autograd.mlp_head); otherwise exactly the loop over the FCLayers."""

    def __init__(self, in_size, hidden_size, out_size, layers, mid_activation="relu", last_activation="none",
                 dropout=0., mid_b_norm=False, last_b_norm=False, device="cpu"):
        super().__init__()
        self.in_size, self.hidden_size, self.out_size = in_size, hidden_size, out_size
        sizes = [in_size] + [hidden_size] * (max(layers, 1) - 1) + [out_size]
        self.fully_connected = nn.ModuleList()
        for i in range(len(sizes) - 1):
            last = i == len(sizes) - 2
            self.fully_connected.append(FCLayer(sizes[i], sizes[i + 1],
                                                activation=last_activation if last else mid_activation,
                                                b_norm=last_b_norm if last else mid_b_norm, device=device,
                                                dropout=dropout))

    def _one_call_path(self, x):
        """Whether this MLP is served by pna_mlp_head_fwd_f32 / _bwd_f32 (functional.mlp_head_path on the layers' nn.Linear and
        activation modules; a 3-D contiguous x as its (B N, D) view): additionally no layer has a batch-norm and none a dropout that
        is active in this mode.  The knob PNA_AMD_MLP_HEAD_ROWS at 0 answers before anything is looked at."""
        from . import functional as PF
        if not PF.MLP_HEAD_ROWS > 0:
            return False
        fcs = list(self.fully_connected)
        if any(type(fc) is not FCLayer or fc.b_norm is not None for fc in fcs):
            return False
        if any(fc.dropout is not None and fc.dropout.p > 0 and fc.dropout.training for fc in fcs):
            return False
        return PF.mlp_head_path(x, [fc.linear for fc in fcs], [fc.activation for fc in fcs])

    def forward(self, x):
        if self._one_call_path(x):
            from . import functional as PF
            from .autograd import mlp_head
            fcs = list(self.fully_connected)
            y = mlp_head(x.reshape(-1, x.shape[-1]), [fc.linear for fc in fcs], [PF.mlp_head_act(fc.activation) for fc in fcs])
            return y.reshape(*x.shape[:-1], -1)
        for fc in self.fully_connected:
            x = fc(x)
        return x

    def __repr__(self):
        return f"{self.__class__.__name__} ({self.in_size} -> {self.out_size})"

    # -- helpers for the fused paths -----------------------------------------------------------
    @property
    def is_affine(self):
        """True when the MLP is a single Linear with no activation / dropout / batch-norm, i.e. the
        form a 1-layer pretrans / posttrans takes (last_activation='none')."""
        if len(self.fully_connected) != 1:
            return False
        fc = self.fully_connected[0]
        return fc.activation is None and fc.b_norm is None and (fc.dropout is None or not self.training)

    def tail(self, x):
        """Everything after the first Linear (its activation, dropout, batch-norm and the later layers)."""
        fc = self.fully_connected[0]
        if fc.activation is not None:
            x = fc.activation(x)
        if fc.dropout is not None:
            x = fc.dropout(x)
        if fc.b_norm is not None:
            x = fc.b_norm(x)
        for fc in self.fully_connected[1:]:
            x = fc(x)
        return x


class GRU(nn.Module):
    """models/layers.py:237-268: the multitask GNN's GRU -- nn.GRU over a length-1 sequence on (B, N, Din <= input_size) inputs with
    (B, N, Dh <= hidden_size) hidden rows, the difference zero-padded; (B, N, hidden_size) out.  Same parameter names
    (`gru.weight_ih_l0` .. `gru.bias_hh_l0`).  With PNA_AMD_GRU_ROWS on and the call in scope (nets.gru_one_call_path) the update is one C
    call each way on the (B N, D) views, the padding expressed through the column counts; otherwise exactly the reference's lines."""

    def __init__(self, input_size, hidden_size, device):
        super().__init__()
        self.input_size, self.hidden_size = input_size, hidden_size
        self.gru = nn.GRU(input_size=input_size, hidden_size=hidden_size).to(device)

    def _one_call_path(self, x, y):
        """nets.GRU._one_call_path on the (B N, D) views of 3-D x and y (a reshape that would copy declines)."""
        from . import functional as PF
        if not PF.GRU_ROWS > 0:
            return False
        if not (x.dim() == 3 and y.dim() == 3 and x.shape[:2] == y.shape[:2] and x.is_contiguous() and y.is_contiguous()):
            return False
        from .nets import gru_one_call_path
        return gru_one_call_path(self.gru, x.reshape(x.shape[0] * x.shape[1], -1), y.reshape(y.shape[0] * y.shape[1], -1))

    def forward(self, x, y):
        assert (x.shape[-1] <= self.input_size and y.shape[-1] <= self.hidden_size)
        (B, N, _) = x.shape
        if self._one_call_path(x, y):
            from .autograd import gru_cell
            return gru_cell(x.reshape(B * N, -1), y.reshape(B * N, -1), self.gru).reshape(B, N, -1)
        x = x.reshape(1, B * N, -1).contiguous()
        y = y.reshape(1, B * N, -1).contiguous()
        if x.shape[-1] < self.input_size:
            x = F.pad(input=x, pad=[0, self.input_size - x.shape[-1]], mode='constant', value=0)
        if y.shape[-1] < self.hidden_size:
            y = F.pad(input=y, pad=[0, self.hidden_size - y.shape[-1]], mode='constant', value=0)
        x = self.gru(x, y)[1]
        return x.reshape(B, N, -1)


class Set2Set(nn.Module):
    """models/layers.py:22-98: the Set2Set pooling of (B, N, nin) rows into (B, nhid) -- `steps` (default: N) rounds of a one-step LSTM on
    q*, the scores x . q, a softmax over the nodes and the weighted sum r, with q* = [q | r].  Same constructor, same parameter names
    (`lstm.weight_ih_l0` .. `lstm.bias_hh_l0`).  With PNA_AMD_S2S_ROWS on and the call in scope (`_one_call_path`) the whole loop is one C
    call each way (autograd.set2set); otherwise exactly the reference's loop over `self.lstm`."""

    def __init__(self, nin, nhid=None, steps=None, num_layers=1, activation=None, device='cpu'):
        super().__init__()
        self.steps = steps
        self.nin = nin
        self.nhid = 2 * nin if nhid is None else nhid
        if self.nhid <= self.nin:
            raise ValueError('Set2Set hidden_dim should be larger than input_dim')
        self.lstm_output_dim = self.nhid - self.nin
        self.num_layers = num_layers
        self.lstm = nn.LSTM(self.nhid, self.nin, num_layers=num_layers, batch_first=True).to(device)
        self.softmax = nn.Softmax(dim=1)

    def _one_call_path(self, x):
        """True where the one-call route covers the call: the knob covers B N rows; x a contiguous fp32 (B, N, nin) tensor on a GPU; one
        LSTM layer of input size 2 nin with biases, fp32 on x's device; N, nin and the step count inside the kernel's scope."""
        from . import functional as PF
        if not PF.S2S_ROWS > 0:
            return False
        if not (x.dim() == 3 and x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()):
            return False
        B, N, D = x.shape
        if not (self.num_layers == 1 and D == self.nin and self.nhid == 2 * self.nin and self.lstm.bias and not self.lstm.bidirectional
                and getattr(self.lstm, "proj_size", 0) == 0):
            return False
        ps = (self.lstm.weight_ih_l0, self.lstm.weight_hh_l0, self.lstm.bias_ih_l0, self.lstm.bias_hh_l0)
        if not all(p.is_cuda and p.dtype == torch.float32 and p.device == x.device for p in ps):
            return False
        return B >= 1 and PF.set2set_fits(N, D, self.steps or N) and B * N <= PF.S2S_ROWS

    def forward(self, x):
        if self._one_call_path(x):
            from .autograd import set2set
            return set2set(x, self.lstm, self.steps or x.shape[1])
        batch_size = x.shape[0]
        n = self.steps or x.shape[1]
        h = (x.new_zeros((self.num_layers, batch_size, self.nin)),
             x.new_zeros((self.num_layers, batch_size, self.nin)))
        q_star = x.new_zeros(batch_size, 1, self.nhid)
        for _ in range(n):
            q, h = self.lstm(q_star, h)                              # q: (B, 1, nin)
            e = torch.matmul(x, torch.transpose(q, 1, 2))            # (B, N, 1)
            a = self.softmax(e)
            r = torch.sum(a * x, dim=1, keepdim=True)
            q_star = torch.cat([q, r], dim=-1)
        return torch.squeeze(q_star, dim=1)


class S2SReadout(nn.Module):
    """models/layers.py:271-289: the graph head -- `Set2Set` over all nodes' features, then an MLP with batch-norm between its layers
    (torch's own ops: it works on B rows).  Parameter names `set2set.lstm.*` and `mlp.fully_connected.{k}.*`."""

    def __init__(self, in_size, hidden_size, out_size, fc_layers=3, device='cpu', final_activation='relu'):
        super().__init__()
        self.set2set = Set2Set(in_size, device=device)
        self.mlp = MLP(in_size=2 * in_size, hidden_size=hidden_size, out_size=out_size, layers=fc_layers, mid_activation="relu",
                       last_activation=final_activation, mid_b_norm=True, last_b_norm=False, device=device)

    def forward(self, x):
        return self.mlp(self.set2set(x))
