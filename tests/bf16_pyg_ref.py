"""Float64 host models of the bf16 PyG front end (PNAConv, PNAConvSimple), shared by the bf16 PyG tests (no tests in here).

Arithmetic contract (u = 2^-8, R = round to bf16 once, everything between roundings fp32):
  P0   enc = R(W_enc e + b_enc)
  P1   x_dst = R(W_i x_t + b), x_src = R(W_j x_t), x_edge = R(W_e enc)      columns of pre_nns[t][0].weight: [x_i | x_j | enc]
       pre_layers = 1: the message (x_src[j] + x_dst[i]) + x_edge stays in fp32
  P1h  pre_layers = L >= 2: z_1 = R(relu(message)), z_l = R(relu(W_l z_(l-1) + b_l)), m = R(W_L z_(L-1) + b_L)
  P2   aggregates with fp32 statistics, each R; var is not clamped; a row without in-edges gives 0, its std R(sqrtf(1e-5f))
  P3   h_cat = R(b_t + W_h x_t + sum_s f_s(v) (W_s z));  PNAConvSimple has no W_h term;  a deeper post_nn: the module's own bf16
       ops, modelled as one rounding per Linear
  P4   out = R(W_lin h_cat + b_lin)                                          PNAConv only

`layer_models` evaluates ref64 (no rounding), emu (R at P0-P4 only) and the bound E that `2u |value| + 4u mass` per rounding gives when
it is propagated through the later stages, with the rules of bf16_tower_ref (linear stage: |W| err; mean / sum / max / min / std / var:
aggregate_error; ReLU 1-Lipschitz).  The mass of an aggregate is bf16_tower_ref.aggregate_mass plus the fp32 floor phi (stat_floor)."""
import numpy as np
import torch

import bf16_tower_ref as B

U = B.U
EMPTY_STD = float(np.sqrt(np.float32(1e-5)))            # sqrtf(1e-5f)
FALSIFICATIONS = ("halves_swapped", "empty_std_dropped", "attenuation_zero_rule_dropped", "lin_bias_dropped")


def factor64(name, deg, avg_deg, zero_rule=True):
    """The PyG scalers (models/pytorch_geometric/scalers.py) per row in float64; zero_rule=False drops `deg == 0 -> 1`."""
    D = np.asarray(deg, dtype=np.float64)
    with np.errstate(divide="ignore"):
        if name == "identity":
            f = np.ones_like(D)
        elif name == "amplification":
            f = np.log(D + 1) / avg_deg["log"]
        elif name == "attenuation":
            f = np.where(D > 0, avg_deg["log"] / np.log(D + 1), 1.0 if zero_rule else 0.0)
        elif name == "linear":
            f = D / avg_deg["lin"]
        elif name == "inverse_linear":
            f = np.where(D > 0, avg_deg["lin"] / np.maximum(D, 1), 1.0 if zero_rule else 0.0)
        else:
            raise KeyError(name)
    return torch.from_numpy(f)[:, None]


class _Rows:
    """Per-row float64 reductions of per-edge messages (edge order) by destination, as torch scatter reductions.  The formulas built
    on them are those of bf16_tower_ref (aggregate64, aggregate_mass, stat_floor, aggregate_error: DESIGN.md 4.11); its reductions
    go through the oracle's degree buckets, which take 20 s at E = 100 003."""

    def __init__(self, dst, N):
        self.dst = torch.as_tensor(dst).long().cpu()
        self.deg = torch.bincount(self.dst, minlength=N).numpy()
        self.N, self.nz = N, self.deg > 0
        self.w = self.deg.astype(np.float64)[:, None]

    def reduce(self, how, m):
        m = torch.as_tensor(m, dtype=torch.float64)
        out = torch.zeros(self.N, m.shape[1], dtype=torch.float64)
        if how == "sum":
            out.index_add_(0, self.dst, m)
        else:
            out.scatter_reduce_(0, self.dst[:, None].expand_as(m), m, how, include_self=False)    # rows without in-edges stay 0
        return out.numpy()

    def mean(self, m):
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(self.nz[:, None], self.reduce("sum", m) / self.w, 0.0)


def _parts(msg, dst, N):
    r = _Rows(dst, N)
    m = msg.numpy()
    mean, msq = r.mean(m), r.mean(m * m)
    var = msq - mean * mean
    std = np.where(r.nz[:, None], np.sqrt(np.maximum(var, 0) + 1e-5), 0.0)
    return r, m, mean, msq, var, std


def aggregate64(msg, src, dst, N, aggs, empty_std=EMPTY_STD):
    """(N, A F) float64 PyG aggregates of per-edge messages (edge order): var = E[m^2] - E[m]^2 without a clamp, rows without in-edges
    are 0, their std `empty_std`."""
    r, m, mean, msq, var, std = _parts(msg, dst, N)
    by = {"sum": lambda: r.reduce("sum", m), "mean": lambda: mean, "max": lambda: r.reduce("amax", m), "min": lambda: r.reduce("amin", m),
          "var": lambda: var, "std": lambda: np.where(r.nz[:, None], std, empty_std)}
    return torch.from_numpy(np.concatenate([by[a]() for a in aggs], axis=1))


def aggregate_bound(msg, src, dst, N, aggs):
    """What ONE rounding of fp32 statistics may cost per aggregate: 2u |z| + 4u (M + phi).  M, the absolute mass: the
    aggregate's formula over absolute terms (mean |m|, sum |m|, E[m^2] + E[m]^2 for var, its root for std, |max|, |min|); phi, the
    floor of fp32 accumulation: C sum |m|, C mean |m|, f = C (E[m^2] + 2 E[|m|]^2) for var, f / (2 std) for std, C = 2e-6."""
    r, m, mean, msq, var, std = _parts(msg, dst, N)
    z = aggregate64(msg, src, dst, N, aggs)
    m1, mabs = r.reduce("sum", np.abs(m)), r.mean(np.abs(m))
    var_mass = msq + mean * mean
    mass = {"sum": m1, "mean": mabs, "var": var_mass, "std": np.where(r.nz[:, None], np.sqrt(var_mass + 1e-5), 0.0),
            "max": np.abs(r.reduce("amax", m)), "min": np.abs(r.reduce("amin", m))}
    f_var = B.C_EPS * (msq + 2 * mabs * mabs)
    floor = {"sum": B.C_EPS * m1, "mean": B.C_EPS * mabs, "var": f_var, "std": f_var / (2 * np.maximum(std, np.sqrt(1e-5))),
             "max": 0 * m1, "min": 0 * m1}
    M = torch.from_numpy(np.concatenate([mass[a] + floor[a] for a in aggs], axis=1))
    return 2 * U * z.abs() + 4 * U * M


def aggregate_error(err, msg, src, dst, N, aggs):
    """Bound on the change of every aggregate when edge message k moves by at most err[k]: the mean / sum / largest edge error for
    mean / sum / max and min, rms(err) for std (|std(m + d) - std(m)| <= rms(d)), 2 std rms + rms^2 for var."""
    r, m, mean, msq, var, std = _parts(msg, dst, N)
    e = err.numpy()
    rms = np.sqrt(r.mean(e * e))
    mx = r.reduce("amax", e)
    by = {"mean": r.mean(e), "sum": r.reduce("sum", e), "max": mx, "min": mx, "std": rms, "var": 2 * std * rms + rms * rms}
    return torch.from_numpy(np.concatenate([by[a] for a in aggs], axis=1))


def _linear(sd, key):
    return sd[key + ".weight"], sd[key + ".bias"]


def _tail(sd, prefix, n, y, y_r, e_y):
    """Linear layers 1.. of an MLP `prefix`.{0,2,..} after its first one: ReLU then Linear, one rounding per Linear in the emulation."""
    for l in range(1, n):
        W, b = _linear(sd, f"{prefix}.{2 * l}")
        a, a_r = torch.relu(y), torch.relu(y_r)
        y, y_r = a @ W.T + b, B.rbf(a_r @ W.T + b)
        e_y = e_y @ W.abs().T + 2 * U * y.abs() + 4 * U * (a.abs() @ W.abs().T + b.abs())
    return y, y_r, e_y


def layer_models(kind, sd, meta, edge_index, N, x, edge_attr, avg_deg, falsify=None):
    """-> (ref64, emu, E) of one PNAConv (kind "pyg_conv") or PNAConvSimple ("pyg_simple") on float64 values.  sd: the state_dict in
    float64; meta: the fixture's meta; falsify: one of FALSIFICATIONS (changes the emulation only: the tests' own teeth)."""
    assert falsify is None or falsify in FALSIFICATIONS
    src, dst = edge_index[0].long().cpu(), edge_index[1].long().cpu()
    aggs, scalers = meta["aggregators"], meta["scalers"]
    A, S = len(aggs), len(scalers)
    deg = torch.bincount(dst, minlength=N).numpy()
    sc = [factor64(s, deg, avg_deg) for s in scalers]
    sc_r = [factor64(s, deg, avg_deg, zero_rule=falsify != "attenuation_zero_rule_dropped") for s in scalers]
    std_r = 0.0 if falsify == "empty_std_dropped" else EMPTY_STD

    def post(prefix, n_post, ht, Fi, z, z_r, e_z, self_term):
        Wp, bp = _linear(sd, prefix + ".0")
        if self_term:
            Wh, Wz = Wp[:, :Fi], Wp[:, Fi:].reshape(-1, S, A * Fi)
            y = ht @ Wh.T + bp
            mass = ht.abs() @ Wh.abs().T + bp.abs()
        else:
            Wz = Wp.reshape(-1, S, A * Fi)
            y = bp.expand(N, -1).clone()
            mass = bp.abs().expand(N, -1).clone()
        y_r, e_y = y.clone(), torch.zeros_like(y)
        for s in range(S):
            y, y_r = y + sc[s] * (z @ Wz[:, s].T), y_r + sc_r[s] * (z_r @ Wz[:, s].T)
            e_y = e_y + sc[s].abs() * (e_z @ Wz[:, s].abs().T)
            mass = mass + sc[s].abs() * (z.abs() @ Wz[:, s].abs().T)
        return _tail(sd, prefix, n_post, y, B.rbf(y_r), e_y + 2 * U * y.abs() + 4 * U * mass)

    if kind == "pyg_simple":
        F = meta["F"]
        msg = x[src]
        z, z_r = aggregate64(msg, src, dst, N, aggs), B.rbf(aggregate64(msg, src, dst, N, aggs, std_r))
        e_z = aggregate_bound(msg, src, dst, N, aggs)
        return post("post_nn", meta["post_layers"], None, F, z, z_r, e_z, False)

    T, L = meta["towers"], meta["pre_layers"]
    Fi = meta["in_c"] // T if meta["divide_input"] else meta["in_c"]
    use_edge = bool(meta["edge_dim"])
    if use_edge:
        We_, be_ = _linear(sd, "edge_encoder")
        enc = edge_attr @ We_.T + be_
        enc_r = B.rbf(enc)
        e_enc = 2 * U * enc.abs() + 4 * U * (edge_attr.abs() @ We_.abs().T + be_.abs())
    ref_c, emu_c, err_c = [], [], []
    for t in range(T):
        ht = x[:, t * Fi:(t + 1) * Fi] if meta["divide_input"] else x
        W, b = _linear(sd, f"pre_nns.{t}.0")
        Wi, Wj, We = W[:, :Fi], W[:, Fi:2 * Fi], W[:, 2 * Fi:]
        xd, xs = ht @ Wi.T + b, ht @ Wj.T
        e_d = 2 * U * xd.abs() + 4 * U * (ht.abs() @ Wi.abs().T + b.abs())
        e_s = 2 * U * xs.abs() + 4 * U * (ht.abs() @ Wj.abs().T)
        msg, e_m, mass_m = xs[src] + xd[dst], e_s[src] + e_d[dst], xs[src].abs() + xd[dst].abs()
        if falsify == "halves_swapped":
            msg_r = B.rbf(ht @ Wi.T)[src] + B.rbf(ht @ Wj.T + b)[dst]
        else:
            msg_r = B.rbf(xs)[src] + B.rbf(xd)[dst]
        if use_edge:
            xe = enc @ We.T
            msg, msg_r = msg + xe, msg_r + B.rbf(enc_r @ We.T)
            e_m = e_m + e_enc @ We.abs().T + 2 * U * xe.abs() + 4 * U * (enc.abs() @ We.abs().T)
            mass_m = mass_m + xe.abs()
        if L > 1:
            zl, zl_r = torch.relu(msg), B.rbf(torch.relu(msg_r))
            e_m = e_m + 2 * U * zl.abs() + 4 * U * mass_m
            for l in range(1, L):
                Wl, bl = _linear(sd, f"pre_nns.{t}.{2 * l}")
                m_, m_r = zl @ Wl.T + bl, B.rbf(zl_r @ Wl.T + bl)
                e_m = e_m @ Wl.abs().T + 2 * U * m_.abs() + 4 * U * (zl.abs() @ Wl.abs().T + bl.abs())
                if l < L - 1:
                    m_, m_r = torch.relu(m_), torch.relu(m_r)
                zl, zl_r = m_, m_r
            msg, msg_r = zl, zl_r
        z, z_r = aggregate64(msg, src, dst, N, aggs), B.rbf(aggregate64(msg_r, src, dst, N, aggs, std_r))
        e_z = aggregate_error(e_m, msg, src, dst, N, aggs) + aggregate_bound(msg, src, dst, N, aggs)
        y, y_r, e_y = post(f"post_nns.{t}", meta["post_layers"], ht, Fi, z, z_r, e_z, True)
        ref_c.append(y)
        emu_c.append(y_r)
        err_c.append(e_y)
    ref, emu, err = torch.cat(ref_c, 1), torch.cat(emu_c, 1), torch.cat(err_c, 1)
    Wm, bm = _linear(sd, "lin")
    out, out_r = ref @ Wm.T + bm, emu @ Wm.T + (0.0 if falsify == "lin_bias_dropped" else bm)
    return out, B.rbf(out_r), err @ Wm.abs().T + 2 * U * out.abs() + 4 * U * (ref.abs() @ Wm.abs().T + bm.abs())


def edge_mlp_models(xs, xd, er, col, row, etype, W, b):
    """pna_edge_mlp_bf16 for ONE tower in float64: xs / xd (nodes, F), er (rows, F) or None, etype (E,) row of every edge or None (edge k
    reads row k), W / b: the hidden layers [(F, F)], [(F)].  -> (ref64 from the EXACT z_1, bound).  z_1 = R(relu((xs + xd) + er)) in
    float32 in the kernel's order is known bit for bit; the bound of the last layer is 2u |ref| + 4u (|W| |z| + |b|), a hidden
    layer's bound propagated through |W| of the next (ReLU 1-Lipschitz)."""
    m = xs.float()[col] + xd.float()[row]
    if er is not None:
        m = m + (er.float()[etype] if etype is not None else er.float())
    z = torch.relu(m).to(torch.bfloat16).double()
    err = torch.zeros_like(z)
    for l, (Wl, bl) in enumerate(zip(W, b)):
        y = z @ Wl.T + bl
        err = err @ Wl.abs().T + 2 * U * y.abs() + 4 * U * (z.abs() @ Wl.abs().T + bl.abs())
        z = torch.relu(y) if l < len(W) - 1 else y
    return z, err
