"""Float64 host models of the bf16 tower path, shared by the bf16 tower tests (no tests in here).

Arithmetic contract (one PNALayer call, bf16 inputs and parameters, u = 2^-8, R = round to bf16 once):
  R1  x_src = R(W_a h_t), x_dst = R(W_b h_t + b), x_edge = R(W_e ef)
      m(u->v) = x_src[u] + x_dst[v] + x_edge          fp32, never rounded
  R2  aggregates of m with fp32 statistics, each R
  R3  h_cat = R(BN(snorm_n * (W_h h_t + sum_s scale_s (W_s z) + b)))
  R4  out = R(h + leaky(W_mix h_cat + b_mix))

`layer_models` evaluates, from the exact bf16 values, ref64 (no rounding), emu (R at R1-R4 only, everything else float64) and the
bound E that `2u |value| + 4u mass` per rounding gives when it is propagated through the later stages:
  linear stage     err_out = |W| err_in (+ row / column factors), mass = |W| |in| + |b|
  mean / sum       the mean / sum of the edge errors;  max / min: the largest edge error of the row
  std              sqrt(mean err^2)   (|std(m + d) - std(m)| <= rms(d));   var: 2 std rms(err) + mean err^2
  LeakyReLU        1-Lipschitz
R2's mass includes phi, the floor of fp32 statistics of tests/test_gpu_bf16_simple_layer.py (same formulas)."""
import numpy as np
import torch

from conftest import mass_stats
from oracle import torch_oracle as O

U = 2.0 ** -8
C_EPS = 2e-6           # conftest.check_blocks


def f64(t):
    return t.detach().float().cpu().double()


def rbf(x):
    """fp64 -> fp32 -> bf16 (nearest even) -> fp64: the kernels' single rounding of an fp32 result."""
    return x.float().to(torch.bfloat16).double()


def scale64(name, D, avg_log):
    D = np.asarray(D, dtype=np.float64)
    with np.errstate(divide="ignore"):
        if name == "identity":
            return np.ones_like(D)
        if name == "amplification":
            return np.log(D + 1) / avg_log
        return np.where(D > 0, avg_log / np.log(D + 1), 0.0)


def csr(src, dst, N):
    src = torch.as_tensor(src).long().cpu()
    dst = torch.as_tensor(dst).long().cpu()
    rp, order, deg = O.csr_by_dst(src, dst, N)
    return src, dst, rp, order, deg


def aggregate64(msg, src, dst, N, aggs):
    """(N, A F) float64 aggregates of per-edge messages (edge order), identity scaler; zero in-degree rows are 0."""
    return O.reduce_bucketed(msg, src, dst, N, list(aggs), ["identity"], torch.tensor(1.0, dtype=torch.float64))


def stat_floor(msg, src, dst, N, aggs):
    """phi (N, A F): what fp32 accumulation of the statistics may cost, per aggregate (0 for max / min)."""
    src, dst, rp, order, deg = csr(src, dst, N)
    m = msg[order].numpy()
    rpn = rp.numpy()
    m1, m2, w = mass_stats(rpn, m)
    s1 = np.zeros_like(m1)
    nz = rpn[1:] > rpn[:-1]
    if len(m):
        s1[nz] = np.add.reduceat(m, rpn[:-1][nz], axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        mean_abs = m1 / w
        f_var = C_EPS * (m2 / w + 2 * mean_abs * mean_abs)
        std64 = np.sqrt(np.maximum(m2 / w - (s1 / w) ** 2, 0) + 1e-5)
        floors = {"sum": C_EPS * m1, "mean": C_EPS * mean_abs, "var": f_var, "std": f_var / (2 * np.maximum(std64, np.sqrt(1e-5))),
                  "max": np.zeros_like(m1), "min": np.zeros_like(m1)}
    floors = {k: np.nan_to_num(v, nan=0.0, posinf=0.0) for k, v in floors.items()}
    return torch.from_numpy(np.concatenate([floors[a] for a in aggs], axis=1))


def aggregate_mass(msg, src, dst, N, aggs):
    """(N, A F): the absolute mass of every aggregate -- its formula with every term replaced by its absolute value: mean |m| for
    the mean, sum |m| for the sum, E[m^2] + E[m]^2 for var = E[m^2] - E[m]^2 and the square root of that (+ 1e-5) for std; max and
    min select one message and have their own absolute value.  It is what a rounding error relative to the TERMS of a statistic
    scales with: an fp32 var of two nearly equal messages of size 1.5 is off by an ulp of 2.4, whatever the var itself is."""
    src, dst, rp, order, deg = csr(src, dst, N)
    m = msg[order].numpy()
    rpn = rp.numpy()
    m1, m2, w = mass_stats(rpn, m)
    s1 = np.zeros_like(m1)
    nz = rpn[1:] > rpn[:-1]
    if len(m):
        s1[nz] = np.add.reduceat(m, rpn[:-1][nz], axis=0)
    z = aggregate64(msg, src, dst, N, ["max", "min"]).numpy()
    F = msg.shape[1]
    with np.errstate(divide="ignore", invalid="ignore"):
        var_mass = np.nan_to_num(m2 / w + (s1 / w) ** 2, nan=0.0, posinf=0.0)
        by = {"sum": m1, "mean": np.nan_to_num(m1 / w, nan=0.0, posinf=0.0), "var": var_mass,
              "std": np.where(nz[:, None], np.sqrt(var_mass + 1e-5), 0.0), "max": np.abs(z[:, :F]), "min": np.abs(z[:, F:])}
    return torch.from_numpy(np.concatenate([by[a] for a in aggs], axis=1))


def aggregate_error(err, msg, src, dst, N, aggs):
    """Bound on the change of every aggregate when edge message k moves by at most err[k] (see the module docstring)."""
    one = torch.tensor(1.0, dtype=torch.float64)
    mean_e, max_e, sum_e = (O.reduce_bucketed(err, src, dst, N, [a], ["identity"], one) for a in ("mean", "max", "sum"))
    rms = torch.sqrt(O.reduce_bucketed(err * err, src, dst, N, ["mean"], ["identity"], one))
    std = O.reduce_bucketed(msg, src, dst, N, ["std"], ["identity"], one)
    by = {"mean": mean_e, "sum": sum_e, "max": max_e, "min": max_e, "std": rms, "var": 2 * std * rms + rms * rms}
    return torch.cat([by[a] for a in aggs], dim=1)


def layer_models(sd, cfg, src, dst, N, h, e, snorm_n, avg_log, stop_after_towers=False, drop_dst_term=False, dst_gain=1.0):
    """-> (ref64, emu, E) of one PNALayer (or, stop_after_towers, of its concatenated towers) on float64 copies of the exact bf16
    values.  cfg: towers, divide_input, aggregators, scalers (lists), graph_norm, batch_norm, residual, edge_features.
    drop_dst_term / dst_gain falsify the emulation (the tests' own teeth): the destination term dropped or scaled."""
    src = torch.as_tensor(src).long().cpu()
    dst = torch.as_tensor(dst).long().cpu()
    T, aggs, scalers = cfg["towers"], cfg["aggregators"], cfg["scalers"]
    A, S = len(aggs), len(scalers)
    in_dim = h.shape[1]
    Fi = in_dim // T if cfg["divide_input"] else in_dim
    deg = torch.bincount(dst, minlength=N).numpy()
    sc = [torch.from_numpy(scale64(s, deg, avg_log))[:, None] for s in scalers]
    sn = snorm_n.reshape(-1, 1) if cfg["graph_norm"] else torch.ones(N, 1, dtype=torch.float64)
    ref_c, emu_c, err_c = [], [], []
    for t in range(T):
        ht = h[:, t * Fi:(t + 1) * Fi] if cfg["divide_input"] else h
        W, b = sd[f"towers.{t}.pretrans.fully_connected.0.linear.weight"], sd[f"towers.{t}.pretrans.fully_connected.0.linear.bias"]
        Wa, Wb, We = W[:, :Fi], W[:, Fi:2 * Fi], W[:, 2 * Fi:]
        xs, xd = ht @ Wa.T, ht @ Wb.T + b
        e_s = 2 * U * xs.abs() + 4 * U * (ht.abs() @ Wa.abs().T)
        e_d = 2 * U * xd.abs() + 4 * U * (ht.abs() @ Wb.abs().T + b.abs())
        msg, msg_r, e_m = xs[src] + xd[dst], rbf(xs)[src] + (0.0 if drop_dst_term else dst_gain) * rbf(xd)[dst], e_s[src] + e_d[dst]
        if cfg["edge_features"]:
            xe = e @ We.T
            msg, msg_r = msg + xe, msg_r + rbf(xe)
            e_m = e_m + 2 * U * xe.abs() + 4 * U * (e.abs() @ We.abs().T)
        z, z_r = aggregate64(msg, src, dst, N, aggs), rbf(aggregate64(msg_r, src, dst, N, aggs))
        e_z = aggregate_error(e_m, msg, src, dst, N, aggs) + 2 * U * z.abs() + 4 * U * (z.abs() + stat_floor(msg, src, dst, N, aggs))
        Wp, bp = sd[f"towers.{t}.posttrans.fully_connected.0.linear.weight"], sd[f"towers.{t}.posttrans.fully_connected.0.linear.bias"]
        Wh, Wz = Wp[:, :Fi], Wp[:, Fi:].reshape(-1, S, A * Fi)
        y, y_r = ht @ Wh.T + bp, ht @ Wh.T + bp
        e_y, mass = torch.zeros_like(y), ht.abs() @ Wh.abs().T + bp.abs()
        for s in range(S):
            y, y_r = y + sc[s] * (z @ Wz[:, s].T), y_r + sc[s] * (z_r @ Wz[:, s].T)
            e_y = e_y + sc[s].abs() * (e_z @ Wz[:, s].abs().T)
            mass = mass + sc[s].abs() * (z.abs() @ Wz[:, s].abs().T)
        y, y_r, e_y, mass = y * sn, y_r * sn, e_y * sn, mass * sn
        if cfg["batch_norm"]:
            p = f"towers.{t}.batchnorm_h"
            cs = sd[f"{p}.weight"] / torch.sqrt(sd[f"{p}.running_var"] + 1e-5)
            ct = sd[f"{p}.bias"] - sd[f"{p}.running_mean"] * cs
            y, y_r, e_y, mass = y * cs + ct, y_r * cs + ct, e_y * cs.abs(), mass * cs.abs() + ct.abs()
        ref_c.append(y)
        emu_c.append(rbf(y_r))
        err_c.append(e_y + 2 * U * y.abs() + 4 * U * mass)
    ref, emu, err = torch.cat(ref_c, 1), torch.cat(emu_c, 1), torch.cat(err_c, 1)
    if stop_after_towers:
        return ref, emu, err
    Wm, bm = sd["mixing_network.linear.weight"], sd["mixing_network.linear.bias"]
    lk = torch.nn.functional.leaky_relu
    out, out_r = lk(ref @ Wm.T + bm, 0.01), lk(emu @ Wm.T + bm, 0.01)
    e_o, mass = err @ Wm.abs().T, ref.abs() @ Wm.abs().T + bm.abs()
    if cfg["residual"] and in_dim == out.shape[1]:
        out, out_r, mass = out + h, out_r + h, mass + h.abs()
    return out, rbf(out_r), e_o + 2 * U * out.abs() + 4 * U * mass


def rho(x, ref, E):
    """max_j |x_j - ref_j| / E_j over every element."""
    return float(((x - ref).abs() / E).max())
