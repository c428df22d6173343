"""Cases, float64 references and DERIVED error bars of the GRU cell calls (pna_gru_cell_fwd_f32 / _bwd_f32): torch.nn.GRU with one layer,
one direction, bias, over a length-1 sequence, gate order r, z, n, with the reference's zero padding of missing x / h columns
(models/layers.py:260-264).  The references are written without autograd (tests/test_gru_host.py checks them against float64 autograd
through torch.nn.GRU).  Everything here runs on the host.

The bars are per element, derived and not measured; no element is excluded (the functions are smooth: no ties, no ReLU flips).
  * dot products: a K-term fp32 dot product, in any order, with fused or separate product roundings, is within gamma(K) mass of the exact
    one, gamma(K) = K u / (1 - K u), u = 2^-24, mass = sum |a| |b|  (`dot_gamma`);
  * gates: an argument error e moves sigmoid by at most e / 4 and tanh by at most e (sigmoid' <= 1/4, tanh' <= 1);
  * products of inexact factors: prod (|a_i| + E_i) - prod |a_i|  (`_prod_err`: every cross term is in it);
  * elementwise allowances: the fp32 operations of each expression counted at their documented bounds -- +, -, *, / correctly rounded
    (u relative each), expf / expm1f / tanhf 1 ulp (2 u relative) -- the count stands next to each constant;
  * results near the subnormal range: TINY = 2^-149 absolute per operation."""
import math

import torch

U = 2.0 ** -24                  # unit roundoff of fp32
TINY = 2.0 ** -149              # the spacing of fp32 subnormals
SLAB = 64                       # _lib.PNA_GRU_SLAB_ROWS (tests/test_gru_host.py pins the two together)
MAX_SLABS = 64
# sigmoid as e / (1 + e) or 1 / (1 + e), e = exp(-|a|): exp 2u; 1 + e: u and at most 2u carried from e; the division u  -> 6u relative
SIG_OPS = 6
# tanh as -m / (m + 2), m = expm1(-2 |a|): expm1 2u (numerator); m + 2: u and at most 2u carried from m (|m| <= 1 <= m + 2); the
# division u -> 6u relative (a library tanhf: 2u)
TANH_OPS = 6
EW_TINY = 8 * TINY              # at most 8 operations between two stored values of any expression below


def dot_gamma(K):
    return K * U / (1.0 - K * U)


def _prod_err(*factors):
    """Error bound of a product of inexact factors given as (magnitude, error bound) pairs: prod (|a| + E) - prod |a|."""
    hi, lo = 1.0, 1.0
    for a, e in factors:
        hi = hi * (a + e)
        lo = lo * a
    return hi - lo


def _pad(t, width):
    return t if t.shape[1] == width else torch.cat([t, t.new_zeros(t.shape[0], width - t.shape[1])], dim=1)


# ---- references ---------------------------------------------------------------------------------------------------------------------
def gru_ref64(x, h, w_ih, w_hh, b_ih, b_hh):
    """-> dict of float64 tensors: out, the saved state r, z, n, gh_n, and the pre-activations a_r, a_z, gi_n."""
    H = w_hh.shape[1]
    x64, h64 = _pad(x.double(), w_ih.shape[1]), _pad(h.double(), H)
    gi = x64 @ w_ih.double().t() + b_ih.double()
    gh = h64 @ w_hh.double().t() + b_hh.double()
    a_r, a_z = gi[:, :H] + gh[:, :H], gi[:, H:2 * H] + gh[:, H:2 * H]
    gi_n, gh_n = gi[:, 2 * H:], gh[:, 2 * H:]
    r, z = torch.sigmoid(a_r), torch.sigmoid(a_z)
    n = torch.tanh(gi_n + r * gh_n)
    return {"out": (1 - z) * n + z * h64, "r": r, "z": z, "n": n, "gh_n": gh_n, "a_r": a_r, "a_z": a_z, "gi_n": gi_n, "x": x64, "h": h64}


def gru_grad_ref64(x, h, w_ih, w_hh, b_ih, b_hh, go):
    """-> (forward dict, dict of the six float64 gradients of sum(out * go) and dgi / dgh); grad_x / grad_h have x's / h's own widths."""
    f = gru_ref64(x, h, w_ih, w_hh, b_ih, b_hh)
    g64, r, z, n, gh_n = go.double(), f["r"], f["z"], f["n"], f["gh_n"]
    d_n = g64 * (1 - z) * (1 - n * n)
    d_z = g64 * (f["h"] - n) * z * (1 - z)
    d_r = d_n * gh_n * r * (1 - r)
    dgi = torch.cat([d_r, d_z, d_n], dim=1)
    dgh = torch.cat([d_r, d_z, d_n * r], dim=1)
    gx = dgi @ w_ih.double()
    gh = dgh @ w_hh.double() + g64 * z
    grads = {"x": gx[:, :x.shape[1]], "h": gh[:, :h.shape[1]], "w_ih": dgi.t() @ f["x"], "w_hh": dgh.t() @ f["h"],
             "b_ih": dgi.sum(0), "b_hh": dgh.sum(0), "dgi": dgi, "dgh": dgh}
    return f, grads


# ---- bars ---------------------------------------------------------------------------------------------------------------------------
def gru_bars(x, h, w_ih, w_hh, b_ih, b_hh, go=None):
    """Per-element bars (float64 tensors) of an fp32 evaluation against gru_ref64 / gru_grad_ref64: keys out, r, z, n, gh_n, and with
    `go` the six gradients x, h, w_ih, w_hh, b_ih, b_hh.  See the module docstring for the rules."""
    H, I, Hc, V = w_hh.shape[1], x.shape[1], h.shape[1], x.shape[0]
    f = gru_ref64(x, h, w_ih, w_hh, b_ih, b_hh)
    ax, ah = f["x"].abs(), f["h"].abs()
    mi = ax @ w_ih.double().abs().t()                        # (V, 3H) masses of x W_ih^T
    mh = ah @ w_hh.double().abs().t()
    bi, bh = b_ih.double().abs(), b_hh.double().abs()
    # pre-activations: a_r, a_z are sums of I + Hc products and two biases in some order; gi_n of I products and one bias; gh_n of Hc and one
    E_ar = dot_gamma(I + Hc + 2) * (mi[:, :H] + mh[:, :H] + bi[:H] + bh[:H])
    E_az = dot_gamma(I + Hc + 2) * (mi[:, H:2 * H] + mh[:, H:2 * H] + bi[H:2 * H] + bh[H:2 * H])
    E_gin = dot_gamma(I + 1) * (mi[:, 2 * H:] + bi[2 * H:])
    E_ghn = dot_gamma(Hc + 1) * (mh[:, 2 * H:] + bh[2 * H:])
    r, z, n, ghn = f["r"], f["z"], f["n"], f["gh_n"]
    E_r = E_ar / 4 + SIG_OPS * U * r + EW_TINY
    E_z = E_az / 4 + SIG_OPS * U * z + EW_TINY
    # the argument of tanh: gi_n + r gh_n -- the product of two inexact factors, its rounding (1), the addition's rounding (1)
    an = f["gi_n"] + r * ghn
    E_an = E_gin + _prod_err((r, E_r), (ghn.abs(), E_ghn)) + U * ((r + E_r) * (ghn.abs() + E_ghn) + an.abs() + E_gin) + EW_TINY
    E_n = E_an + TANH_OPS * U * n.abs() + EW_TINY
    # out = (1 - z) n + z h (1 - z: 1; two products: 2; the sum: 1) or n + z (h - n) (h - n: 1, the product: 1, the sum: 1): the
    # allowance below dominates both -- 2 (1 - z) |n| + 2 z (|h| + |n|) + |out|
    hh, fz = f["h"], 1 - z
    E_out = (_prod_err((fz, E_z), (n.abs(), E_n)) + ah * E_z
             + U * (2 * (fz + E_z) * (n.abs() + E_n) + 2 * (z + E_z) * (ah + n.abs() + E_n) + f["out"].abs()) + EW_TINY)
    bars = {"out": E_out, "r": E_r, "z": E_z, "n": E_n, "gh_n": E_ghn + EW_TINY}
    if go is None:
        return bars
    _, g = gru_grad_ref64(x, h, w_ih, w_hh, b_ih, b_hh, go)
    ag = go.double().abs()
    # gf = go (1 - z): as go * (1 - z) (1 - z: 1, the product: 1) or go - go z (the product: 1 on |go| z, the difference: 1): u |go| (z + 2 (1 - z))
    gf = ag * fz
    E_gf = ag * E_z + U * ag * (z + E_z + 2 * (fz + E_z)) + EW_TINY
    # t = 1 - n^2: as (1 - n)(1 + n) (3 operations on t) or 1 - n n (n n: 1 on n^2; the difference: 1 on t): u (n^2 + 3 t); dt/dn = -2 n
    t = 1 - n * n
    E_t = 2 * n.abs() * E_n + E_n * E_n + U * (n * n + 3 * t + 2 * n.abs() * E_n) + EW_TINY
    d_n = gf * t
    E_dn = _prod_err((gf, E_gf), (t, E_t)) + U * (gf + E_gf) * (t + E_t) + EW_TINY                      # the product: 1
    # p = h - n (1);  s = z (1 - z): 1 - z (1), the product (1), ds/dz = 1 - 2 z
    p = (hh - n).abs()
    E_p = E_n + U * (p + E_n) + EW_TINY
    s = z * fz
    E_s = (1 - 2 * z).abs() * E_z + E_z * E_z + 2 * U * (s + E_z) + EW_TINY
    E_dz = _prod_err((ag, 0.0), (p, E_p), (s, E_s)) + 2 * U * ag * (p + E_p) * (s + E_s) + EW_TINY        # go p (1), times s (1)
    sr = r * (1 - r)
    E_sr = (1 - 2 * r).abs() * E_r + E_r * E_r + 2 * U * (sr + E_r) + EW_TINY
    adn = d_n.abs()
    E_dr = (_prod_err((adn, E_dn), (ghn.abs(), E_ghn), (sr, E_sr))
            + 2 * U * (adn + E_dn) * (ghn.abs() + E_ghn) * (sr + E_sr) + EW_TINY)                        # d_n gh_n (1), times sr (1)
    E_dnr = _prod_err((adn, E_dn), (r, E_r)) + U * (adn + E_dn) * (r + E_r) + EW_TINY                      # the product: 1
    E_dgi = torch.cat([E_dr, E_dz, E_dn], dim=1)
    E_dgh = torch.cat([E_dr, E_dz, E_dnr], dim=1)
    Mgi, Mgh = g["dgi"].abs() + E_dgi, g["dgh"].abs() + E_dgh
    awi, awh = w_ih.double().abs(), w_hh.double().abs()
    # grad_x: 3H-term dot products of inexact dgi with exact weights
    bars["x"] = ((E_dgi @ awi) + dot_gamma(3 * H) * (Mgi @ awi))[:, :I] + EW_TINY
    # grad_h: the same and one more term go z (its product: 1, z inexact): 3H + 1 terms, + 1 for that product's rounding
    gz = ag * (z + E_z)
    bars["h"] = ((E_dgh @ awh) + ag * E_z + dot_gamma(3 * H + 2) * ((Mgh @ awh) + gz))[:, :Hc] + EW_TINY
    # weight gradients: K = V terms (+ 1: the final rounding of the float64 slab sum); bias gradients: V-term sums
    bars["w_ih"] = E_dgi.t() @ ax + dot_gamma(V + 1) * (Mgi.t() @ ax) + EW_TINY * (ax.sum(0) > 0)
    bars["w_hh"] = E_dgh.t() @ ah + dot_gamma(V + 1) * (Mgh.t() @ ah) + EW_TINY * (ah.sum(0) > 0)
    bars["b_ih"] = E_dgi.sum(0) + dot_gamma(V + 1) * Mgi.sum(0) + EW_TINY
    bars["b_hh"] = E_dgh.sum(0) + dot_gamma(V + 1) * Mgh.sum(0) + EW_TINY
    bars["dgi"], bars["dgh"] = E_dgi, E_dgh
    return bars


def worst_ratio(got, ref, bar):
    """max |got - ref| / bar over every element (0 / 0 = 0: an element whose bar is 0 must be exact)."""
    err = (got.double() - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bar)
    return float(ratio.max()) if ratio.numel() else 0.0


# ---- cases --------------------------------------------------------------------------------------------------------------------------
# (input_size, hidden_size, I, Hc)
WIDTHS = {
    "mt_first": (16, 16, 2, 16),          # the multitask model's first iteration: 2 input features under a 16-wide GRU
    "mt_later": (16, 16, 16, 16),
    "floor": (2, 2, 1, 2),
    "h75": (75, 75, 75, 75),              # ZINC: K % 4 = 3, a column tail
    "h110": (110, 110, 110, 110),
    "h128": (128, 128, 128, 128),
    "pad_x": (80, 80, 37, 80),
    "pad_h": (80, 80, 80, 41),
    "rect": (24, 40, 24, 40),             # input_size != hidden_size
}
ROWS = (2, 15, 16, 17, 33, SLAB - 1, SLAB, SLAB + 1, 3 * SLAB + 17)

# every row count with H = 16 and H = 75; every width with a sub-tile and a multi-slab row count
KERNEL_CASES = ([("mt_later", v) for v in ROWS] + [("h75", v) for v in ROWS] +
                [(w, v) for w in ("mt_first", "floor", "h110", "h128", "pad_x", "pad_h", "rect") for v in (15, 3 * SLAB + 17)] +
                [("mt_first", SLAB + 1), ("h128", SLAB)])


def slab_rows(V):
    return max(SLAB, -(-V // MAX_SLABS))


def gru_case(width, V, scale=None):
    """-> dict of host fp32 tensors x (V, I), h (V, Hc), w_ih, w_hh, b_ih, b_hh (nn.GRU's shapes and init range), go (V, H); the same for
    every caller.  scale: the four parameters are multiplied by one factor so that the largest |pre-activation| is `scale`."""
    IN, H, I, Hc = WIDTHS[width]
    gen = torch.Generator().manual_seed(1000 * sorted(WIDTHS).index(width) + V)
    k = 1.0 / math.sqrt(H)
    c = {"x": torch.randn(V, I, generator=gen), "h": torch.randn(V, Hc, generator=gen),
         "w_ih": (torch.rand(3 * H, IN, generator=gen) * 2 - 1) * k, "w_hh": (torch.rand(3 * H, H, generator=gen) * 2 - 1) * k,
         "b_ih": (torch.rand(3 * H, generator=gen) * 2 - 1) * k, "b_hh": (torch.rand(3 * H, generator=gen) * 2 - 1) * k,
         "go": torch.randn(V, H, generator=gen)}
    if scale is not None:
        f = gru_ref64(c["x"], c["h"], c["w_ih"], c["w_hh"], c["b_ih"], c["b_hh"])
        top = max(float(f["a_r"].abs().max()), float(f["a_z"].abs().max()), float((f["gi_n"] + f["r"] * f["gh_n"]).abs().max()))
        for name in ("w_ih", "w_hh", "b_ih", "b_hh"):
            c[name] = (c[name].double() * (scale / top)).float()
    return c


PARAMS = ("w_ih", "w_hh", "b_ih", "b_hh")
NN_NAMES = {"w_ih": "weight_ih_l0", "w_hh": "weight_hh_l0", "b_ih": "bias_ih_l0", "b_hh": "bias_hh_l0"}      # torch.nn.GRU's


def case_params(c):
    return [c[k] for k in ("x", "h") + PARAMS]
