"""Host side of the kernel-level tests of pna_tower_layer_bf16 (pna_bf16_small.hip), no tests in here: weight images built from the
layout text of include/pna_amd.h alone, a ctypes caller that owns every pointer and pitch of pna_tower_layer_bf16_args, and staged
float64 models of launch 2 on the exact bf16 operands.

The stage probes make the LATER stages exact, so that each stage is held to the single-rounding contract of bf16_tower_ref.py,
|got - ref64| <= 2u |ref64| + 4u M (u = 2^-8, M the absolute mass of the element), instead of a bound propagated through the layer:
  gather    post_img is a 0/1 selector (Fo = A Fi, one identity scaler, nothing else): y IS the LDS aggregate tile.  Messages are
            rebuilt in fp32 from the x_cat the call left behind, (x_src[u] + x_dst[v]) + table[type], the kernel's own association
  towers    aggregators max / min only: the bf16 A operand in LDS is a selection, known exactly on the host; mix_img NULL
  mixing    the tower stage is a selector of the exact max aggregate, so hc is exact and the mixing network is the one rounding
A `case` is a dict of host tensors: the operands as the kernel gets them (bf16 / fp32 / int32) and, under "W", the same weights as
float64 tensors in model layout: Wa, Wb (T, Fi, Fi), b (T, Fi), Wz (T, S, Fo, A, Fi), Wh (T, Fo, Fi), bias (T Fo), Wm (No, T Fo),
bm (No), table (n_types, T, Fi).  The falsified models (`falsify=`) are the teeth of test_bf16_small_ref_host.py."""
import ctypes

import torch

import bf16_tower_ref as B
from pna_amd import _lib

U = B.U
BF = torch.bfloat16
CANARY = 1232.0                                   # exact in bf16; never the value of an output of these cases
DEGREES = (0, 1, 2, 3, 4, 5, 7, 8, 9, 11)         # row i has in-degree DEGREES[i % 10]: every class of the 4-edge unroll and its tail
HUB = 1003                                        # ... and one row walks about a thousand edges (1003 = 4 * 250 + 3)


def rnd(x, m):
    return (x + m - 1) // m * m


def dims(T, Fi, Fo, A):
    """Fp, Fop, Kp, Khp of include/pna_amd.h."""
    Fp = rnd(Fi, 8)
    return Fp, rnd(Fo, 16), rnd(A * Fp, 32), rnd(Fi, 32)


# ---- weight images, from the header's layout text --------------------------------------------------------------------------------
def contract_image(rows):
    """pna_contract_bf16_args.w_img of one block: (N, K) -> bf16 (1, R, round32(K)), R = 16 t ceil(N / (16 t)), t the kernel's tiles."""
    N, K = rows.shape
    tiles = _lib.lib().pna_contract_bf16_tiles(N)
    assert tiles > 0, N
    img = torch.zeros(1, rnd(N, 16 * tiles), rnd(K, 32), dtype=BF)
    img[0, :N, :K] = rows
    return img


def proj_images(Wa, Wb, b, divide):
    """proj_img, proj_bias: 2 T Fp projection rows, tower t's W_a at rows t Fp, W_b at T Fp + t Fp, over Kin input columns."""
    T, Fi = Wa.shape[0], Wa.shape[1]
    Fp = rnd(Fi, 8)
    rows = torch.zeros(2 * T * Fp, T * Fi if divide else Fi, dtype=BF)
    bias = torch.zeros(2 * T * Fp, dtype=BF)
    for t in range(T):
        c0 = t * Fi if divide else 0
        rows[t * Fp:t * Fp + Fi, c0:c0 + Fi] = Wa[t]
        rows[(T + t) * Fp:(T + t) * Fp + Fi, c0:c0 + Fi] = Wb[t]
        bias[(T + t) * Fp:(T + t) * Fp + Fi] = b[t]
    return contract_image(rows), bias


def edge_image(We):
    """The contraction image that makes the edge table: (T, Fi, ed) -> T Fp rows, W_e of tower t at rows t Fp."""
    T, Fi, ed = We.shape
    Fp = rnd(Fi, 8)
    rows = torch.zeros(T * Fp, ed, dtype=BF)
    for t in range(T):
        rows[t * Fp:t * Fp + Fi] = We[t]
    return contract_image(rows)


def edge_table(rows, pitch=None):
    """bf16 (n_types, pitch >= T Fp): the (n_types, T, Fi) type rows of every tower at columns t Fp, zeros between."""
    n, T, Fi = rows.shape
    Fp = rnd(Fi, 8)
    tab = torch.zeros(n, pitch or T * Fp, dtype=BF)
    for t in range(T):
        tab[:, t * Fp:t * Fp + Fi] = rows[:, t]
    return tab


def post_image(Wz, Wh):
    """post_img, flat: [T][S][Fop][Kp] with element [t][s][n][a Fp + f] = Wz[t][s][n][a][f], then (Wh not None) [T][Fop][Khp]."""
    T, S, Fo, A, Fi = Wz.shape
    Fp, Fop, Kp, Khp = dims(T, Fi, Fo, A)
    img = torch.zeros(T, S, Fop, Kp, dtype=BF)
    for a in range(A):
        img[:, :, :Fo, a * Fp:a * Fp + Fi] = Wz[:, :, :, a, :]
    if Wh is None:
        return img.reshape(-1)
    own = torch.zeros(T, Fop, Khp, dtype=BF)
    own[:, :Fo, :Fi] = Wh
    return torch.cat([img.reshape(-1), own.reshape(-1)])


def mix_image(Wm):
    No, K = Wm.shape
    img = torch.zeros(rnd(No, 16), rnd(K, 32), dtype=BF)
    img[:No, :K] = Wm
    return img


def tower_weights(towers):
    """Model-layout weights of PNATower modules: the pretrans Linear is [W_a | W_b | W_e] over [h_src | h_dst | ef], the posttrans
    Linear [W_h | scaler-major, aggregator, feature] (models/dgl/pna_layer.py:35-50, :65-74)."""
    t0 = towers[0]
    Fi, A, S = t0.in_dim, len(t0.aggregators), len(t0.scalers)
    pre = [t.pretrans.fully_connected[0].linear for t in towers]
    post = [t.posttrans.fully_connected[0].linear for t in towers]
    Fo = post[0].out_features
    return {"Wa": torch.stack([l.weight[:, :Fi] for l in pre]), "Wb": torch.stack([l.weight[:, Fi:2 * Fi] for l in pre]),
            "We": torch.stack([l.weight[:, 2 * Fi:] for l in pre]), "b": torch.stack([l.bias for l in pre]),
            "Wh": torch.stack([l.weight[:, :Fi] for l in post]),
            "Wz": torch.stack([l.weight[:, Fi:].reshape(Fo, S, A, Fi).permute(1, 0, 2, 3) for l in post]),
            "bias": torch.cat([l.bias for l in post])}


def images_from_towers(towers, mix, divide):
    """The images of _small_images_bf16, independently: proj, proj_bias, edge, post, post_bias, mix, mix_bias."""
    with torch.no_grad():
        w = tower_weights(towers)
        proj, pbias = proj_images(w["Wa"], w["Wb"], w["b"], divide)
        return {"proj": proj, "proj_bias": pbias, "edge": edge_image(w["We"]) if w["We"].shape[2] else None,
                "post": post_image(w["Wz"], w["Wh"]), "post_bias": w["bias"].clone(),
                "mix": None if mix is None else mix_image(mix.linear.weight), "mix_bias": None if mix is None else mix.linear.bias.clone()}


def images_from_simple_layer(layer):
    """The images of _small_simple_images_bf16: the posttrans Linear of PNASimpleLayer is [scaler-major, aggregator, feature]."""
    lin = layer.posttrans.fully_connected[0].linear
    A, S, F, N = len(layer.aggregators), len(layer.scalers), layer.in_dim, lin.out_features
    with torch.no_grad():
        Wz = lin.weight.reshape(N, S, A, F).permute(1, 0, 2, 3)[None]
        Fp, Fop, Kp, _ = dims(1, F, N, A)
        return {"post": post_image(Wz, None).reshape(1, S, Fop, Kp), "post_bias": lin.bias.clone()}


def fold_batchnorm64(bn):
    """col_scale, col_shift of an eval BatchNorm1d in float64."""
    cs = bn.weight.detach().double() / torch.sqrt(bn.running_var.double() + bn.eps)
    return cs, bn.bias.detach().double() - bn.running_mean.double() * cs


# ---- graphs with prescribed in-degrees ---------------------------------------------------------------------------------------------
def degree_graph(V, seed, hub=HUB):
    """CSR by destination with in-degree DEGREES[i % 10] at row i and `hub` edges into one row -> rowptr, col (int32), dst (int64)."""
    deg = torch.tensor([DEGREES[i % len(DEGREES)] for i in range(V)])
    hub_row = 10 if V > 10 else V - 1
    if hub:
        deg[hub_row] = hub
    rowptr = torch.zeros(V + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(deg, 0)
    col = torch.randint(0, V, (int(rowptr[-1]),), generator=torch.Generator().manual_seed(seed))
    return rowptr.to(torch.int32), col.to(torch.int32), torch.arange(V).repeat_interleave(deg)


def assert_degree_classes(rowptr, V, hub=HUB):
    """Every row class the graph was built for is there: in-degrees 0..5, 7, 8, 9, 11 (V permitting) and the hub row."""
    deg = (rowptr[1:] - rowptr[:-1]).long()
    hist = torch.bincount(deg)
    want = {}
    for i in range(V):
        want[DEGREES[i % 10]] = want.get(DEGREES[i % 10], 0) + 1
    if hub:
        was = DEGREES[(10 if V > 10 else V - 1) % 10]
        want[was] -= 1
        want[hub] = want.get(hub, 0) + 1
    for d, n in want.items():
        assert (int(hist[d]) if d < hist.numel() else 0) == n, (d, n, hist.tolist()[:12])
    assert int(hist.sum()) == V and (V <= 10 or all(int(hist[d]) >= 1 for d in DEGREES))
    if hub:
        assert int(deg.max()) == hub and hub % 4 == 3


# ---- cases -------------------------------------------------------------------------------------------------------------------------
def make_case(seed, V, T, Fi, Fo, aggs, *, divide=False, scales=(False,), post="random", self_block=True, post_bias=False,
              row_post=False, bn=False, slope=1.0, residual=False, No=None, mix_bias=False, n_types=0, bad_types=False,
              no_self=False, hub=HUB):
    """One call's operands.  post: "random" weights or the "selector" (Fo = A Fi: output a Fi + f of a tower is its aggregate a,
    feature f; no self block weights).  scales: one bool per scaler block, True = an fp32 row scale, False = NULL.  No: the mixing
    network's output width (None = no mixing network).  bad_types: edge types -3 and 9 among the in-range ones."""
    gen = torch.Generator().manual_seed(seed)
    A, S = len(aggs), len(scales)
    Kin = T * Fi if divide else Fi
    rowptr, col, dst = degree_graph(V, seed + 1, hub)
    E = col.numel()

    def randn(*shape, scale=1.0, shift=0.0):
        return (torch.randn(*shape, generator=gen) * scale + shift).to(BF)

    c = dict(V=V, T=T, Fi=Fi, Fo=Fo, divide=divide, aggs=list(aggs), S=S, rowptr=rowptr, col=col, dst=dst, slope=float(slope),
             no_self=no_self, No=No, hub=hub)
    c["h"] = randn(V, Kin, scale=1.5, shift=0.25)
    W = {}
    if not no_self:
        W["Wa"], W["Wb"] = randn(T, Fi, Fi, scale=Fi ** -0.5), randn(T, Fi, Fi, scale=Fi ** -0.5)
        W["b"] = randn(T, Fi, scale=0.5)
        c["proj_img"], c["proj_bias"] = proj_images(W["Wa"], W["Wb"], W["b"], divide)
    if post == "selector":
        assert Fo == A * Fi
        Wz = torch.zeros(T, S, Fo, A, Fi, dtype=BF)
        for a in range(A):
            Wz[:, 0, a * Fi:(a + 1) * Fi, a, :] = torch.eye(Fi, dtype=BF)
        Wh = torch.zeros(T, Fo, Fi, dtype=BF)
    else:
        Wz = randn(T, S, Fo, A, Fi, scale=(A * Fi) ** -0.5)
        Wh = randn(T, Fo, Fi, scale=Fi ** -0.5) if self_block else torch.zeros(T, Fo, Fi, dtype=BF)
    W["Wz"], W["Wh"] = Wz, None if no_self else Wh
    c["post_img"] = post_image(Wz, W["Wh"])
    c["row_scale"] = [(torch.rand(V, generator=gen) * 1.5 + 0.3).float() if on else None for on in scales]
    c["post_bias"] = randn(T * Fo, scale=0.5) if post_bias else None
    c["row_post"] = (torch.rand(V, generator=gen) * 0.5 + 0.1).float() if row_post else None
    c["col_scale"] = (torch.rand(T * Fo, generator=gen) + 0.5).float() if bn else None
    c["col_shift"] = (torch.randn(T * Fo, generator=gen) * 0.5).float() if bn else None
    W["bias"] = c["post_bias"]
    if No is not None:
        W["Wm"] = randn(No, T * Fo, scale=(T * Fo) ** -0.5)
        W["bm"] = randn(No, scale=0.5) if mix_bias else None
        c["mix_img"], c["mix_bias"] = mix_image(W["Wm"]), W["bm"]
    width = No if No is not None else T * Fo
    c["residual"] = randn(V, width) if residual else None
    if n_types:
        W["table"] = randn(n_types, T, Fi, scale=0.7)
        c["edge_table"] = edge_table(W["table"])
        et = torch.randint(0, n_types, (E,), generator=gen).to(torch.int32)
        if bad_types:
            et[torch.arange(0, E, 5)] = -3
            et[torch.arange(2, E, 7)] = 9
            assert int((et == -3).sum()) and int((et == 9).sum())
        c["edge_type"], c["n_types"] = et, n_types
    c["W"] = {k: None if v is None else v.double() for k, v in W.items()}
    return c


def width_of(c):
    return c["No"] if c["No"] is not None else c["T"] * c["Fo"]


# ---- the direct caller -------------------------------------------------------------------------------------------------------------
def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def run(dev, c, *, x_extra=8, y_extra=5, h_pitch=None, res_pitch=None, h_tail_readable=0, table_pitch=None):
    """pna_tower_layer_bf16 on case c through ctypes.  y and x_cat are round16(V) + 16 rows of width + y_extra / 2 T Fp + x_extra
    columns prefilled with CANARY; h and residual sit inside NaN-filled buffers of h_pitch / res_pitch columns when given.
    -> dict(rc, y, x_cat (whole buffers, on the host), h_dev, keep).  Every pointer of the args struct is set here and only here."""
    V, T, Fi, Fo = c["V"], c["T"], c["Fi"], c["Fo"]
    Fp = rnd(Fi, 8)
    xw, width, rows = 2 * T * Fp, width_of(c), rnd(V, 16) + 16
    keep = []

    def d(t):
        if t is None:
            return None
        keep.append(t.contiguous().to(dev))
        return keep[-1]

    def pitched(t, pitch):
        if t is None or pitch is None:
            return d(t)
        buf = torch.full((t.shape[0], pitch), float("nan"), dtype=BF)
        buf[:, :t.shape[1]] = t
        return d(buf)[:, :t.shape[1]]

    a = _lib.PnaTowerLayerBf16Args()
    a.rowptr, a.col = _ptr(d(c["rowptr"])), _ptr(d(c["col"]))
    a.V, a.n_tower, a.Fi, a.Fo, a.divide_input, a.n_scaler, a.n_aggr = V, T, Fi, Fo, int(c["divide"]), c["S"], len(c["aggs"])
    a.no_self_panel, a.h_tail_readable = int(c["no_self"]), int(h_tail_readable)
    for i, name in enumerate(c["aggs"]):
        a.aggr[i] = _lib.AGG_CODES[name]
    h = pitched(c["h"], h_pitch)
    a.h, a.ldh = _ptr(h), h.stride(0)
    y = torch.full((rows, width + y_extra), CANARY, dtype=BF, device=dev)
    a.y, a.ldy = _ptr(y), width + y_extra
    x_cat = None
    if not c["no_self"]:
        x_cat = torch.full((rows, xw + x_extra), CANARY, dtype=BF, device=dev)
        a.x_cat, a.ldx = _ptr(x_cat), xw + x_extra
        a.proj_img, a.proj_bias = _ptr(d(c["proj_img"])), _ptr(d(c.get("proj_bias")))
    for s, rs in enumerate(c["row_scale"]):
        a.row_scale[s] = None if rs is None else d(rs).data_ptr()
    a.post_img, a.post_bias = _ptr(d(c["post_img"])), _ptr(d(c["post_bias"]))
    a.row_post, a.col_scale, a.col_shift = _ptr(d(c["row_post"])), _ptr(d(c["col_scale"])), _ptr(d(c["col_shift"]))
    if c["No"] is not None:
        a.mix_img, a.mix_bias, a.No = _ptr(d(c["mix_img"])), _ptr(d(c["mix_bias"])), c["No"]
    a.mix_slope = c["slope"]
    res = pitched(c["residual"], res_pitch)
    if res is not None:
        a.residual, a.ld_res = _ptr(res), res.stride(0)
    if c.get("edge_type") is not None:
        tab = c["edge_table"] if table_pitch is None else edge_table(c["W"]["table"].to(BF), table_pitch)
        tab = d(tab)
        a.edge_type, a.edge_table, a.ld_edge_table, a.n_edge_types = _ptr(d(c["edge_type"])), _ptr(tab), tab.stride(0), c["n_types"]
    rc = _lib.lib().pna_tower_layer_bf16(ctypes.byref(a), _lib.stream_ptr(dev))
    torch.cuda.synchronize(dev)
    err = _lib.lib().pna_last_error().decode() if rc else ""
    return {"rc": rc, "error": err, "y": y.cpu(), "x_cat": None if x_cat is None else x_cat.cpu(), "h_dev": h, "keep": keep,
            "width": width, "xw": xw, "rows": rows}


def assert_untouched(buf, V, cols, what):
    """Columns >= cols of every row and all of the rows >= V of a CANARY-prefilled buffer still hold the canary."""
    assert bool((buf[:, cols:] == CANARY).all()), f"{what}: columns beyond {cols} were written"
    assert bool((buf[V:] == CANARY).all()), f"{what}: rows beyond {V} were written"


# ---- staged float64 models ---------------------------------------------------------------------------------------------------------
def towers_h(c):
    """(V, T, Fi) float64: the input slice of every tower."""
    h, T, Fi = c["h"].double(), c["T"], c["Fi"]
    return h.reshape(-1, T, Fi) if c["divide"] else h[:, None, :].expand(-1, T, -1)


def project64(c):
    """Launch 1: ref64 (V, 2 T Fp) and its absolute mass; the padding columns [Fi, Fp) of every block are exact zeros."""
    W, T, Fi = c["W"], c["T"], c["Fi"]
    Fp = rnd(Fi, 8)
    ht = towers_h(c)
    ref = torch.zeros(c["V"], 2, T, Fp, dtype=torch.float64)
    mass = torch.zeros_like(ref)
    ref[:, 0, :, :Fi] = torch.einsum("vtf,tnf->vtn", ht, W["Wa"])
    ref[:, 1, :, :Fi] = torch.einsum("vtf,tnf->vtn", ht, W["Wb"]) + W["b"]
    mass[:, 0, :, :Fi] = torch.einsum("vtf,tnf->vtn", ht.abs(), W["Wa"].abs())
    mass[:, 1, :, :Fi] = torch.einsum("vtf,tnf->vtn", ht.abs(), W["Wb"].abs()) + W["b"].abs()
    return ref.reshape(c["V"], -1), mass.reshape(c["V"], -1)


def contract_tol(ref, mass):
    return 2 * U * ref.abs() + 4 * U * mass


def messages(c, x_cat, dtype=torch.float32, clamp=True, skip_tail3=False):
    """Per-edge messages (E', T Fi) in CSR order from the bf16 x_cat (V, >= 2 T Fp) of the call (no_self: from h), in the kernel's
    association (x_src[u] + x_dst[v]) + table[type] -- exact in float64, the kernel's own bits in float32 -- and their col / dst.
    Falsifiers: clamp=False gives an out-of-table type no edge term; skip_tail3 drops the last edge of rows with deg % 4 == 3."""
    T, Fi, V = c["T"], c["Fi"], c["V"]
    Fp = rnd(Fi, 8)
    u, v = c["col"].long(), c["dst"]
    if c["no_self"]:
        m = c["h"].to(dtype)[u][:, None, :]
    else:
        x = x_cat[:V, :2 * T * Fp].to(dtype).reshape(V, 2, T, Fp)[..., :Fi]
        m = x[u, 0] + x[v, 1]
        if c.get("edge_type") is not None:
            tab, et = c["W"]["table"].to(dtype), c["edge_type"].long()
            n = tab.shape[0]
            term = tab[et.clamp(0, n - 1)]
            if not clamp:
                term = term * ((et >= 0) & (et < n)).to(dtype)[:, None, None]
            m = m + term
    m = m.reshape(-1, T * Fi)
    if skip_tail3:
        rp = c["rowptr"].long()
        deg = rp[1:] - rp[:-1]
        last = rp[1:][deg % 4 == 3] - 1
        keep = torch.ones(u.numel(), dtype=torch.bool)
        keep[last] = False
        return m[keep], u[keep], v[keep]
    return m, u, v


def _blocks(z, c, A):
    """(V, A T Fi) aggregator-major -> (V, T, A, Fi)."""
    return z.reshape(c["V"], A, c["T"], c["Fi"]).permute(0, 2, 1, 3)


def gather64(c, x_cat, **falsify):
    """The aggregates (V, T, A, Fi) in float64 of the exact messages."""
    m, u, v = messages(c, x_cat, torch.float64, **falsify)
    return _blocks(B.aggregate64(m, u, v, c["V"], c["aggs"]), c, len(c["aggs"]))


def gather_tol(c, x_cat):
    """_check_gather's bar of test_gpu_bf16_tower_kernels.py: 2u |z| + 4u (aggregate_mass + stat_floor), (V, T, A, Fi)."""
    m, u, v = messages(c, x_cat, torch.float64)
    z = B.aggregate64(m, u, v, c["V"], c["aggs"])
    tol = 2 * U * z.abs() + 4 * U * (B.aggregate_mass(m, u, v, c["V"], c["aggs"]) + B.stat_floor(m, u, v, c["V"], c["aggs"]))
    return _blocks(tol, c, len(c["aggs"]))


def selections(c, x_cat, names=("max", "min")):
    """bf16 (V, T, len(names), Fi): max / min of the fp32 messages, rounded once -- what the kernel holds bit for bit."""
    m, u, v = messages(c, x_cat, torch.float32)
    return _blocks(B.aggregate64(m, u, v, c["V"], list(names)).to(BF), c, len(names))


def selector_view(y, c):
    """y (>= V, >= T A Fi) of a selector case -> (V, T, A, Fi)."""
    T, A, Fi = c["T"], len(c["aggs"]), c["Fi"]
    return y[:c["V"], :T * A * Fi].reshape(c["V"], T, A, Fi)


def towers64(c, a, falsify=None):
    """z and its absolute mass (V, T Fo) before the activation: ((b + W_h h + sum_s rs_s (W_s a)) * row_post) * cs + ct on the exact
    aggregates a (V, T, A, Fi) float64.  falsify: ("drop_self", t) | ("swap_scales", i, j) | ("shift_block", t, a) -- that block's
    weights moved one feature up -- | ("pad_weight", t): weight 1 in every output row of tower t's scaler block 0 on the padded
    column Fi of aggregator block 0, the column holding the last feature again (a tile whose padding is not zeroed)."""
    W, T, Fo, V = c["W"], c["T"], c["Fo"], c["V"]
    Wz, Wh = W["Wz"], W["Wh"]
    rs = [torch.ones(V, dtype=torch.float64) if r is None else r.double() for r in c["row_scale"]]
    kind = falsify[0] if falsify else None
    if kind == "swap_scales":
        rs[falsify[1]], rs[falsify[2]] = rs[falsify[2]], rs[falsify[1]]
    if kind == "shift_block":
        Wz = Wz.clone()
        Wz[falsify[1], :, :, falsify[2], :] = torch.roll(Wz[falsify[1], :, :, falsify[2], :], 1, dims=-1)
    z = torch.zeros(V, T, Fo, dtype=torch.float64)
    mass = torch.zeros_like(z)
    if W.get("bias") is not None:
        z, mass = z + W["bias"].reshape(T, Fo), mass + W["bias"].abs().reshape(T, Fo)
    if Wh is not None:
        ht = towers_h(c)
        own = torch.einsum("vtf,tnf->vtn", ht, Wh)
        if kind == "drop_self":
            own[:, falsify[1]] = 0
        z, mass = z + own, mass + torch.einsum("vtf,tnf->vtn", ht.abs(), Wh.abs())
    for s in range(c["S"]):
        z = z + rs[s][:, None, None] * torch.einsum("vtaf,tnaf->vtn", a, Wz[:, s])
        mass = mass + rs[s].abs()[:, None, None] * torch.einsum("vtaf,tnaf->vtn", a.abs(), Wz[:, s].abs())
    if kind == "pad_weight":
        z[:, falsify[1]] += (rs[0] * a[:, falsify[1], 0, -1])[:, None]
    z, mass = z.reshape(V, T * Fo), mass.reshape(V, T * Fo)
    if c["row_post"] is not None:
        z, mass = z * c["row_post"].double()[:, None], mass * c["row_post"].double().abs()[:, None]
    if c["col_scale"] is not None:
        cs, ct = c["col_scale"].double(), c["col_shift"].double()
        z, mass = z * cs + ct, mass * cs.abs() + ct.abs()
    return z, mass


def finish64(c, z, mass):
    """residual + act(z) and its mass."""
    z = torch.where(z < 0, c["slope"] * z, z)
    if c["residual"] is not None:
        z, mass = z + c["residual"].double(), mass + c["residual"].double().abs()
    return z, mass


def mix64(c, zc, falsify=None):
    """W_mix zc + b_mix and its mass (V, No) before the activation; falsify: ("drop_mix_bias",)."""
    W = c["W"]
    z, mass = zc @ W["Wm"].T, zc.abs() @ W["Wm"].abs().T
    if W.get("bm") is not None:
        mass = mass + W["bm"].abs()
        if not falsify:
            z = z + W["bm"]
    return z, mass


def towers_expect(c, x_cat, falsify=None):
    """Tower contraction probe (max / min aggregators, no mixing network): ref64, tol (V, T Fo)."""
    a = selections(c, x_cat, c["aggs"]).double()
    z, mass = finish64(c, *towers64(c, a, falsify))
    return z, contract_tol(z, mass)


def mix_expect(c, x_cat, falsify=None):
    """Mixing probe (the tower stage selects the exact max aggregate): ref64, tol (V, No)."""
    zc = selections(c, x_cat, ["max"]).double().reshape(c["V"], -1)
    z, mass = finish64(c, *mix64(c, zc, falsify))
    return z, contract_tol(z, mass)


def compose64(c):
    """All stages in float64 without any rounding: the projections, the aggregates of the exact messages, the towers, the mixing
    network, activation and residual -- ref64 of bf16_tower_ref.layer_models, stage by stage."""
    x, _ = project64(c)
    a = gather64(c, x)
    z, mass = towers64(c, a)
    if c["No"] is None:
        return finish64(c, z, mass)[0]
    return finish64(c, *mix64(c, z))[0]


def emulated_x_cat(c):
    """x_cat as launch 1 leaves it up to its own rounding: R(project64), for the host-only teeth."""
    return B.rbf(project64(c)[0]).to(BF)


def outside(x, ref, tol):
    """Number of elements of x outside the bar."""
    return int((~((x - ref).abs() <= tol)).sum())


def worst(x, ref, tol):
    bad = ~((x - ref).abs() <= tol)
    err = (x - ref).abs()
    return f"{int(bad.sum())} elements outside the contract, worst {float(err[bad].max()) if bad.any() else 0.0:.3e} at {bad.nonzero()[:3].tolist()}"


def case_from_layer(layer, cfg, rowptr, col, dst, h, snorm_n, avg_log, type_rows=None, edge_type=None):
    """The case of a PNALayer (float64 copies of its bf16 state) for compose64: cfg as in bf16_tower_ref.layer_models."""
    towers = list(layer.towers)
    V, T = h.shape[0], len(towers)
    w = {k: v.detach().double() for k, v in tower_weights(towers).items()}
    Fi, Fo = w["Wa"].shape[1], w["Wh"].shape[1]
    deg = (rowptr[1:] - rowptr[:-1]).numpy()
    c = dict(V=V, T=T, Fi=Fi, Fo=Fo, divide=cfg["divide_input"], aggs=cfg["aggregators"], S=len(cfg["scalers"]), rowptr=rowptr, col=col,
             dst=dst, slope=0.01, no_self=False, No=layer.out_dim, h=h)
    c["row_scale"] = [None if s == "identity" else torch.from_numpy(B.scale64(s, deg, avg_log)) for s in cfg["scalers"]]
    c["row_post"] = snorm_n.double().reshape(-1) if cfg["graph_norm"] else None
    c["col_scale"] = c["col_shift"] = None
    if cfg["batch_norm"]:
        folds = [fold_batchnorm64(t.batchnorm_h) for t in towers]
        c["col_scale"], c["col_shift"] = torch.cat([f[0] for f in folds]), torch.cat([f[1] for f in folds])
    c["residual"] = h if layer.residual else None
    mix = layer.mixing_network.linear
    W = {"Wa": w["Wa"], "Wb": w["Wb"], "b": w["b"], "Wz": w["Wz"], "Wh": w["Wh"], "bias": w["bias"],
         "Wm": mix.weight.detach().double(), "bm": mix.bias.detach().double()}
    if type_rows is not None:
        W["table"] = torch.einsum("ne,tfe->ntf", type_rows.double(), w["We"])
        c["edge_type"], c["n_types"] = edge_type, type_rows.shape[0]
    c["W"] = W
    return c


# ---- the probes' inputs (shared by the GPU probes and the host-only teeth) ---------------------------------------------------------
ALL_AGGS = ["mean", "sum", "max", "min", "std", "var"]

# gather probe: V, T, Fi, aggregators, edge types, out-of-table types among them.  T round8(Fi) <= 512: pna_gather_bf16 serves the same rows
GATHER = [
    dict(V=1, T=1, Fi=1, aggs=ALL_AGGS, n_types=0, bad_types=False, hub=3),
    dict(V=15, T=5, Fi=7, aggs=ALL_AGGS, n_types=1, bad_types=True),
    dict(V=16, T=8, Fi=8, aggs=ALL_AGGS, n_types=2, bad_types=True),
    dict(V=17, T=1, Fi=33, aggs=ALL_AGGS, n_types=4, bad_types=True),
    dict(V=33, T=5, Fi=75, aggs=["mean", "max", "min", "std"], n_types=4, bad_types=True),
    dict(V=33, T=8, Fi=1, aggs=["var", "min", "sum"], n_types=2, bad_types=False),
    dict(V=700, T=5, Fi=75, aggs=ALL_AGGS, n_types=4, bad_types=False),
    dict(V=700, T=8, Fi=33, aggs=ALL_AGGS, n_types=2, bad_types=True),
    dict(V=700, T=1, Fi=75, aggs=["std", "max", "mean"], n_types=0, bad_types=False),
    dict(V=700, T=1, Fi=8, aggs=ALL_AGGS, n_types=4, bad_types=True),
]


def gather_case(i):
    k = dict(GATHER[i])
    A = len(k["aggs"])
    return make_case(100 + i, k.pop("V"), k.pop("T"), k["Fi"], A * k.pop("Fi"), k.pop("aggs"), post="selector", **k)


# the no_self_panel form of the gather probe: Fi, pitch of the NaN-padded buffer h sits in (None = contiguous), h_tail_readable
GATHER_SIMPLE = [(80, None, 0), (75, None, 0), (75, 88, 1)]


def gather_simple_case(i, V=700):
    Fi = GATHER_SIMPLE[i][0]
    return make_case(200 + i, V, 1, Fi, 6 * Fi, ALL_AGGS, post="selector", no_self=True)


# tower contraction probe.  scales: True = an fp32 row scale, False = NULL ([None, amp, None] is (False, True, False))
TOWERS = [
    dict(V=33, T=1, Fi=1, Fo=1, aggs=["max"], scales=(False,)),
    dict(V=700, T=5, Fi=75, Fo=14, aggs=["max", "min"], scales=(False, True, True), post_bias=True, row_post=True, bn=True, slope=0.01,
         residual=True, n_types=4, bad_types=True),
    dict(V=17, T=3, Fi=7, Fo=16, aggs=["max", "min"], scales=(True, True), divide=True, post_bias=True, slope=0.0),
    dict(V=700, T=8, Fi=20, Fo=17, aggs=["max"], scales=(False, True, False), divide=True, row_post=True, residual=True),
    dict(V=100, T=1, Fi=33, Fo=75, aggs=["max", "min"], scales=(True, True, True), bn=True, slope=0.0, n_types=2),
    dict(V=50, T=3, Fi=33, Fo=130, aggs=["max", "min"], scales=(False,), post_bias=True, bn=True, slope=0.01, residual=True),
    dict(V=700, T=5, Fi=75, Fo=75, aggs=["max"], scales=(True,), divide=True, row_post=True, slope=0.01),
    dict(V=16, T=8, Fi=7, Fo=14, aggs=["max", "min"], scales=(True, False), post_bias=True, row_post=True, bn=True, slope=0.0, residual=True,
         n_types=1, bad_types=True),
]


def towers_case(i):
    k = dict(TOWERS[i])
    return make_case(300 + i, k.pop("V"), k.pop("T"), k.pop("Fi"), k.pop("Fo"), k.pop("aggs"), **k)


def largest_tile_shape(Fi=33, A=2):
    """(T, bytes): the most towers of Fi features and A aggregators (shared input, no mixing network) whose 16-row tile
    ops.tower_layer_bf16_lds_bytes still admits under 160 KiB and whose 2 T Fp projection columns pna_contract_bf16 serves."""
    from pna_amd import ops
    best = None
    for T in range(1, 65):
        b = ops.tower_layer_bf16_lds_bytes(T, Fi, 3, A, False)
        if b <= 160 * 1024 and 2 * T * rnd(Fi, 8) <= 4096:
            best = (T, b)
    return best


def largest_tile_case():
    T, _ = largest_tile_shape()
    return make_case(390, 40, T, 33, 3, ["max", "min"], scales=(False, True), post_bias=True, row_post=True, slope=0.01, hub=203)


# mixing probe: (T, Fi) with T Fi = T Fo in {14, 70, 75, 128}, No in {1, 16, 30, 75, 200}
MIX = [
    dict(V=33, T=2, Fi=7, No=1),
    dict(V=700, T=5, Fi=14, No=16, mix_bias=True, slope=0.01, residual=True),
    dict(V=100, T=1, Fi=75, No=30, mix_bias=True, slope=0.0),
    dict(V=700, T=8, Fi=16, No=75, slope=0.01, residual=True, n_types=4),
    dict(V=17, T=5, Fi=15, No=200, mix_bias=True, slope=0.0, residual=True),
]


def mix_case(i):
    k = dict(MIX[i])
    Fi = k.pop("Fi")
    return make_case(400 + i, k.pop("V"), k.pop("T"), Fi, Fi, ["max"], post="selector", **k)
