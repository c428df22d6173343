"""pna_simple_train_fwd_f32 / pna_simple_train_bwd_f32 through ctypes (PNASimpleLayer's training forward and backward on a molecule
batch as one C call each: models/dgl/pna_layer.py:197-213 in train mode): the saved state against pna_segreduce_fwd_f32's bits, z and
the BatchNorm statistics against float64, every gradient per element against oracle.torch_oracle.simple_layer_train_step in float64,
bitwise repeatability, the argument checks."""
import ctypes
import types

import pytest
import torch

import small_train_cases as C
from pna_amd import _lib, autograd as AG, ops
from pna_amd import functional as PF
from pna_amd.dgl.pna_layer import PNASimpleLayer, _row_scales
from pna_amd.graph import Graph
from tower_train_run import pitched_input, pitched_output

pytestmark = pytest.mark.gpu

# F, N, scalers, nodes: the two golden graphs (V no multiple of 16; a row of 132 in-edges), the smallest and the largest widths, and the
# hand-made graph (a row without in-edges, rows of in-degree 1, an arg tie) with and without the residual
CASES = ["simple_train_f20", "simple_train_f75", "narrow", "wide", "hand_res", "hand_nores"]


class _Run:
    """One forward + backward through the two C calls on a case's inputs: every output as a tensor.  pitches: None = every operand
    contiguous; a dict {"h" / "out" / "go": row pitch} (the operands whose pitch the ABI carries: grad_h has none) = that operand is a
    tower_train_run.pitched_input / pitched_output view (`buffers` keeps the outputs' whole buffers)."""

    def __init__(self, name, dev, repeat=1, pitches=None):
        meta, a, sd, ref = C.case(name)
        self.meta, self.arrays, self.sd, self.ref = meta, a, sd, ref
        V, F, N = meta["N"], meta["F"], meta["out_dim"]
        scalers = meta["scalers"].split()
        S = len(scalers)
        self.g = g = Graph(a["src"], a["dst"], V).to(dev)
        pitches = dict(pitches or {})
        assert set(pitches) <= {"h", "out", "go"}, pitches
        self.pitches, self.buffers = pitches, {}
        self.h = h = a["h"].to(dev)
        if "h" in pitches:
            self.h = h = pitched_input(h, pitches["h"])
        self.w, self.b = sd[C.W_KEY].to(dev).contiguous(), sd[C.B_KEY].to(dev)
        self.scales = _row_scales(g, scalers, {"log": a["avg_log"]}, dev)
        self.plan = plan = AG._SmallTrainPlan(g, F, N, S, dev)
        go = a["R"].to(dev)
        if "go" in pitches:
            go = pitched_input(go, pitches["go"])
        self.history = []
        for _ in range(repeat):
            bn = types.SimpleNamespace(weight=sd["batchnorm_h.weight"].to(dev), bias=sd["batchnorm_h.bias"].to(dev), eps=1e-5, momentum=0.1,
                                       running_mean=sd["batchnorm_h.running_mean"].to(dev).clone(),
                                       running_var=sd["batchnorm_h.running_var"].to(dev).clone())
            fbuf, ibuf = saved = plan.new_saved()
            plan.ws.fill_(float("nan"))                         # (the workspace needs no initialisation)
            out = torch.empty(V, N, device=dev)
            if "out" in pitches:
                out, self.buffers["out"] = pitched_output(V, N, pitches["out"], dev)
            args = plan.args(g, h, self.w, self.b, bn, self.scales, meta["residual"], saved)
            args.out, args.ld_out = out.data_ptr(), out.stride(0)
            self.args = args
            _lib.check(_lib.lib().pna_simple_train_fwd_f32(ctypes.byref(args), _lib.stream_ptr(dev)), "fwd")
            gh, gw, gv = torch.empty(V, F, device=dev), torch.empty(N, S * 4 * F, device=dev), torch.empty(3, N, device=dev)
            plan.ws.fill_(float("nan"))                         # (the backward reads nothing the forward left there)
            args.momentum = -1.0
            args.grad_out, args.ld_go = go.data_ptr(), go.stride(0)
            args.col_t, args.rank_t, args.items_t = plan.col_t.data_ptr(), plan.rank_t.data_ptr(), plan.items_t.data_ptr()
            args.n_items_t = plan.items_t.shape[0]
            args.grad_h, args.grad_w, args.grad_b, args.grad_gamma, args.grad_beta = (gh.data_ptr(), gw.data_ptr(), gv[0].data_ptr(),
                                                                                      gv[1].data_ptr(), gv[2].data_ptr())
            _lib.check(_lib.lib().pna_simple_train_bwd_f32(ctypes.byref(args), _lib.stream_ptr(dev)), "bwd")
            torch.cuda.synchronize(dev)
            self.bn, self.out, self.gh, self.gw, self.gv, self.go = bn, out, gh, gw, gv, go
            self.a = fbuf[:V * 4 * F].view(V, 4 * F)
            self.z = fbuf[V * 4 * F:V * 4 * F + V * N].view(V, N)
            self.stats = fbuf[V * 4 * F + V * N:].view(2, N)
            self.amx, self.amn = ibuf[0], ibuf[1]
            self.history.append([t.clone() for t in (out, self.a, self.z, self.stats, self.amx, self.amn, bn.running_mean, bn.running_var, gh, gw, gv)])


_runs = {}


def _run(name, dev):
    if name not in _runs:
        _runs[name] = _Run(name, dev)
    return _runs[name]


@pytest.mark.parametrize("name", CASES)
def test_saved_state_has_the_gather_kernels_bits(cuda_device, name):
    """a = [mean | max | min | std] and argmax / argmin equal pna_segreduce_fwd_f32's (want_arg) bit for bit on every row of in-degree
    <= 128 (a longer row is cut into segments there, reduced serially here: compared against float64 instead)."""
    r = _run(name, cuda_device)
    csr = r.g.csr
    F = r.meta["F"]
    ident, amx, amn = ops.segreduce(csr.rowptr, csr.col, r.h, F, C.AGGS, [None], tower_stride_in=F, want_arg=True,
                                    heavy=r.g.heavy_schedule(), workspace=r.g.workspace, items=r.g.work_items())
    deg = (csr.rowptr[1:] - csr.rowptr[:-1]).long()
    light = deg <= 128
    assert bool(light.any())
    assert torch.equal(r.a[light], ident[light])
    assert torch.equal(r.amx[light], amx[light, :F]) and torch.equal(r.amn[light], amn[light, :F])
    # the longer rows against float64.  Bars from fp32 arithmetic: a serial sum of D terms is off by at most D 2^-24 times the sum of the
    # terms' magnitudes, so mean by D 2^-24 mean|x|, E[x^2] and mean^2 by D 2^-24 E[x^2] each, std = sqrt(var + 1e-5) by half their sum
    # over std; max / min are exact
    heavy = (~light).cpu()
    if bool(heavy.any()):
        h64 = r.arrays["h"].double()
        src, dst = r.arrays["src"].long(), r.arrays["dst"].long()
        got, ref = r.a.double().cpu()[heavy], r.ref.a[heavy]
        for i, v in enumerate(torch.nonzero(heavy).flatten().tolist()):
            x = h64[src[dst == v]]
            D, u = x.shape[0], 2.0 ** -24
            tol_mean = 1e-5 * ref[i, :F].abs() + D * u * x.abs().mean(0)
            tol_std = 1e-5 * ref[i, 3 * F:] + D * u * (x * x).mean(0) / ref[i, 3 * F:]
            assert bool(((got[i, :F] - ref[i, :F]).abs() <= tol_mean).all()) and bool(((got[i, 3 * F:] - ref[i, 3 * F:]).abs() <= tol_std).all()), v
            assert torch.equal(got[i, F:3 * F], ref[i, F:3 * F]), v


@pytest.mark.parametrize("name", CASES)
def test_z_and_batch_statistics_against_float64(cuda_device, name):
    r = _run(name, cuda_device)
    ref = r.ref
    err = (r.z.double().cpu() - ref.z).abs()
    tol = 1e-5 * ref.z.abs() + 2e-6 * ref.mass                                          # the project's bar (bench.py)
    print(f"[small_train] z: max err / tol = {(err / tol).max().item():.3f}")
    assert bool((err <= tol).all()), (err / tol).max().item()
    torch.testing.assert_close(r.stats[0].double().cpu(), ref.mean, rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(r.stats[1].double().cpu(), ref.invstd, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(r.bn.running_mean.double().cpu(), ref.rm, rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(r.bn.running_var.double().cpu(), ref.rv, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(r.out.cpu(), ref.out.float(), rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("name", CASES)
def test_gradients_per_element_against_float64(cuda_device, name):
    r = _run(name, cuda_device)
    C.check_gradients(r.meta, r.arrays, r.ref, r.gh, {C.W_KEY: r.gw, C.B_KEY: r.gv[0], "batchnorm_h.weight": r.gv[1], "batchnorm_h.bias": r.gv[2]})


def test_rows_of_in_degree_one_and_the_arg_tie(cuda_device):
    """In-degree 1: std is exactly sqrt(1e-5) (var = E[x^2] - E[x]^2 = 0 exactly) and its gradient 0 -- node 30's only out-edge goes into
    such a row, so its gradient row is G_mean + G_max + G_min of that row and nothing else.  Two in-neighbours with identical rows: the
    earlier edge holds argmax and argmin."""
    r = _run("hand_nores", cuda_device)
    F = r.meta["F"]
    csr = r.g.csr
    rp = csr.rowptr.cpu()
    one = torch.sqrt(torch.tensor(1e-5, dtype=torch.float32))
    for v in range(1, 6):
        assert int(rp[v + 1] - rp[v]) == 1
        assert torch.equal(r.a[v, 3 * F:].cpu(), one.expand(F))
        assert torch.equal(r.amx[v].cpu(), torch.full((F,), int(rp[v]), dtype=torch.int32))
    assert int(rp[1] - rp[0]) == 0 and torch.equal(r.a[0].cpu(), torch.zeros(4 * F)) and bool((r.amx[0] == -1).all()) and bool((r.amn[0] == -1).all())
    first = int(rp[6])
    assert csr.col[first].item() == 7 and csr.col[first + 1].item() == 8
    assert bool((r.amx[6] == first).all()) and bool((r.amn[6] == first).all())
    # node 30 -> node 1 only: grad_h[30] = (G_mean + G_max + G_min)[1] in float64, the std block contributes 0
    ref = r.ref
    scalers = r.meta["scalers"].split()
    sd64 = {k: v.double() for k, v in r.sd.items() if v.is_floating_point()}
    pre = ref.pre
    gp = r.arrays["R"].double() * (pre > 0)
    xhat = (ref.z - ref.mean) * ref.invstd
    gz = sd64["batchnorm_h.weight"] * ref.invstd * (gp - gp.mean(0) - xhat * (gp * xhat).mean(0))
    import numpy as np
    lg = float(np.log(2.0))
    sc = {"identity": 1.0, "amplification": lg / float(r.arrays["avg_log"]), "attenuation": float(r.arrays["avg_log"]) / lg}
    G = sum(sc[s] * (gz[1] @ sd64[C.W_KEY][:, i * 4 * F:(i + 1) * 4 * F]) for i, s in enumerate(scalers))
    want = G[:F] + G[F:2 * F] + G[2 * F:3 * F]
    torch.testing.assert_close(r.gh[30].double().cpu(), want, rtol=1e-5, atol=2e-6 * float(ref.grad_h.abs().max()))
    torch.testing.assert_close(ref.grad_h[30], want, rtol=1e-9, atol=1e-12)               # (the oracle agrees: the std term is 0)


@pytest.mark.parametrize("name", ["hand_res", "hand_nores"])
def test_row_without_in_edges_matches_the_existing_route(cuda_device, name, monkeypatch):
    """Node 0 of the hand-made graph has no in-edges: z = bias there.  Its output row and the gradient rows it touches agree with the
    generic training route (AggregateFn / PosttransFn / BnTailFn) on the same inputs; the two routes' batch statistics differ by
    rounding, hence fp32-level bars, not bits."""
    monkeypatch.setattr(PF, "SMALL_TRAIN_ROWS", 0)
    r = _run(name, cuda_device)
    meta, a, sd = r.meta, r.arrays, r.sd
    layer = PNASimpleLayer(meta["F"], meta["out_dim"], meta["aggregators"], meta["scalers"], {"log": a["avg_log"]}, 0.0, True, meta["residual"])
    layer.load_state_dict(sd)
    layer = layer.to(cuda_device).train()
    h = a["h"].to(cuda_device).requires_grad_(True)
    out = layer(r.g, h)
    (out * a["R"].to(cuda_device)).sum().backward()
    torch.testing.assert_close(r.out[0], out[0].detach(), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(r.gh[0], h.grad[0], rtol=1e-5, atol=2e-6 * float(h.grad.abs().max()))


@pytest.mark.parametrize("name", ["simple_train_f20", "hand_res"])
def test_twenty_calls_give_identical_bits(cuda_device, name):
    r = _Run(name, cuda_device, repeat=20)
    for k, again in enumerate(r.history[1:]):
        for t0, t in zip(r.history[0], again):
            assert torch.equal(t0, t), k


def test_out_of_scope_arguments_are_refused(cuda_device):
    r = _run("hand_res", cuda_device)
    L = _lib.lib()
    st = _lib.stream_ptr(cuda_device)

    def variant(**kw):
        a = _lib.PnaSimpleTrainArgs()
        ctypes.memmove(ctypes.byref(a), ctypes.byref(r.args), ctypes.sizeof(a))
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    assert L.pna_simple_train_bwd_f32(ctypes.byref(variant()), st) == 0          # (the unchanged block is accepted)
    torch.cuda.synchronize(cuda_device)
    bad = [dict(F=3), dict(F=129), dict(N=0), dict(N=129), dict(n_scaler=0), dict(n_scaler=4), dict(V=1), dict(N=7, residual=1),
           dict(workspace_bytes=r.args.workspace_bytes - 4), dict(struct_size=ctypes.sizeof(_lib.PnaSimpleTrainArgs) - 8), dict(struct_size=0)]
    for kw in bad:
        for fn in (L.pna_simple_train_fwd_f32, L.pna_simple_train_bwd_f32):
            assert fn(ctypes.byref(variant(**kw)), st) == -1, kw
    assert L.pna_simple_train_bwd_f32(ctypes.byref(variant(n_items_t=r.args.n_items_t - 1)), st) == -1
    assert L.pna_simple_train_workspace_bytes(40, 100, 3, 8, 3) == -1
