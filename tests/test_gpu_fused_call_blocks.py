"""What the three drivers of the one-kernel layer (functional.FusedDegreeCall / FusedTowerCall / FusedMultiTowerCall) put into their
pna_fused_degree_args blocks: the number of launches and their order, every block's source slice, sizes, epilogue operands and
partial-sum chain, the tables the tile-order binding shares between the blocks, the warm-hit path of set_spare, the per-row factor that
must move with the rows of a balanced tile order -- and the output, against the two-kernel grouped path.

One small graph for all cases (V = 3000: eight degree groups = 52 tiles of 64 rows, 119 rest rows with isolated rows, rare degrees and one
hub row that the heavy schedule cuts into segments)."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

V = 3000
AGGS, SCALERS = "mean max min std", "identity amplification attenuation"
SHARED = ("tile_desc", "row_perm", "tile_counter", "guard_ws", "guard_ws_bytes", "spare_workgroups")
_EDGES = []


def _edges():
    if not _EDGES:
        rng = np.random.default_rng(7)
        src = rng.integers(0, V, 12000)
        dst = rng.integers(0, V, 12000)
        src = np.concatenate([src, rng.integers(0, V, 300)])
        dst = np.concatenate([dst, np.full(300, 1500)])
        _EDGES.append((torch.from_numpy(src), torch.from_numpy(dst)))
    return _EDGES[0]


def _graph(dev):
    """A fresh Graph object (and with it a fresh plan) over the module's edge list."""
    from pna_amd import Graph
    src, dst = _edges()
    return Graph(src.to(dev), dst.to(dev), V, [V // 2, V - V // 2])


@pytest.fixture(autouse=True)
def _knobs(monkeypatch):
    from pna_amd import degree_groups as DG, functional as PF
    for name, value in (("ENABLED", True), ("MIN_ROWS", 1), ("MIN_OUT", 1), ("FUSED", True)):
        monkeypatch.setattr(DG, name, value)
    monkeypatch.setattr(PF, "SMALL_TOWER_ROWS", 0)
    monkeypatch.setattr(PF, "SMALL_SIMPLE_ROWS", 0)


def _pitched(x, mult=8):
    P = (x.shape[1] + mult - 1) // mult * mult
    buf = torch.full((x.shape[0], P), float("nan"), dtype=x.dtype, device=x.device)
    buf[:, :x.shape[1]] = x
    return buf[:, :x.shape[1]]


def _check_plan(g):
    from pna_amd import degree_groups as DG
    plan = DG.plan_of(g)
    deg = g.in_degrees()[plan.rest_rows]
    assert plan.G >= 2 and plan.NR > 0 and plan.NV // 64 >= 7
    assert bool((deg == 0).any()) and bool((deg > g.heavy_schedule().threshold).any())
    return plan


def _ptr(t, byte_offset=0):
    return t.data_ptr() + byte_offset


def _blocks(call):
    """The argument blocks in launch order: `launch_order` where a call keeps one, else `panel_args`, else its one block."""
    order = getattr(call, "launch_order", None) or getattr(call, "panel_args", None)
    return [a for a, _ in order] if order else [call.args]


def _check_blocks(call, plan, expect):
    """`expect`: per block, in launch order, a dict of field -> value; pointer fields that must only be (non-)null are given as bool."""
    blocks = _blocks(call)
    assert len(blocks) == len(expect)
    n_rec = plan.fused_tables()[2]
    for i, (a, e) in enumerate(zip(blocks, expect)):
        assert (a.M, a.n_nodes, a.n_records) == (plan.NV, V, n_rec), i
        for name, want in e.items():
            got = getattr(a, name)
            if isinstance(want, bool):
                assert bool(got) == want, (i, name, got)
            elif isinstance(want, float):
                assert got == ctypes.c_float(want).value, (i, name, got, want)
            else:
                assert (got or 0) == want, (i, name, got, want)
        assert not a.pre_add or a.pre_add != a.y, i                        # (a launch never adds to the rows it reads)
    for prev, nxt in zip(blocks, blocks[1:]):
        if prev.relu == 0 and nxt.pre_add:                                   # the chain of partial sums
            assert nxt.pre_add == prev.y and nxt.ld_pre_add == prev.ldy


def _final(y, c0, ycw, relu, slope, bias, cs, ct, res, row_post):
    return dict(y=_ptr(y, 4 * c0), ldy=y.stride(0), relu=relu, act_slope=float(slope), y_cols_writable=ycw, bias=bias, col_scale=cs, col_shift=ct,
                residual=res, row_post=row_post)


def _partial(buf, c0, ycw):
    return dict(y=_ptr(buf, 4 * c0), ldy=buf.stride(0), relu=0, y_cols_writable=ycw, bias=False, col_scale=False, col_shift=False, residual=False,
                row_post=False)


def _check_binding(call):
    """The tables of the tile-order binding are shared by all blocks, whatever grid was bound last; a second binding of the same grid (the
    warm hit in front of every launch) changes no byte of any block."""
    from pna_amd import degree_groups as DG
    blocks = _blocks(call)

    def shared():
        first = [getattr(blocks[0], f) for f in SHARED]
        for a in blocks[1:]:
            assert [getattr(a, f) for f in SHARED] == first
        assert call.args.spare_workgroups == first[-1]
        return first[-1]
    shared()
    for on in (True, False):
        call.set_spare(on)
        assert shared() == (DG.FUSED_SPARE_WGS if on else 0)
        image = [bytes(a) for a in blocks]
        call.set_spare(on)
        assert [bytes(a) for a in blocks] == image
    assert all(a.tile_desc and a.row_perm for a in blocks)


def _check_output(call, y_ref):
    from pna_amd import functional as PF
    y = PF.run_fused_call(call).clone()
    assert torch.equal(PF.run_fused_call(call), y)
    assert torch.isfinite(y).all()
    # per element: 1e-5 relative + 2e-6 of the row's largest output (cancelling terms), as test_one_kernel_tower_layer_equals_two_kernel_grouped_path
    tol = 1e-5 * y_ref.abs() + 2e-6 * y_ref.abs().max(dim=1, keepdim=True).values + 1e-6
    err = (y - y_ref).abs()
    print(f"max err / tol = {float((err / tol).max()):.3f}, elements over = {int((err > tol).sum())}")
    assert not bool((err > tol).any()), (int((err > tol).sum()), float((err / tol).max()))


def _simple_layer(F, N, dev):
    from pna_amd.dgl.pna_layer import PNASimpleLayer
    torch.manual_seed(F + N)
    layer = PNASimpleLayer(F, N, AGGS, SCALERS, {"log": torch.tensor(1.6)}, 0.0, True, F == N)
    with torch.no_grad():
        for p in layer.parameters():
            p.copy_(torch.randn_like(p) / (p.shape[-1] ** 0.5 if p.dim() == 2 else 3.0))
        layer.batchnorm_h.running_mean.normal_()
        layer.batchnorm_h.running_var.uniform_(0.5, 2.0)
    return layer.to(dev).eval()


SIMPLE_SHAPES = {"one_launch": (75, 75), "column_panels": (75, 100), "feature_ranges": (90, 90)}


@pytest.mark.parametrize("kind,own_out", [("one_launch", False), ("one_launch", True), ("column_panels", False), ("feature_ranges", False)])
def test_simple_layer_call_blocks(cuda_device, kind, own_out):
    from pna_amd import degree_groups as DG, functional as PF
    F, N = SIMPLE_SHAPES[kind]
    g = _graph(cuda_device)
    plan = _check_plan(g)
    layer = _simple_layer(F, N, cuda_device)
    torch.manual_seed(1)
    h = torch.randn(V, F, device=cuda_device)
    panels = DG.fused_panels(F, N)
    assert panels is not None and DG.fused_applies(g, h, F, N)
    ranges = sorted({(f0, f1) for f0, f1, _, _ in panels})
    if kind == "one_launch":
        assert panels == [(0, F, 0, N)]
    elif kind == "column_panels":
        assert len(panels) > 1 and ranges == [(0, F)]
    else:
        assert len(ranges) == 2 and ranges[0][0] == 0 and ranges[1][1] == F
    out = torch.empty(V, N, device=cuda_device) if own_out else None
    with torch.no_grad():
        call = PF.FusedDegreeCall(layer, g, h, x=h, out=out)
        assert call.plan is plan and (call.y is out if own_out else call.y.shape == (V, N))
        has_res = bool(layer.residual)
        last_f0 = panels[-1][0]
        expect = []
        for f0, f1, c0, c1 in panels:
            e = dict(F=f1 - f0, N=c1 - c0, x=_ptr(h, 4 * f0), ldx=h.stride(0), x_rows=V)
            if f0 == last_f0:
                ycw = 0 if own_out else PF.own_buffer_cols(call.y.stride(0), c0, c1, N)
                e.update(_final(call.y, c0, ycw, 1, 0.0, True, True, True, has_res, False))
            else:
                e.update(_partial(call.part, c0, PF.own_buffer_cols(call.part.stride(0), c0, c1, N)))
            e["pre_add"] = _ptr(call.part, 4 * c0) if f0 else 0
            expect.append(e)
        assert (call.part is not None) == (len(ranges) == 2)
        _check_blocks(call, plan, expect)
        _check_binding(call)
        y_ref = PF.degree_grouped_posttrans(layer, g, h, PF.degree_grouped_aggregate(layer, g, h, plan), plan)    # the two-kernel path
        _check_output(call, y_ref)


def _tower_layer(in_dim, out, T, divide, gn, bn, dev):
    from pna_amd.dgl.pna_layer import PNALayer
    torch.manual_seed(in_dim + out + T)
    layer = PNALayer(in_dim, out, AGGS, SCALERS, {"log": torch.tensor(1.6)}, 0.0, gn, bn, towers=T, divide_input=divide,
                     residual=in_dim == out).to(dev).eval()
    with torch.no_grad():
        if bn:
            for t in layer.towers:
                t.batchnorm_h.running_mean.normal_()
                t.batchnorm_h.running_var.uniform_(0.5, 2.0)
    return layer


def _tower_inputs(layer, dev):
    """(h, snorm_n, projection table) as PNALayer.forward hands them to the one-kernel drivers."""
    from pna_amd import functional as PF, ops
    from pna_amd.dgl import pna_layer as PL
    towers = list(layer.towers)
    T, Fi = len(towers), towers[0].in_dim
    torch.manual_seed(2)
    h = _pitched(torch.randn(V, layer.in_dim, device=dev))
    snorm = torch.rand(V, 1, device=dev) + 0.5
    if T == 1:
        Wpad, bpad = PL._projection_cache_padded(towers[0], Fi, PF.tower_projection_pitch(Fi))
    elif layer.divide_input:
        Wpad, bpad = PL._projection_cache_padded_div(towers, Fi, PF.tower_projection_pitch(T * Fi))
    else:
        Wt, Wn = PL._projection_cache_padded_multi(towers, Fi, PF.tower_projection_pitch(Fi))
        return h, snorm, (ops.project(h, Fi, Wn) if ops.project_applies(h, Fi, Wn.shape[0]) else torch.mm(h, Wt))
    return h, snorm, PF.linear_act(h, Wpad, bpad)


def _two_kernel_tower(layer, g, h, snorm, monkeypatch):
    from pna_amd import degree_groups as DG, functional as PF
    with monkeypatch.context() as m:
        m.setattr(DG, "FUSED", False)
        assert not PF.tower_layer_degree_fused_applies(layer, g, h) and PF.tower_layer_degree_grouped_applies(layer, g, h)
        return layer(g, h, None, snorm)


@pytest.mark.parametrize("in_dim,out,T,divide,gn,bn", [(75, 75, 1, False, True, True), (64, 64, 4, True, False, True)])
def test_tower_call_blocks(cuda_device, monkeypatch, in_dim, out, T, divide, gn, bn):
    from pna_amd import functional as PF
    g = _graph(cuda_device)
    plan = _check_plan(g)
    layer = _tower_layer(in_dim, out, T, divide, gn, bn, cuda_device)
    with torch.no_grad():
        h, snorm, x_cat = _tower_inputs(layer, cuda_device)
        assert PF.tower_layer_degree_fused_applies(layer, g, h)
        call = PF.FusedTowerCall(layer, g, h, snorm, x_cat)
        Fe, P = in_dim, x_cat.shape[1] // 2
        slope = layer.mixing_network.activation.negative_slope
        e = dict(F=Fe, N=out, x=_ptr(x_cat), ldx=x_cat.stride(0), x_rows=V, x_dst=_ptr(x_cat, 4 * P), ld_xdst=x_cat.stride(0), h_self=_ptr(h),
                 ld_h=h.stride(0), pre_add=0)
        e.update(_final(call.y, 0, PF.own_buffer_cols(call.y.stride(0), 0, out, out), 2, slope, True, True, True, bool(layer.residual), True))
        assert call.plan is plan and call.y.shape == (V, out)
        _check_blocks(call, plan, [e])
        _check_binding(call)
        _check_output(call, _two_kernel_tower(layer, g, h, snorm, monkeypatch))


@pytest.mark.parametrize("in_dim,out,T,gn", [(64, 48, 3, True), (64, 64, 2, False)])
def test_multi_tower_call_blocks(cuda_device, monkeypatch, in_dim, out, T, gn):
    from pna_amd import functional as PF
    g = _graph(cuda_device)
    plan = _check_plan(g)
    layer = _tower_layer(in_dim, out, T, False, gn, True, cuda_device)
    with torch.no_grad():
        h, snorm, x_src = _tower_inputs(layer, cuda_device)
        assert PF.tower_layer_degree_fused_applies(layer, g, h)
        call = PF.FusedMultiTowerCall(layer, g, h, snorm, x_src)
        P = x_src.shape[1] // T
        slope = layer.mixing_network.activation.negative_slope
        bufs = (call.part, call.part2)                                      # the partial sums ping-pong: launch t reads bufs[t % 2]
        expect = []
        for t in range(T):
            e = dict(F=in_dim, N=out, x=_ptr(x_src, 4 * t * P), ldx=x_src.stride(0), x_rows=V, pre_add=_ptr(bufs[t % 2]),
                     ld_pre_add=bufs[t % 2].stride(0), x_dst=False, h_self=False)
            if t == T - 1:
                e.update(_final(call.y, 0, PF.own_buffer_cols(call.y.stride(0), 0, out, out), 2, slope, True, True, True, bool(layer.residual), True))
            else:
                dst = bufs[(t + 1) % 2]
                e.update(_partial(dst, 0, PF.own_buffer_cols(dst.stride(0), 0, out, out)))
            expect.append(e)
        assert call.plan is plan and call.y.shape == (V, out) and call.args is _blocks(call)[-1]
        _check_blocks(call, plan, expect)
        _check_binding(call)
        _check_output(call, _two_kernel_tower(layer, g, h, snorm, monkeypatch))


def test_balanced_order_moves_row_post_with_its_rows(cuda_device, monkeypatch):
    """A grid of 2 workgroups and a tail of 1 x 2 tiles: 52 tiles > 2 * (2 + 2), the dynamic schedule's list is a real permutation of the
    plan's tiles -- the graph norm's per-row factor has to follow it.  The same tiles in another order: identical bits."""
    from pna_amd import degree_groups as DG, functional as PF
    layer = _tower_layer(75, 75, 1, False, True, True, cuda_device)
    monkeypatch.setattr(PF, "_fused_grid", lambda device, spare, n_tiles64: 2)
    monkeypatch.setattr(DG, "FUSED_DYNAMIC_TAIL", 1)
    ys = {}
    with torch.no_grad():
        h, snorm, x_cat = _tower_inputs(layer, cuda_device)
        for balance in ("dynamic", "off"):
            monkeypatch.setattr(DG, "FUSED_BALANCE", balance)
            g = _graph(cuda_device)
            plan = _check_plan(g)
            call = PF.FusedTowerCall(layer, g, h, snorm, x_cat)
            if balance == "dynamic":
                order = plan.fused_balance(2)[2]
                assert not torch.equal(order, torch.arange(plan.NV // 64, device=order.device))
                assert call.args.tile_counter
            else:
                assert plan.fused_balance(2) is None and not call.args.tile_counter
            ys[balance] = PF.run_fused_call(call).clone()
    assert torch.equal(ys["dynamic"], ys["off"])
