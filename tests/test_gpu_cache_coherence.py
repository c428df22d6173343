"""Cache coherence of every forward path: a WARM layer whose state was changed the way torch changes state gives,
on its next call, bit for bit the output of a FRESH layer of the same constructor arguments loaded with the same state_dict, on the same
forced path.  Bit equality needs no tolerance (every path is run-to-run deterministic: test_gpu_determinism.py); two safeguards go with
it, per path: the CONTROL -- two independently built fresh layers give equal bits before any mutation -- and the ANCHOR -- after the last
mutation the fresh layer is held to float64 at the bar of the path's existing accuracy test (cache_probe.anchor_*), so that warm and fresh
cannot be equally wrong.  Each case asserts the path predicate and the cache tags the path fills, and prints both."""
import pytest
import torch

import cache_probe as CP
from cache_probe import AGG, BF, SCA

pytestmark = pytest.mark.gpu


def _mods():
    from pna_amd import degree_groups as DG, functional as PF
    return PF, DG


def _ops():
    from pna_amd import ops
    return ops


def _knobs(kind):
    """The module knobs that force a path (the ones the existing path tests use), as (module name, attribute) -> value."""
    small = {("PF", "SMALL_TOWER_ROWS"): 32768, ("PF", "SMALL_SIMPLE_ROWS"): 4096, ("PF", "BF16_SMALL_ROWS"): 1 << 20}
    large = {("PF", "SMALL_TOWER_ROWS"): 0, ("PF", "SMALL_SIMPLE_ROWS"): 0, ("PF", "BF16_SMALL_ROWS"): 0, ("DG", "MIN_ROWS"): 1, ("DG", "MIN_OUT"): 1}
    return {"small": small,
            "fused": {**large, ("DG", "ENABLED"): True, ("DG", "FUSED"): True},
            "grouped": {**large, ("DG", "ENABLED"): True, ("DG", "FUSED"): False},
            "ordinary": {**large, ("DG", "ENABLED"): False},
            # the bf16x3 contraction and the contraction-kernel projection, which graphs of >= 16384 rows take (ops.X3_MIN_ROWS)
            "ordinary_x3": {**large, ("DG", "ENABLED"): False, ("OPS", "X3_MIN_ROWS"): 1}}[kind]


def _set_knobs(monkeypatch, kind):
    PF, DG = _mods()
    for (mod, attr), value in _knobs(kind).items():
        monkeypatch.setattr({"PF": PF, "DG": DG, "OPS": _ops()}[mod], attr, value)


# ---- the paths ----------------------------------------------------------------------------------------------------------------
def _tower_cfg(in_dim, out_dim, towers, divide_input, residual=True, edge_dim=0, pretrans_layers=1):
    return dict(in_dim=in_dim, out_dim=out_dim, towers=towers, divide_input=divide_input, residual=residual and in_dim == out_dim,
                edge_dim=edge_dim, pretrans_layers=pretrans_layers, scalers=SCA, graph_norm=True, batch_norm=True)


# name -> (layer kind, knobs, constructor cfg, edge features (None | "types" | "rows"), graph kwargs, dtype, predicate names, tags)
PATHS = {
    # PNALayer, fp32
    "tower_small": ("tower", "small", _tower_cfg(30, 30, 5, True), None, {}, None, ["small"], ["_pna_amd_small", "_pna_amd_fold"]),
    "tower_small_etab": ("tower", "small", _tower_cfg(20, 20, 4, False, edge_dim=6), "types", {}, None, ["small", "etab"], ["_pna_amd_small", "_pna_amd_fold"]),
    "tower_fused_t1": ("tower", "fused", _tower_cfg(64, 64, 1, False), None, {}, None, ["grouped", "fused", "rest_rows"],
                       ["_pna_amd_proj_pad", "_pna_amd_collapsed", "_pna_amd_fused_img", "_pna_amd_degree_plan"]),
    "tower_fused_div": ("tower", "fused", _tower_cfg(64, 64, 4, True), None, {}, None, ["grouped", "fused", "rest_rows"],
                        ["_pna_amd_proj_pad_div", "_pna_amd_collapsed", "_pna_amd_flat", "_pna_amd_fused_img"]),
    "tower_fused_multi": ("tower", "fused", _tower_cfg(56, 56, 4, False), None, {}, None, ["grouped", "fused", "rest_rows"],
                          ["_pna_amd_proj_pad_multi", "_pna_amd_collapsed", "_pna_amd_pass_w", "_pna_amd_beta_pad"]),
    "tower_grouped": ("tower", "grouped", _tower_cfg(24, 24, 3, False), None, {}, None, ["grouped", "not_fused", "rest_rows"],
                      ["_pna_amd_proj", "_pna_amd_collapsed", "_pna_amd_group_img"]),
    "tower_grouped_div": ("tower", "grouped", _tower_cfg(24, 24, 3, True), None, {}, None, ["grouped", "not_fused", "rest_rows"],
                          ["_pna_amd_collapsed", "_pna_amd_group_img"]),
    "tower_ordinary": ("tower", "ordinary", _tower_cfg(24, 24, 3, False), None, {}, None, ["ordinary"],
                       ["_pna_amd_proj", "_pna_amd_bias_stack", "_pna_amd_cs_stack", "_pna_amd_ct_stack", "_pna_amd_fold", "_pna_amd_pack",
                        "_pna_amd_tower_pack", "_pna_amd_float"]),
    "tower_ordinary_x3": ("tower", "ordinary_x3", _tower_cfg(24, 24, 3, False), None, {}, None, ["ordinary", "x3"],
                          ["_pna_amd_proj", "_pna_amd_fold", "_pna_amd_pack_x3", "_pna_amd_tower_pack"]),
    "tower_ordinary_rows": ("tower", "ordinary", _tower_cfg(24, 24, 3, False, edge_dim=5), "rows", {}, None, ["ordinary", "no_etab"],
                            ["_pna_amd_fold", "_pna_amd_pack", "_pna_amd_tower_pack"]),
    "tower_ordinary_etab": ("tower", "ordinary", _tower_cfg(24, 24, 3, True, edge_dim=5), "types", {}, None, ["ordinary", "etab"],
                            ["_pna_amd_fold", "_pna_amd_pack", "_pna_amd_tower_pack"]),
    "tower_pretrans2": ("tower", "ordinary", _tower_cfg(16, 16, 2, False, pretrans_layers=2), None, {}, None, ["ordinary"], ["_pna_amd_fold"]),
    "tower_alone": ("pnatower", "ordinary", _tower_cfg(24, 24, 1, False), None, {}, None, ["not_bf16", "not_x3"],
                    ["_pna_amd_proj", "_pna_amd_fold", "_pna_amd_pack"]),
    # PNASimpleLayer, fp32
    "simple_small": ("simple", "small", dict(F=40, aggs=AGG), None, {}, None, ["small"], ["_pna_amd_small", "_pna_amd_fold"]),
    "simple_fused_f64": ("simple", "fused", dict(F=64, aggs=AGG), None, {}, None, ["grouped", "fused", "rest_rows"], ["_pna_amd_fused_img", "_pna_amd_fold"]),
    "simple_fused_f120": ("simple", "fused", dict(F=120, aggs=AGG), None, {}, None, ["grouped", "fused", "rest_rows"], ["_pna_amd_fused_img", "_pna_amd_fold"]),
    "simple_fused_aggs": ("simple", "fused", dict(F=48, aggs="mean sum max"), None, {}, None, ["grouped", "fused", "rest_rows"],
                          ["_pna_amd_fused_img", "_pna_amd_virtual"]),
    "simple_grouped": ("simple", "grouped", dict(F=48, aggs=AGG), None, {}, None, ["grouped", "not_fused", "rest_rows"], ["_pna_amd_group_img", "_pna_amd_fold"]),
    "simple_ordinary": ("simple", "ordinary", dict(F=48, aggs=AGG), None, {}, None, ["ordinary", "not_x3"],
                        ["_pna_amd_fold", "_pna_amd_pack", "_pna_amd_float"]),
    "simple_ordinary_x3": ("simple", "ordinary_x3", dict(F=48, aggs=AGG), None, {}, None, ["ordinary", "x3"], ["_pna_amd_fold", "_pna_amd_pack_x3"]),
    "simple_ordinary_aggs": ("simple", "ordinary", dict(F=48, aggs="mean sum max"), None, {}, None, ["ordinary"], ["_pna_amd_fold", "_pna_amd_pack"]),
    # bf16
    "bf16_tower_multi": ("tower", "ordinary", _tower_cfg(40, 40, 5, False), None, {}, BF, ["bf16", "not_bf16_small"],
                         ["_pna_amd_bf16_images", "_pna_amd_bf16_mix", "_pna_amd_fold_f32"]),
    "bf16_tower_small": ("tower", "small", _tower_cfg(40, 40, 5, False, edge_dim=6), "types", dict(hub=None), BF, ["bf16", "bf16_small"],
                         ["_pna_amd_bf16_small", "_pna_amd_fold_f32"]),
    "bf16_simple": ("simple", "small", dict(F=40, aggs=AGG), None, dict(hub=None), BF, ["bf16", "bf16_small"], ["_pna_amd_bf16_small", "_pna_amd_fold_f32"]),
    "bf16_simple_multi": ("simple", "ordinary", dict(F=40, aggs=AGG), None, {}, BF, ["bf16", "not_bf16_small"], ["_pna_amd_pack_bf16", "_pna_amd_fold_f32"]),
}


class Ctx:
    """One path on the device: its graph, inputs, layer builder and call."""

    def __init__(self, name, dev):
        self.name, self.dev = name, dev
        self.kind, self.knobs, self.cfg, self.edge, gk, self.dtype, self.preds, self.tags = PATHS[name]
        self.gk = gk
        self.g = self.new_graph()
        self.avg = CP.avg_of(self.g)
        if self.dtype is BF:
            self.avg = {"log": self.avg["log"].to(BF).float()}
        V, E = self.g.num_nodes, self.g.csr.col.numel()
        gen = torch.Generator().manual_seed(7)
        width = self.cfg["F"] if self.kind == "simple" else self.cfg["in_dim"]
        dt = self.dtype or torch.float32
        self.h = torch.randn(V, width, generator=gen).to(dt).to(dev)
        self.sn = (torch.rand(V, 1, generator=gen) + 0.5).to(dt).to(dev)
        self.e = None
        if self.edge is not None:
            ed = self.cfg["edge_dim"]
            self.type_rows = torch.randn(3, ed, generator=gen).to(dt).to(dev)
            self.types = torch.randint(0, 3, (E,), generator=gen).to(dev)
            self.e = self.type_rows[self.types].contiguous() if self.edge == "types" else torch.randn(E, ed, generator=gen).to(dt).to(dev)

    def new_graph(self):
        return CP.make_graph(seed=3, **self.gk).to(self.dev)

    def build(self, avg=None):
        """The layer on the host, fp32, eval, with non-trivial values (the same every time)."""
        from pna_amd.dgl.pna_layer import PNALayer, PNASimpleLayer, PNATower
        avg = self.avg if avg is None else avg
        c = self.cfg
        if self.kind == "simple":
            layer = PNASimpleLayer(c["F"], c["F"], c["aggs"], SCA, avg, 0.0, True, True)
        elif self.kind == "pnatower":
            layer = PNATower(c["in_dim"], c["out_dim"], 0.0, True, True, AGG.split(), SCA.split(), avg, 1, 1, False, 0)
        else:
            layer = PNALayer(c["in_dim"], c["out_dim"], AGG, c["scalers"], avg, 0.0, c["graph_norm"], c["batch_norm"], towers=c["towers"],
                             pretrans_layers=c["pretrans_layers"], divide_input=c["divide_input"], residual=c["residual"],
                             edge_features=c["edge_dim"] > 0, edge_dim=c["edge_dim"])
        return CP.randomise(layer.eval(), 11)

    def fresh_of(self, layer, avg=None):
        return CP.fresh_like(lambda: self.build(avg), layer, self.dev, self.dtype).eval()

    def run(self, layer, g=None, h=None, e=None, sn=None):
        g = self.g if g is None else g
        h = self.h if h is None else h
        if self.kind == "simple":
            return layer(g, h)
        return layer(g, h, self.e if e is None else e, self.sn if sn is None else sn)

    def predicates(self, layer):
        PF, DG = _mods()
        from pna_amd.dgl.pna_layer import _bf16_towers_path
        g, h, e = self.g, self.h, self.e
        plan = DG.plan_of(g)
        simple = self.kind == "simple"
        out = {}
        for p in self.preds:
            if p == "small":
                out[p] = layer._small_batch_path(g, h)
            elif p == "etab":
                out[p] = g.edge_type_table(e) is not None
            elif p == "no_etab":
                out[p] = g.edge_type_table(e) is None
            elif p == "grouped":
                out[p] = layer._degree_grouped_path(g, h) if simple else PF.tower_layer_degree_grouped_applies(layer, g, h)
            elif p == "fused":
                out[p] = (DG.fused_applies(g, h, layer.in_dim, layer.out_dim, tuple(layer.aggregators)) if simple
                          else PF.tower_layer_degree_fused_applies(layer, g, h))
            elif p == "not_fused":
                out[p] = not (DG.fused_applies(g, h, layer.in_dim, layer.out_dim, tuple(layer.aggregators)) if simple
                              else PF.tower_layer_degree_fused_applies(layer, g, h))
            elif p == "rest_rows":
                out[p] = plan.G > 0 and plan.NR > 0 and int((g.in_degrees() == 0).sum()) >= 3
            elif p == "ordinary":
                small = layer._small_batch_path(g, h)
                grouped = layer._degree_grouped_path(g, h) if simple else PF.tower_layer_degree_grouped_applies(layer, g, h)
                out[p] = not small and not grouped and not (layer._bf16_path(g, h) if simple else layer._bf16_path(g, h, e))
            elif p == "bf16":
                out[p] = layer._bf16_path(g, h) if simple else layer._bf16_path(g, h, e)
            elif p == "not_bf16":
                out[p] = not (layer._bf16_path(g, h) if simple else layer._bf16_path(g, h, e))
            elif p in ("x3", "not_x3"):                    # what ops.posttrans / posttrans_towers decide from (`auto`, <= 3 scalers)
                ops = _ops()
                out[p] = (ops.POSTTRANS_ARITH == "auto" and len(SCA.split()) <= 3 and h.shape[0] >= ops.X3_MIN_ROWS) == (p == "x3")
            elif p in ("bf16_small", "not_bf16_small"):
                if simple:
                    ok = PF.bf16_small_applies(g, h.shape[0], T=1, Fi=layer.in_dim, Fo=layer.out_dim, A=len(layer.aggregators), divide_input=False,
                                               posttrans_affine=True, no_self_panel=True)
                else:
                    t0 = layer.towers[0]
                    ok = PF.bf16_small_applies(g, h.shape[0], T=len(layer.towers), Fi=t0.in_dim, Fo=t0.out_dim, A=4, divide_input=layer.divide_input,
                                               posttrans_affine=True, edge_features=t0.edge_features,
                                               etab=None if e is None else g.edge_type_table(e), No=layer.out_dim)
                out[p] = ok == (p == "bf16_small")
        return out

    def anchor(self, layer, y):
        """The fresh layer's output against float64 at the bar of this path's existing accuracy test."""
        avg = float(self.avg["log"])
        if self.dtype is BF and self.kind == "simple":
            from test_gpu_bf16_simple_layer import assert_contract, reference
            ref, tol, _ = reference(layer, self.g.csr.col.long().cpu(), self.g.csr.row.long().cpu(), self.h.shape[0], self.h)
            assert_contract(y, ref, tol, self.name)
            return "bf16 contract of test_gpu_bf16_simple_layer.py"
        if self.dtype is BF:
            import bf16_tower_ref as B
            c = self.cfg
            cfg = dict(towers=c["towers"], divide_input=c["divide_input"], aggregators=AGG.split(), scalers=SCA.split(), graph_norm=True,
                       batch_norm=True, residual=c["residual"], edge_features=self.e is not None)
            sd = {k: (v.detach().float().cpu().double() if v.is_floating_point() else v.cpu()) for k, v in layer.state_dict().items()}
            src, dst = self.g.src.long().cpu(), self.g.dst.long().cpu()
            ref, emu, E = B.layer_models(sd, cfg, src, dst, self.h.shape[0], B.f64(self.h), None if self.e is None else B.f64(self.e), B.f64(self.sn), avg)
            rho_gpu, rho_emu = B.rho(B.f64(y), ref, E), B.rho(emu, ref, E)
            assert rho_gpu <= 2 * rho_emu, (rho_gpu, rho_emu)
            return f"rho_gpu {rho_gpu:.3f} <= 2 x rho_emu {rho_emu:.3f}"
        if self.kind == "simple":
            return f"row error {CP.anchor_simple(layer, self.g, self.h, y, avg):.2e} <= 2e-5"
        if self.kind == "pnatower":
            from oracle import torch_oracle as O
            sd = {"t." + k: v for k, v in CP._sd64(layer).items()}
            src, dst = self.g.csr.col.long().cpu(), self.g.csr.row.long().cpu()
            y64 = O.tower_forward(sd, "t", src, dst, self.h.shape[0], self.h.double().cpu(), None, self.sn.double().cpu(), AGG.split(), SCA.split(),
                                  torch.tensor(avg, dtype=torch.float64), True, True, False)
            return f"share {CP.anchor_tower_large(y, y64):.5f} >= 0.999"
        y64 = CP.tower_layer_f64(layer, self.g, self.h, self.e, self.sn, self.cfg, avg)
        if self.knobs == "small":
            return f"max error {CP.anchor_tower_small(y, y64):.2e} <= 2e-5"
        return f"share {CP.anchor_tower_large(y, y64):.5f} >= 0.999"


def _diff(a, b):
    return float((a.double() - b.double()).abs().max()) if a.shape == b.shape else float("nan")


class Probe:
    """The invariant, applied: `step(label, mutate)` runs the warm layer, mutates, runs it again and compares with a fresh layer."""

    def __init__(self, c, layer):
        self.c, self.layer, self.found = c, layer, []

    def step(self, label, mutate, observable=True, layer=None, fresh=None):
        c = self.c
        layer = self.layer if layer is None else layer
        before = c.run(layer)
        mutate()
        after = c.run(layer)
        want = c.run(c.fresh_of(layer)) if fresh is None else fresh()
        assert after.dtype == want.dtype and torch.equal(after, want), \
            f"{c.name} / {label}: the warm layer differs from a fresh one with the same state (max |diff| {_diff(after, want):.3e})"
        if observable:
            assert not torch.equal(before, after), f"{c.name} / {label}: the mutation did not change the output"
        return after


def _copy_checks(c, layer, how, label):
    """copy.deepcopy / torch.save + load of a WARM layer: both succeed, the copy computes what the original computes, shares no storage
    with it, and each follows its own later updates only."""
    y = c.run(layer)
    other = how(layer)
    for (n, a), (_, b) in zip(CP.state_tensors(layer), CP.state_tensors(other)):
        assert a.data_ptr() != b.data_ptr(), (label, n)
    assert torch.equal(c.run(other), y), f"{c.name} / {label}: the copy computes something else (max |diff| {_diff(c.run(other), y):.3e})"
    name, t = CP.state_tensors(other)[0]
    Probe(c, other).step(f"{label}: copy mutated ({name})", lambda: CP.perturb_(name, t))
    assert torch.equal(c.run(layer), y), f"{c.name} / {label}: mutating the copy changed the original"
    y_other = c.run(other)
    name, t = CP.state_tensors(layer)[-1]
    Probe(c, layer).step(f"{label}: original mutated ({name})", lambda: CP.perturb_(name, t))
    assert torch.equal(c.run(other), y_other), f"{c.name} / {label}: mutating the original changed the copy"


@pytest.mark.parametrize("name", list(PATHS))
def test_path_follows_every_state_change(monkeypatch, cuda_device, name):
    c = Ctx(name, cuda_device)
    _set_knobs(monkeypatch, c.knobs)
    fp32 = c.dtype is None
    with torch.no_grad():
        layer = c.fresh_of(c.build())
        y0 = c.run(layer)
        assert torch.equal(c.run(layer), y0) and torch.isfinite(y0.float()).all()          # warm: served twice, same bits
        preds = c.predicates(layer)
        tags = CP.warm_tags(layer, c.g, c.e, c.avg["log"])
        print(f"\n[{name}] path predicates {preds}\n[{name}] warm cache tags {sorted(tags)}")
        assert all(preds.values()), preds
        assert set(c.tags) <= tags, sorted(set(c.tags) - tags)
        # control: two independently built fresh layers give equal bits (and the warm layer's)
        f1, f2 = c.run(c.fresh_of(layer)), c.run(c.fresh_of(layer))
        control = torch.equal(f1, f2) and torch.equal(f1, y0)
        print(f"[{name}] control: two fresh layers bit-equal = {control}")
        assert control, (_diff(f1, f2), _diff(f1, y0))
        P = Probe(c, layer)
        # 1. every parameter and floating-point buffer, one at a time, in place (the way an optimizer writes)
        for k, (tname, t) in enumerate(CP.state_tensors(layer)):
            P.step(f"in place: {tname}", lambda: CP.perturb_(tname, t, k))
        # 2. load_state_dict: the whole state; then the pretrans tensors alone (strict=False)
        P.step("load_state_dict (full)", lambda: layer.load_state_dict(CP.perturbed_state(layer)))
        if c.kind != "simple":
            part = CP.perturbed_state(layer, only="pretrans")
            assert part and all("pretrans" in k for k in part)
            P.step("load_state_dict (pretrans only, strict=False)", lambda: layer.load_state_dict(part, strict=False))
        # 3. p.data = other: the version counter stays, the address moves
        for pname, p in layer.named_parameters():
            def swap(p=p):
                p.data = p.data.clone() * 0.75
            P.step(f"p.data = other: {pname}", swap)
        # 4. a real optimizer step (fp32: the bf16 layers are inference-only)
        if fp32:
            def adam_step():
                layer.train()
                with torch.enable_grad():
                    opt = torch.optim.Adam(layer.parameters(), lr=1e-2)
                    c.run(layer).square().mean().backward()
                    opt.step()
                layer.zero_grad(set_to_none=True)
                layer.eval()
            P.step("Adam step", adam_step)
        # 5. dtype and device round trips of the warm layer
        if fp32:
            P.step(".to(bfloat16).float()", lambda: layer.to(BF).float())
        P.step(".cpu().cuda()", lambda: layer.cpu().to(cuda_device), observable=False)
        # 6. copies of the warm layer
        _copy_checks(c, layer, CP.deep, "deepcopy")
        _copy_checks(c, layer, CP.roundtrip_save, "torch.save / torch.load")

        # 7. what the graph or the call owns: compared with a fresh layer over a FRESH graph and fresh tensors of the same values
        def fresh_call(**kw):
            def run():
                avg = {"log": c.avg["log"].clone()}
                return c.run(c.fresh_of(layer, avg), g=c.new_graph(), h=c.h.clone(), e=None if c.e is None else c.e.clone(), sn=c.sn.clone(), **kw)
            return run
        P.step("avg_d['log'] edited in place", lambda: c.avg["log"].mul_(1.25), fresh=fresh_call())
        if c.kind != "simple":
            P.step("snorm_n edited in place", lambda: c.sn.mul_(1.25), fresh=fresh_call())
        if c.e is not None:
            P.step("e edited in place", lambda: c.e.mul_(1.5), fresh=fresh_call())

            def new_e():
                perm = torch.tensor([1, 2, 0], device=cuda_device)
                c.e = (c.type_rows[perm[c.types]] if c.edge == "types" else c.e.flip(0)).contiguous()
            P.step("a new e of the same shape", new_e, fresh=fresh_call())
        # anchor: the fresh layer after the last mutation against float64
        last = c.fresh_of(layer)
        print(f"[{name}] anchor: {c.anchor(last, c.run(last))}")


def test_fused_simple_follows_its_weight(cuda_device):
    """ops.fused_simple keeps its packed weight on the weight tensor (`_pna_amd_fpack`).  No layer calls the op, but it is public: after
    an in-place write and after `w.data = other` a warm weight gives bit for bit what a never-seen tensor of the same values gives.
    Anchor: the two-kernel path at the bar of test_gpu_fused.py (2e-5 of the output scale; no hub rows here)."""
    from pna_amd import functional as PF, ops
    g = CP.make_graph(V=300, E=1500, seed=5, hub=None, isolated=(0, 299)).to(cuda_device)
    V, F, N, S = 300, 20, 24, 3
    gen = torch.Generator().manual_seed(2)
    x = torch.randn(V, F, generator=gen).to(cuda_device)
    w = (torch.randn(N, S * 4 * F, generator=gen) / (S * 4 * F) ** 0.5).to(cuda_device)
    b = torch.randn(N, generator=gen).to(cuda_device)
    scales = [None] + [(torch.rand(V, generator=gen) + 0.5).to(cuda_device) for _ in range(S - 1)]
    run = lambda w_: ops.fused_simple(g.csr.rowptr, g.csr.col, x, F, w_, scales, b, relu=True)      # noqa: E731
    y0 = run(w)
    assert torch.equal(run(w), y0) and "_pna_amd_fpack" in CP.warm_tags(w)
    assert torch.equal(run(w.clone()), y0)                               # control: a never-seen tensor, same values, same bits
    w.mul_(1.5)
    y1 = run(w)
    assert torch.equal(y1, run(w.clone())) and not torch.equal(y1, y0)
    w.data = w.data.clone() * 0.75                                       # same version counter, new address
    y2 = run(w)
    assert torch.equal(y2, run(w.clone())) and not torch.equal(y2, y1)
    want = ops.posttrans(PF.aggregate(g, x, F, AGG.split()), 4 * F, w.clone(), scales, b, relu=True)
    assert (y2 - want).abs().max().item() <= 2e-5 * max(1.0, want.abs().max().item())


# ---- front ends ---------------------------------------------------------------------------------------------------------------
TOL = dict(rtol=1e-5, atol=1e-5)                              # the bar of the front ends' and nets' golden tests (test_gpu_pyg.py, test_gpu_layers.py)


def _follow(run, layer, fresh_out, label, mutate, observable=True):
    """One step of the invariant for a module that is not a Ctx path: `fresh_out()` = the output of a fresh module with the same state."""
    before = run(layer)
    mutate()
    after = run(layer)
    want = fresh_out()
    assert torch.equal(after, want), f"{label}: the warm module differs from a fresh one with the same state (max |diff| {_diff(after, want):.3e})"
    if observable:
        assert not torch.equal(before, after), f"{label}: the mutation did not change the output"
    return after


def _pyg_names():
    from conftest import golden_names
    return golden_names("pyg_conv")


@pytest.mark.parametrize("name", _pyg_names())
def test_pyg_conv(cuda_device, name):
    """The PyG PNAConv: every state tensor in place, and the edge_index edited in place (the CSR is cached on the tensor per version)."""
    from conftest import load_golden
    from pna_amd.pytorch_geometric import PNAConv
    meta, a, sd = load_golden(name)

    def build():
        return PNAConv(meta["in_c"], meta["out_c"], meta["aggregators"], meta["scalers"], a["deg_hist"], edge_dim=meta["edge_dim"] or None,
                       towers=meta["towers"], pre_layers=meta["pre_layers"], post_layers=meta["post_layers"], divide_input=meta["divide_input"])
    layer = build()
    layer.load_state_dict(sd)
    layer = layer.to(cuda_device).eval()
    x, ei = a["x"].to(cuda_device), a["edge_index"].to(cuda_device)
    ea = a["edge_attr"].to(cuda_device) if meta["edge_dim"] else None
    run = lambda l, e_=None: l(x, ei if e_ is None else e_, ea)      # noqa: E731
    fresh = lambda e_=None: run(CP.fresh_like(build, layer, cuda_device).eval(), e_)      # noqa: E731
    with torch.no_grad():
        y0 = run(layer)
        assert torch.equal(run(layer), y0)
        tags = CP.warm_tags(layer, ei)
        print(f"\n[pyg {name}] warm cache tags {sorted(tags)}")
        assert "_pna_amd_graph" in tags
        control = torch.equal(fresh(), fresh()) and torch.equal(fresh(), y0)
        print(f"[pyg {name}] control: two fresh layers bit-equal = {control}")
        assert control
        for k, (tname, t) in enumerate(CP.state_tensors(layer)):
            _follow(run, layer, fresh, f"pyg {name} / in place: {tname}", lambda: CP.perturb_(tname, t, k))
        V = x.shape[0]
        keep = ei[:, 0].clone()

        def rewire():
            ei[0, 0] = (ei[0, 0] + 1) % V
            ei[1, 0] = (ei[1, 0] + 2) % V
        _follow(run, layer, lambda: fresh(ei.clone()), f"pyg {name} / edge_index edited in place", rewire)
        # anchor: the golden state and graph restored -- two more mutations -- against the reference's own output
        ei[:, 0] = keep
        y = _follow(run, layer, fresh, f"pyg {name} / load_state_dict (golden)", lambda: layer.load_state_dict(sd))
        torch.testing.assert_close(y.cpu(), a["out"], **TOL)


def _dense_names():
    from conftest import golden_names
    return golden_names("dense")


@pytest.mark.parametrize("name", _dense_names())
def test_dense_layer(cuda_device, name):
    """The dense pytorch/pna layer through sparsify: every state tensor in place, and the adjacency edited in place."""
    from conftest import load_golden
    from pna_amd.pytorch.pna.layer import PNALayer as DensePNALayer
    from test_gpu_layers import _assert_close_with_reference_floor, _dense_ref64
    meta, a, sd = load_golden(name)
    avg_d = {"log": a["avg_log"].to(cuda_device), "lin": a["avg_lin"].to(cuda_device)}

    def build():
        return DensePNALayer(meta["in_features"], meta["out_features"], meta["aggregators"], meta["scalers"], avg_d, towers=meta["towers"],
                             self_loop=meta["self_loop"], divide_input=meta["divide_input"], device=cuda_device)
    layer = build()
    layer.load_state_dict(sd)
    layer = layer.to(cuda_device).eval()
    x, adj = a["x"].to(cuda_device), a["adj"].to(cuda_device)
    run = lambda l, adj_=None: l(x, adj if adj_ is None else adj_)      # noqa: E731
    fresh = lambda adj_=None: run(CP.fresh_like(build, layer, cuda_device).eval(), adj_)      # noqa: E731
    with torch.no_grad():
        y0 = run(layer)
        assert torch.equal(run(layer), y0)
        tags = CP.warm_tags(layer, adj)
        print(f"\n[dense {name}] warm cache tags {sorted(tags)}")
        assert "_pna_amd_sparse" in tags
        control = torch.equal(fresh(), fresh()) and torch.equal(fresh(), y0)
        print(f"[dense {name}] control: two fresh layers bit-equal = {control}")
        assert control
        for k, (tname, t) in enumerate(CP.state_tensors(layer)):
            _follow(run, layer, fresh, f"dense {name} / in place: {tname}", lambda: CP.perturb_(tname, t, k))
        # an edge removed in place (a present one, so that no row loses its last neighbour by accident of the fixture: restored below)
        nz = torch.nonzero(adj)
        rows_with_two = ((adj != 0).sum(dim=-1) >= 2)[nz[:, 0], nz[:, 1]]
        assert bool(rows_with_two.any()), f"dense {name}: no row with two neighbours to cut an edge from"
        b, i, j = (int(v) for v in nz[rows_with_two][0])
        keep = adj[b, i, j].clone()

        def cut():
            adj[b, i, j] = 0.0
        _follow(run, layer, lambda: fresh(adj.clone()), f"dense {name} / adjacency edited in place", cut)
        adj[b, i, j] = keep
        y = _follow(run, layer, fresh, f"dense {name} / load_state_dict (golden)", lambda: layer.load_state_dict(sd))
        _assert_close_with_reference_floor(y.cpu(), a["out"], lambda x_, dt=torch.float64: _dense_ref64(meta, a, sd, x=x_, dtype=dt), x=a["x"])


# ---- nets ---------------------------------------------------------------------------------------------------------------------
NETS = ["net_zinc_sum_edgefeat", "net_hiv_readme", "net_superpixels_edgefeat_gru"]
# the weight-derived cache tags of the layers' forward paths: a warm net carries the folded eval BatchNorm of its layers (every fixture
# has batch_norm) -- `_pna_amd_fold` in fp32, `_pna_amd_fold_f32` in bf16 -- whichever of the layer paths above its sizes select
NET_TAGS = {"fp32": "_pna_amd_fold", "bf16": "_pna_amd_fold_f32"}


def _net(name):
    """(meta, arrays, golden state, builder of the fp32 net on the host, call) of a golden net fixture."""
    from conftest import load_golden
    from pna_amd.nets import PNANet, PNANetHIV, PNANetSuperpixels
    from test_gpu_layers import _superpixels_params
    from test_host_logic import _net_params
    meta, a, sd = load_golden(name)

    def build():
        if meta["kind"] == "net_hiv":
            return PNANetHIV(dict(hidden_dim=meta["hidden_dim"], out_dim=meta["out_dim"], in_feat_dropout=0.0, dropout=0.0, L=meta["L"],
                                  readout=meta["readout"], batch_norm=True, residual=True, aggregators=meta["aggregators"],
                                  scalers=meta["scalers"], avg_d={"log": a["avg_log"]}, posttrans_layers=1, device="cpu")).eval()
        if meta["kind"] == "net_superpixels":
            return PNANetSuperpixels(_superpixels_params(meta, a)).eval()
        return PNANet(_net_params(meta, a)).eval()

    def call(net, g, dev, dtype):
        cast = lambda t: t.to(dev) if dtype is None or not t.is_floating_point() else t.to(dtype).to(dev)      # noqa: E731
        if meta["kind"] == "net_hiv":
            return net(g, a["atoms"].to(dev))
        if meta["kind"] == "net_superpixels":
            return net(g, cast(a["x"]), cast(a["e"]), cast(a["snorm_n"]), None)
        return net(g, a["atoms"].to(dev), a["bonds"].to(dev), cast(a["snorm_n"]), None)
    return meta, a, sd, build, call


@pytest.mark.parametrize("dtype", [None, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", NETS)
def test_net_follows_its_state(cuda_device, name, dtype):
    """Whole nets: after an eval forward, the node and edge embeddings, one middle layer's pretrans bias (posttrans bias in the HIV net,
    which has no pretrans), the GRU and the readout MLP are perturbed in turn; every next eval forward equals a fresh net's.  Then one
    optimizer step (fp32).  Anchor: the golden state restored -- a load_state_dict on the warm net -- against the reference's own output
    (fp32), resp. bit-equal to a fresh net in the golden state, which test_gpu_bf16_tower_layers.py holds to its emulation bar (bf16)."""
    from pna_amd.graph import Graph
    meta, a, sd, build, call = _net(name)
    g = Graph(a["src"], a["dst"], meta["N"], meta["sizes"]).to(cuda_device)
    net = CP.fresh_like(build, build().eval(), cuda_device, dtype).eval()
    net.load_state_dict(sd)
    run = lambda n: call(n, g, cuda_device, dtype)      # noqa: E731
    fresh = lambda: run(CP.fresh_like(build, net, cuda_device, dtype).eval())      # noqa: E731
    with torch.no_grad():
        y0 = run(net)
        assert torch.equal(run(net), y0)
        tags = CP.warm_tags(net, g)
        print(f"\n[{name} {'bf16' if dtype else 'fp32'}] warm cache tags {sorted(tags)}")
        assert NET_TAGS["bf16" if dtype else "fp32"] in tags, sorted(tags)
        control = torch.equal(fresh(), fresh()) and torch.equal(fresh(), y0)
        print(f"[{name} {'bf16' if dtype else 'fp32'}] control: two fresh nets bit-equal = {control}")
        assert control
        names = [n for n, _ in CP.state_tensors(net)]
        mid = meta["L"] // 2
        groups = ["embedding_h.", "embedding_e.", f"layers.{mid}.towers.0.pretrans.fully_connected.0.linear.bias",
                  f"layers.{mid}.posttrans.fully_connected.0.linear.bias", "gru", "MLP_layer."]
        hits = {}
        for part in groups:
            # (from the golden state each time: perturbations that pile up push the output to magnitudes whose bf16 spacing hides a bias)
            _follow(run, net, fresh, f"{name} / load_state_dict (golden) before {part}", lambda: net.load_state_dict(sd), observable=False)
            for k, (tname, t) in enumerate(CP.state_tensors(net)):
                if part in tname:
                    _follow(run, net, fresh, f"{name} / in place: {tname}", lambda: CP.perturb_(tname, t, k))
                    hits[part] = hits.get(part, 0) + 1
        present = [part for part in groups if any(part in n for n in names)]
        print(f"[{name} {'bf16' if dtype else 'fp32'}] perturbed tensors per group {hits}")
        assert len(present) >= 3 and all(hits.get(part, 0) >= 1 for part in present), (present, hits)
        assert any("embedding_h." == part for part in present) and any("MLP_layer." == part for part in present), present
        assert any(part.startswith("layers.") for part in present), present
        if dtype is None:
            def adam_step():
                net.train()
                with torch.enable_grad():
                    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
                    run(net).square().mean().backward()
                    opt.step()
                net.zero_grad(set_to_none=True)
                net.eval()
            _follow(run, net, fresh, f"{name} / Adam step", adam_step)
        y = _follow(run, net, fresh, f"{name} / load_state_dict (golden)", lambda: net.load_state_dict(sd))
        if dtype is None:
            torch.testing.assert_close(y.cpu(), a["out"], **TOL)


# ---- training -----------------------------------------------------------------------------------------------------------------
def _train_step(layer, call, h, opt=None):
    """loss, parameter gradients and the gradient of the input h of one training step (and the optimizer step, when given)."""
    layer.zero_grad(set_to_none=True)
    h.grad = None
    out = call(layer)
    loss = (out * torch.linspace(0.5, 1.5, out.shape[1], device=out.device)).sum() / out.shape[0]
    loss.backward()
    grads = {n: p.grad.clone() for n, p in layer.named_parameters()}
    grads["(input h)"] = h.grad.clone()
    if opt is not None:
        opt.step()
    return loss.detach().clone(), grads


@pytest.mark.parametrize("kind", ["simple", "tower5"])
def test_second_training_step_equals_a_fresh_layers(cuda_device, monkeypatch, kind):
    """Two consecutive training steps on a warm layer over a graph large enough for autograd.py's cached operands (the packed posttrans
    weight, the transposed graph, the grouped dW plan): the loss and every parameter gradient of step 2 equal those of a fresh layer
    loaded with the state after step 1.  The control -- two fresh layers, same state, same step -- decides whether `equal` is bit equality;
    where it is not, the per-element bars of test_gpu_backward.py::test_simple_layer_training_step_in_degree_plan_order hold instead
    (loss 2e-6, gradients 5e-3 of the tensor's largest entry) and the observed run-to-run difference is printed."""
    from pna_amd import Graph
    from pna_amd.dgl.pna_layer import PNALayer, PNASimpleLayer
    from pna_amd.synth import powerlaw_graph
    PF, DG = _mods()
    monkeypatch.setattr(DG, "MIN_ROWS", 1)
    monkeypatch.setattr(DG, "MIN_OUT", 1)
    V, E, F = 40_000, 400_000, 75
    src, dst = powerlaw_graph(V, E, seed=17)
    keep = dst >= 50
    g = Graph(src[keep], dst[keep], V).to(cuda_device)
    avg = {"log": torch.log(g.in_degrees().float().cpu() + 1).mean()}

    def build():
        if kind == "simple":
            layer = PNASimpleLayer(F, F, AGG, SCA, avg, 0.0, True, True)
        else:
            layer = PNALayer(F, F, AGG, SCA, avg, 0.0, True, True, towers=5, divide_input=False, residual=True)
        return CP.randomise(layer, 5)
    # (h asks for its gradient, as the output of an earlier layer does: the pull over the transposed graph runs for both layers)
    h = torch.randn(V, F, generator=torch.Generator().manual_seed(1)).to(cuda_device).requires_grad_(True)
    sn = g.snorm_n()
    call = (lambda l: l(g, h)) if kind == "simple" else (lambda l: l(g, h, None, sn))
    layer = build().to(cuda_device)
    with torch.no_grad():
        layer.eval()
        call(layer), call(layer)                                          # warm on the inference path too
    layer.train()
    opt = torch.optim.Adam(layer.parameters(), lr=1e-3)
    _train_step(layer, call, h, opt)                                      # step 1
    on_layer, on_graph = CP.warm_tags(layer), CP.warm_tags(g)
    gT = g.__dict__.get("_pna_amd_transposed")
    on_gT = CP.warm_tags(gT)
    print(f"\n[train {kind}] warm cache tags after step 1: layer {sorted(on_layer)}, graph {sorted(on_graph)}, transposed graph {sorted(on_gT)}")
    # the sizes reach autograd.py's cached operands: a packed or grouped image of the posttrans weight, the transposed graph (the pull
    # of d h; its rank / position tables are topology), the degree plan the grouped dW kernel orders its rows by
    assert V >= _ops().X3_MIN_ROWS and on_layer & {"_pna_amd_pack_x3", "_pna_amd_pack", "_pna_amd_group_img"}, sorted(on_layer)
    assert {"_pna_amd_transposed", "_pna_amd_degree_plan"} <= on_graph, sorted(on_graph)
    assert gT is not None and gT.num_nodes == V
    from pna_amd import autograd as AG
    plan = DG.plan_of(g)
    assert AG.DW_KERNEL and AG.DW_GROUPED and V >= AG.DW_MIN_ROWS and plan.G > 0 and plan.NR <= DG.MAX_REST_FRACTION * V      # the grouped dW route
    state1 = {k: v.clone() for k, v in layer.state_dict().items()}
    loss2, grads2 = _train_step(layer, call, h)                            # step 2 of the warm layer (no update: the state stays comparable)

    def fresh_step():
        f = build().to(cuda_device)
        f.load_state_dict(state1)
        return _train_step(f.train(), call, h)
    (la, ga), (lb, gb) = fresh_step(), fresh_step()
    rel = lambda x, y: (x - y).abs().max().item() / max(1e-30, y.abs().max().item())      # noqa: E731
    bit = torch.equal(la, lb) and all(torch.equal(ga[n], gb[n]) for n in ga)
    print(f"[train {kind}] control: two fresh layers bit-equal = {bit}; run-to-run loss {rel(la, lb):.2e}, gradients "
          + ", ".join(f"{n} {rel(ga[n], gb[n]):.2e}" for n in ga if not torch.equal(ga[n], gb[n])))
    assert loss2.item() != 0.0 and all(torch.isfinite(v).all() for v in grads2.values())
    if bit:
        assert torch.equal(loss2, la), (loss2.item(), la.item())
        for n in grads2:
            assert torch.equal(grads2[n], ga[n]), (n, rel(grads2[n], ga[n]))
    else:
        assert rel(loss2, la) <= 2e-6, rel(loss2, la)
        for n in grads2:
            assert rel(grads2[n], ga[n]) <= 5e-3, (n, rel(grads2[n], ga[n]))
