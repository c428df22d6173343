"""The harness of test_gpu_tower_aggr_train_kernels.py: one forward + backward on a case's inputs through pna_tower_aggr_train_*_f32
(or, for the bitwise comparisons on mean max min std, through the older entry pair the shape and key select), every output as a tensor.
A helper module like tower_train_run, imported by the tests; it collects nothing itself."""
import ctypes

import torch

from pna_amd import _lib, autograd as AG
from pna_amd.dgl.pna_layer import _row_scales
from pna_amd.graph import Graph
from tower_aggr_train_cases import SLOPE, codes_of
from tower_train_run import OPERANDS, pitched_input, pitched_output

NAN = float("nan")


class Run:
    """Forward + backward through the two C calls on `case` = (meta, arrays, state_dict, ref, key) of tower_aggr_train_cases.  old False:
    pna_tower_aggr_train_* with the case's list; old True (a case with mean max min std only): pna_tower_drop_train_* under a key, else
    pna_tower_edge_train_* with edge features, else pna_tower_train_*.  `repeat` calls on the same plan, each from the case's running
    statistics: `history` holds every call's outputs by name.  The workspace, the saved state, grad_e and the gradient buffers are
    NaN-filled before the call that writes them: none needs an initialisation.  tweak(which, base, edge, block): changes the argument
    blocks just before a call (the refusal tests); expect: the return code both calls must give.  pitches: None = every operand contiguous;
    a dict {operand of tower_train_run.OPERANDS: row pitch} = that operand is a tower_train_run.pitched_input / pitched_output view
    (`buffers` keeps the outputs' whole buffers)."""

    def __init__(self, case, dev, *, old=False, repeat=1, tweak=None, expect=0, pitches=None):
        meta, a, sd, ref, key = case
        self.meta, self.arrays, self.sd, self.ref, self.key = meta, a, sd, ref, key
        V, T, div, ed = meta["N"], meta["towers"], meta["divide_input"], meta["edge_dim"]
        Fi, Fo = (meta["in_dim"] // T if div else meta["in_dim"]), meta["out_dim"] // T
        scalers = meta["scalers"].split()
        S, Cc = len(scalers), T * Fo
        codes = codes_of(meta)
        A = len(codes)
        self.T, self.Fi, self.Fo, self.S, self.ed, self.A, self.codes = T, Fi, Fo, S, ed, A, codes
        self.g = g = Graph(a["src"], a["dst"], V).to(dev)
        h, e = a["h"].to(dev), a["e"].to(dev)
        pitches = dict(pitches or {})
        assert set(pitches) <= set(OPERANDS), pitches
        self.pitches, self.buffers = pitches, {}
        if "h" in pitches:
            h = pitched_input(h, pitches["h"])
        if "e" in pitches and ed:
            e = pitched_input(e, pitches["e"])
        sn = a["snorm_n"].reshape(-1).to(dev).contiguous()
        scales = _row_scales(g, scalers, {"log": a["avg_log"]}, dev)
        dsd = {k: v.to(dev) for k, v in sd.items()}
        self.plan = plan = AG._TowerTrainPlan(g, T, Fi, Fo, S, div, dev, edge_dim=ed, aggr=None if old else codes)
        go = a["R"].to(dev)
        if "go" in pitches:
            go = pitched_input(go, pitches["go"])
        L, st = _lib.lib(), _lib.stream_ptr(dev)
        names = [(f"towers.{t}.pretrans.fully_connected.0.linear.", f"towers.{t}.posttrans.fully_connected.0.linear.", f"towers.{t}.batchnorm_h.")
                 for t in range(T)]

        def call(which, base, edge, saved):
            if old:
                if key is not None:
                    fn, block = f"pna_tower_drop_train_{which}_f32", AG._tower_drop_args(base, edge, key)
                elif ed:
                    fn, block = f"pna_tower_edge_train_{which}_f32", edge
                else:
                    fn, block = f"pna_tower_train_{which}_f32", base
            else:
                fn, block = f"pna_tower_aggr_train_{which}_f32", plan.aggr_args(base, edge, key, saved, backward=which == "bwd")
            if tweak is not None:
                tweak(which, base, edge, block)
            rc = getattr(L, fn)(ctypes.byref(block), st)
            torch.cuda.synchronize(dev)
            assert rc == expect, (fn, rc, L.pna_last_error())

        self.history = []
        for _ in range(repeat):
            towers, running = [], {}
            for pre, post, bn in names:
                rm, rv = dsd[bn + "running_mean"].clone(), dsd[bn + "running_var"].clone()
                running[bn + "running_mean"], running[bn + "running_var"] = rm, rv
                towers.append((dsd[pre + "weight"], dsd[pre + "bias"], dsd[post + "weight"], dsd[post + "bias"], dsd[bn + "weight"], dsd[bn + "bias"],
                               rm, rv, 1e-5, 0.1))
            saved = plan.new_saved()
            saved[0].fill_(NAN)
            saved[1].fill_(-7)
            plan.ws.fill_(NAN)                                  # (the workspace needs no initialisation)
            out = torch.full((V, Cc), NAN, device=dev)
            if "out" in pitches:
                out, self.buffers["out"] = pitched_output(V, Cc, pitches["out"], dev)
            args = plan.args(g, h, sn, scales, towers, dsd["mixing_network.linear.weight"], dsd["mixing_network.linear.bias"], SLOPE, meta["residual"], saved)
            args.out, args.ld_out = out.data_ptr(), out.stride(0)
            call("fwd", args, plan.edge_args(args, e, saved) if ed else None, saved)
            gh = torch.full((V, meta["in_dim"]), NAN, device=dev)
            ge = torch.full((e.shape[0], ed), NAN, device=dev) if ed else None
            if ed and "ge" in pitches:
                ge, self.buffers["ge"] = pitched_output(e.shape[0], ed, pitches["ge"], dev)
            grads, named = [], {}
            for pre, post, bn in names:
                gt = (torch.empty(Fi, 2 * Fi + ed, device=dev), torch.empty(Fi, device=dev), torch.empty(Fo, (1 + A * S) * Fi, device=dev),
                      torch.empty(Fo, device=dev), torch.empty(Fo, device=dev), torch.empty(Fo, device=dev))
                for x in gt:
                    x.fill_(NAN)
                grads.append(gt)
                named.update({pre + "weight": gt[0], pre + "bias": gt[1], post + "weight": gt[2], post + "bias": gt[3], bn + "weight": gt[4], bn + "bias": gt[5]})
            gmw, gmb = torch.full((Cc, Cc), NAN, device=dev), torch.full((Cc,), NAN, device=dev)
            named.update({"mixing_network.linear.weight": gmw, "mixing_network.linear.bias": gmb})
            plan.ws.fill_(NAN)                                  # (the backward reads nothing the forward left there)
            plan.set_backward(args, go, gh, grads, gmw, gmb)
            qb = plan.edge_args(args, e, saved, grad_e=ge, backward=True) if ed else None
            self.keep, self.saved = (towers, grads, go, ge, args, qb), saved
            call("bwd", args, qb, saved)
            self.out, self.gh, self.ge, self.grads, self.running = out, gh, ge, named, running
            self.x_cat, self.a, self.z, self.p, self.stats, self.amx, self.amn = plan.views(saved)
            self.row_mean = plan.row_mean(saved) if not old else None
            fwd = {"out": out, "x_cat": self.x_cat, "a": self.a, "z": self.z, "p": self.p, "stats": self.stats, "amx": self.amx, "amn": self.amn}
            if ed:
                fwd["x_edge"] = plan.x_edge(saved)
            fwd.update({"run/" + k: v for k, v in running.items()})
            bwd = {"grad_h": gh}
            if ed:
                bwd["grad_e"] = ge
            bwd.update({"grad/" + k: v for k, v in named.items()})
            self.fwd, self.bwd = {k: v.clone() for k, v in fwd.items()}, {k: v.clone() for k, v in bwd.items()}
            self.history.append({**self.fwd, **self.bwd})
