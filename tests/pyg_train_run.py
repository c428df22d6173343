"""The harness of test_gpu_pyg_train_kernels.py: forward + backward on a case of pyg_train_cases through pna_pyg_conv_train_fwd_f32 /
pna_pyg_conv_train_bwd_f32 by ctypes, every output as a tensor.  A helper module like tower_aggr_train_run; it collects nothing."""
import ctypes

import torch

from pna_amd import _lib, autograd as AG
from pna_amd.graph import Graph
from pna_amd.pytorch_geometric.pna import _row_factors

NAN = float("nan")


class Run:
    """`repeat` forward + backward calls on `case` = (meta, arrays, state_dict, ref); `history` holds every call's outputs by name.  The
    workspace, the saved state and every output buffer are NaN-filled before the call that writes them.  tweak(which, base, edge, block,
    y): changes the argument blocks just before a call; expect: the return code both calls must give."""

    def __init__(self, case, dev, *, repeat=1, tweak=None, expect=0):
        meta, a, sd, ref = case
        self.meta, self.ref = meta, ref
        V, T, Fi, Fo, ed, div = meta["N"], meta["towers"], meta["F_in"], meta["F_out"], meta["edge_dim"], meta["divide_input"]
        S, A, Cc = len(meta["scalers"]), len(meta["aggregators"]), T * Fo
        codes = tuple(_lib.AGG_CODES[n] for n in meta["aggregators"])
        self.T, self.Fi, self.Fo, self.ed, self.A, self.S = T, Fi, Fo, ed, A, S
        self.g = g = Graph(a["edge_index"][0], a["edge_index"][1], V).to(dev)
        x, e, go = a["x"].to(dev), a["edge_attr"].to(dev), a["R"].to(dev)
        scales = _row_factors(g, meta["scalers"], meta["avg_deg"])[0]
        d = {k: v.to(dev) for k, v in sd.items()}
        params = []
        for t in range(T):
            params += [d[f"pre_nns.{t}.0.weight"], d[f"pre_nns.{t}.0.bias"], d[f"post_nns.{t}.0.weight"], d[f"post_nns.{t}.0.bias"]]
        pre = [params[4 * t:4 * t + 2] for t in range(T)]
        enc = (d["edge_encoder.weight"], d["edge_encoder.bias"]) if ed else None
        self.plan = plan = AG._TowerTrainPlan(g, T, Fi, Fo, S, div, dev, edge_dim=ed, aggr=codes, pyg=True)
        L, st = _lib.lib(), _lib.stream_ptr(dev)

        def call(which, base, edge, saved, grads=None):
            block = plan.aggr_args(base, edge, None, saved, backward=which == "bwd")
            y = AG._pyg_conv_args(plan, block, pre, enc, saved, grads=grads)
            if tweak is not None:
                tweak(which, base, edge, block, y)
            rc = getattr(L, f"pna_pyg_conv_train_{which}_f32")(ctypes.byref(y), st)
            torch.cuda.synchronize(dev)
            assert rc == expect, (which, rc, L.pna_last_error())

        full = lambda *s: torch.full(s, NAN, device=dev)      # noqa: E731
        self.history = []
        for _ in range(repeat):
            saved = plan.new_saved()
            saved[0].fill_(NAN)
            saved[1].fill_(-7)
            plan.ws.fill_(NAN)
            out = full(V, Cc)
            args = plan.args(g, x, None, scales, AG._pyg_towers(params, T), d["lin.weight"], d["lin.bias"], 1.0, False, saved)
            args.out, args.ld_out = out.data_ptr(), out.stride(0)
            call("fwd", args, plan.edge_args(args, e, saved) if ed else None, saved)
            gx, ge = full(V, meta["in_c"]), (full(e.shape[0], ed) if ed else None)
            named, base_grads, own = {}, [], []
            for t in range(T):
                gwp, gbp, gwo, gbo = full(Fi, (3 if ed else 2) * Fi), full(Fi), full(Fo, (1 + A * S) * Fi), full(Fo)
                named.update({f"pre_nns.{t}.0.weight": gwp, f"pre_nns.{t}.0.bias": gbp, f"post_nns.{t}.0.weight": gwo, f"post_nns.{t}.0.bias": gbo})
                base_grads.append((gwp, gbp, gwo, gbo, None, None))      # (the base's pretrans pointers are not read)
                own.append((gwp, gbp))
            gmw, gmb = full(Cc, Cc), full(Cc)
            named.update({"lin.weight": gmw, "lin.bias": gmb})
            genc = (full(Fi, ed), full(Fi)) if ed else None
            if ed:
                named.update({"edge_encoder.weight": genc[0], "edge_encoder.bias": genc[1]})
            plan.ws.fill_(NAN)                                  # (the backward reads nothing the forward left there)
            plan.set_backward(args, go, gx, base_grads, gmw, gmb)
            qb = plan.edge_args(args, e, saved, grad_e=ge, backward=True) if ed else None
            self.keep = (args, qb, params, go, e, x, scales)
            call("bwd", args, qb, saved, grads=(own, genc))
            self.out, self.gx, self.ge, self.grads, self.saved = out, gx, ge, named, saved
            self.x_cat, self.a, self.z, self.p, _, self.amx, self.amn = plan.views(saved)
            res = {"out": out, "x_cat": self.x_cat, "a": self.a, "z": self.z, "p": self.p, "packed": plan.packed(saved), "grad_x": gx}
            if ed:
                res["grad_e"] = ge
            res.update({"grad/" + k: v for k, v in named.items()})
            self.history.append({k: v.clone() for k, v in res.items()})
