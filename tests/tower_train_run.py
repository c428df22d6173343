"""The harness of the three tower training kernel test files (test_gpu_tower_train_kernels.py, test_gpu_tower_edge_train_kernels.py,
test_gpu_tower_drop_train_kernels.py): one forward + backward on a case's inputs through the C entry pair its shape and key select,
every output as a tensor.  A helper module like tower_train_cases, imported by the tests; it collects nothing itself."""
import ctypes

import torch

from pna_amd import _lib, autograd as AG
from pna_amd.dgl.pna_layer import _row_scales
from pna_amd.graph import Graph
from tower_train_cases import SLOPE

NAN = float("nan")
SENTINEL = 0x7FA5C3D1     # an fp32 NaN bit pattern no result takes (test_gpu_bf16_pyg_kernels.CANARY's idea)
OPERANDS = ("h", "out", "go", "e", "ge")     # the operands of the tower entries that carry a row pitch


def pitched_input(t, pitch):
    """t as the [:, :width] view of a (rows + 2, pitch) buffer: NaN in the padding columns and in one guard row each side."""
    buf = torch.full((t.shape[0] + 2, pitch), NAN, dtype=t.dtype, device=t.device)
    view = buf[1:-1, :t.shape[1]]
    view.copy_(t)
    return view


def pitched_output(rows, width, pitch, dev):
    """(view, buffer): the [:, :width] view of a (rows + 2, pitch) buffer, NaN in the view (the call has to write all of it), SENTINEL in
    the padding columns and in the guard row each side (the call may write none of it)."""
    buf = torch.full((rows + 2, pitch), SENTINEL, dtype=torch.int32, device=dev).view(torch.float32)
    view = buf[1:-1, :width]
    view.fill_(NAN)
    return view, buf


def padding_untouched(buf, width):
    """Whether everything of a pitched_output buffer outside its view still holds SENTINEL."""
    outside = torch.ones(buf.shape, dtype=torch.bool, device=buf.device)
    outside[1:-1, :width] = False
    return bool((buf.view(torch.int32)[outside] == SENTINEL).all())


class Run:
    """Forward + backward through the two C calls on `case` = (meta, arrays, state_dict, ref, ...) of one of the tower case modules:
    with dropout under `key` = (p, seed, offset) (pna_tower_drop_train_*), else with the case's edge features (pna_tower_edge_train_*),
    else pna_tower_train_*.  snorm: "case" = the case's factor, "ones" = a factor of ones, None = graph norm off.  want_grad_e False:
    grad_e = NULL.  `repeat` calls on the same plan, each from the case's running statistics: `history` holds every call's outputs,
    `everything` the last one's; the attributes are the last call's.  The workspace, the saved state, grad_e and the towers' gradient
    buffers are NaN-filled before the call that writes them: none needs an initialisation.  pitches: None = every operand contiguous; a
    dict {operand of OPERANDS: row pitch} = that operand is a pitched_input / pitched_output view (`buffers` keeps the outputs' whole
    buffers for padding_untouched)."""

    def __init__(self, name, case, dev, *, key=None, repeat=1, snorm="case", want_grad_e=True, pitches=None):
        meta, a, sd, ref = case[:4]
        self.name, self.meta, self.arrays, self.sd, self.ref, self.key = name, meta, a, sd, ref, key
        V, T, div, ed = meta["N"], meta["towers"], meta["divide_input"], meta["edge_dim"]
        Fi, Fo = (meta["in_dim"] // T if div else meta["in_dim"]), meta["out_dim"] // T
        scalers = meta["scalers"].split()
        S, Cc = len(scalers), T * Fo
        self.T, self.Fi, self.Fo, self.S, self.ed = T, Fi, Fo, S, ed
        self.g = g = Graph(a["src"], a["dst"], V).to(dev)
        pitches = dict(pitches or {})
        assert set(pitches) <= set(OPERANDS), pitches
        self.pitches, self.buffers = pitches, {}
        self.h = h = a["h"].to(dev)
        self.e = e = a["e"].to(dev)
        if "h" in pitches:
            self.h = h = pitched_input(h, pitches["h"])
        if "e" in pitches and ed:
            self.e = e = pitched_input(e, pitches["e"])
        sn = {"case": a["snorm_n"].reshape(-1).to(dev).contiguous(), "ones": torch.ones(V, device=dev), None: None}[snorm]
        self.scales = _row_scales(g, scalers, {"log": a["avg_log"]}, dev)
        dsd = {k: v.to(dev) for k, v in sd.items()}
        self.plan = plan = AG._TowerTrainPlan(g, T, Fi, Fo, S, div, dev, edge_dim=ed)
        go = a["R"].to(dev)
        if "go" in pitches:
            go = pitched_input(go, pitches["go"])
        L, st = _lib.lib(), _lib.stream_ptr(dev)
        names = [(f"towers.{t}.pretrans.fully_connected.0.linear.", f"towers.{t}.posttrans.fully_connected.0.linear.", f"towers.{t}.batchnorm_h.")
                 for t in range(T)]

        def call(which, base, edge):
            if key is not None:
                fn, block = f"pna_tower_drop_train_{which}_f32", AG._tower_drop_args(base, edge, key)
            elif ed:
                fn, block = f"pna_tower_edge_train_{which}_f32", edge
            else:
                fn, block = f"pna_tower_train_{which}_f32", base
            _lib.check(getattr(L, fn)(ctypes.byref(block), st), which)

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
            plan.ws.fill_(NAN)                                  # (the workspace needs no initialisation)
            out = torch.empty(V, Cc, device=dev)
            if "out" in pitches:
                out, self.buffers["out"] = pitched_output(V, Cc, pitches["out"], dev)
            args = plan.args(g, h, sn, self.scales, towers, dsd["mixing_network.linear.weight"], dsd["mixing_network.linear.bias"], SLOPE,
                             meta["residual"], saved)
            args.out, args.ld_out = out.data_ptr(), out.stride(0)
            call("fwd", args, plan.edge_args(args, e, saved) if ed else None)
            gh = torch.empty(V, meta["in_dim"], device=dev)
            ge = torch.full((e.shape[0], ed), NAN, device=dev) if (ed and want_grad_e) else None
            if ge is not None and "ge" in pitches:
                ge, self.buffers["ge"] = pitched_output(e.shape[0], ed, pitches["ge"], dev)
            grads, named = [], {}
            for pre, post, bn in names:
                gt = (torch.empty(Fi, 2 * Fi + ed, device=dev), torch.empty(Fi, device=dev), torch.empty(Fo, (1 + 4 * S) * Fi, device=dev),
                      torch.empty(Fo, device=dev), torch.empty(Fo, device=dev), torch.empty(Fo, device=dev))
                for x in gt:
                    x.fill_(NAN)
                grads.append(gt)
                named.update({pre + "weight": gt[0], pre + "bias": gt[1], post + "weight": gt[2], post + "bias": gt[3], bn + "weight": gt[4], bn + "bias": gt[5]})
            gmw, gmb = torch.empty(Cc, Cc, device=dev), torch.empty(Cc, device=dev)
            named.update({"mixing_network.linear.weight": gmw, "mixing_network.linear.bias": gmb})
            plan.ws.fill_(NAN)                                  # (the backward reads nothing the forward left there)
            plan.set_backward(args, go, gh, grads, gmw, gmb)
            qb = plan.edge_args(args, e, saved, grad_e=ge, backward=True) if ed else None
            self.args, self.q, self.keep = args, qb, (towers, grads, go, ge, args, qb)
            call("bwd", args, qb)
            torch.cuda.synchronize(dev)
            self.out, self.gh, self.ge, self.grads, self.running = out, gh, ge, named, running
            self.x_cat, self.a, self.z, self.p, self.stats, self.amx, self.amn = plan.views(saved)
            self.x_edge = plan.x_edge(saved) if ed else None
            self.everything = [t.clone() for t in [out, self.x_cat] + ([self.x_edge] if ed else []) + [self.a, self.z, self.p, self.stats, self.amx, self.amn, gh]
                               + ([ge] if ge is not None else []) + list(named.values()) + list(running.values())]
            self.history.append(self.everything)
