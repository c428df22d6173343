"""Hand-built batches for the batch plan (pna_batch_plan_i32, graph.BATCH_PLAN_ROWS) and the reference every test compares with: the
route collate_flat takes with the knob off, then the lazy properties and autograd._transposed_whole_rows.  A case is a dict of host
int64 tensors `src`, `dst` (LOCAL ids, members one after the other) and lists `edge_counts`, `num_nodes`."""
import functools

import numpy as np
import torch

from pna_amd import autograd as AG
from pna_amd import graph as G
from pna_amd.graph import Graph


def _batch(members):
    """members: [(n_nodes, src, dst)] with local ids."""
    src = np.concatenate([np.asarray(s, dtype=np.int64).reshape(-1) for _, s, _ in members]) if members else np.zeros(0, np.int64)
    dst = np.concatenate([np.asarray(d, dtype=np.int64).reshape(-1) for _, _, d in members]) if members else np.zeros(0, np.int64)
    return dict(src=torch.from_numpy(src), dst=torch.from_numpy(dst), edge_counts=[len(np.asarray(s).reshape(-1)) for _, s, _ in members],
                num_nodes=[int(n) for n, _, _ in members])


def _empty(n):
    return (n, [], [])


def _ring(n):
    u = np.arange(n)
    return (n, np.concatenate([u, (u + 1) % n]), np.concatenate([(u + 1) % n, u]))


def _random(n, e, rng):
    return (n, rng.integers(0, n, e), rng.integers(0, n, e))


def _molecule(n, rng):
    """A random recursive tree + ~10 % ring-closing bonds, symmetrised, the edge order shuffled (pna_amd.synth.molecule_batch's member)."""
    u = np.arange(1, n)
    v = (rng.random(n - 1) * u).astype(np.int64)
    k = max(1, n // 10)
    ru, rv = rng.integers(0, n, k), rng.integers(0, n, k)
    keep = ru != rv
    a, b = np.concatenate([u, ru[keep]]), np.concatenate([v, rv[keep]])
    s, d = np.concatenate([a, b]), np.concatenate([b, a])
    order = rng.permutation(s.size)
    return (n, s[order], d[order])


def _in_star(deg):
    return (deg + 1, np.arange(1, deg + 1), np.zeros(deg, np.int64))


def _out_star(deg):
    return (deg + 1, np.zeros(deg, np.int64), np.arange(1, deg + 1))


def _interleaved():
    """Parallel edges and self-loops interleaved: only a stable order reproduces eid."""
    s = [0, 1, 0, 2, 1, 0, 1, 0, 1, 2, 2, 0, 1, 1, 0, 2, 0]
    d = [1, 1, 1, 1, 1, 1, 0, 0, 0, 2, 1, 1, 1, 0, 0, 2, 1]
    return (3, s, d)


def _sorted_member(rng, reverse):
    n, s, d = _random(40, 150, rng)
    order = np.argsort(d, kind="stable")
    if reverse:
        order = order[::-1]
    return (n, s[order], d[order])


def molecules(n_graphs, seed, lo=9, hi=38):
    rng = np.random.default_rng(seed)
    return _batch([_molecule(int(rng.integers(lo, hi + 1)), rng) for _ in range(n_graphs)])


def _build(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    lim_n, lim_e = G.batch_plan_limits()
    if name == "b1":
        return _batch([_molecule(7, rng)])
    if name == "empty_members":
        return _batch([_empty(3), _ring(4), _empty(2), _empty(1), _ring(5), _molecule(12, rng), _empty(4)])
    if name == "one_node_self_loop":
        return _batch([_ring(3), (1, [0], [0]), (1, [0, 0, 0], [0, 0, 0]), _ring(4)])
    if name == "interleaved":
        return _batch([_ring(3), _interleaved(), _interleaved(), _ring(5)])
    if name == "sorted_and_reversed":
        return _batch([_sorted_member(rng, False), _sorted_member(rng, True), _molecule(20, rng)])
    if name == "in_star_128":
        return _batch([_ring(4), _in_star(128), _ring(3)])
    if name == "in_star_129":
        return _batch([_ring(4), _in_star(129), _ring(3)])
    if name == "out_star_129":
        return _batch([_ring(4), _out_star(129), _ring(3)])
    if name == "at_max_member_nodes":
        return _batch([_molecule(11, rng), _random(lim_n, 3 * lim_n, rng), _molecule(9, rng)])
    if name == "at_max_member_edges":
        return _batch([_molecule(11, rng), _random(300, lim_e, rng), _molecule(9, rng)])
    if name == "molecules_300":
        return molecules(300, 5)
    if name == "alternating_1_200":
        return _batch([(1, [0], [0]) if i % 4 == 0 else _empty(1) if i % 2 == 0 else _random(200, 700, rng) for i in range(14)])
    raise KeyError(name)


NAMES = ["b1", "empty_members", "one_node_self_loop", "interleaved", "sorted_and_reversed", "in_star_128", "in_star_129", "out_star_129",
         "at_max_member_nodes", "at_max_member_edges", "molecules_300", "alternating_1_200"]


@functools.lru_cache(maxsize=None)
def case(name):
    return _build(name)


def unplanned(c, device):
    """collate_flat with the knob off, whatever it is set to."""
    keep, G.BATCH_PLAN_ROWS = G.BATCH_PLAN_ROWS, 0
    try:
        return Graph.collate_flat(c["src"], c["dst"], c["edge_counts"], c["num_nodes"], device=device)
    finally:
        G.BATCH_PLAN_ROWS = keep


def reference(c, device, avg_logs=()):
    """Every array of the plan from the route of today, on `device`: {name: tensor or int}.  Degree scalers (GPU only) for `avg_logs`."""
    keep, G.BATCH_PLAN_ROWS = G.BATCH_PLAN_ROWS, 0
    try:
        g = Graph.collate_flat(c["src"], c["dst"], c["edge_counts"], c["num_nodes"], device=device)
        csr = g.csr
        col_t, rank_t, items_t = AG._transposed_whole_rows(g)
        gT = g._pna_amd_transposed
        sizes = torch.tensor([0] + list(c["num_nodes"]), dtype=torch.int64)
        ref = dict(src=g.src, dst=g.dst, rowptr=csr.rowptr, col=csr.col, row=csr.row, eid64=csr.eid, eid=g.edge_ids32(), items=g.work_items(),
                   snorm_n=g.snorm_n().reshape(-1), readout_offsets=sizes.cumsum(0).to(torch.int32).to(g.device),
                   rowptr_t=gT.csr.rowptr, col_t=col_t, row_t=gT.csr.row, pos_t64=gT.csr.eid, pos_t=gT.csr.eid.to(torch.int32), rank_t=rank_t,
                   items_t=items_t, row64=gT.src, col64=gT.dst, max_in=csr.max_degree, max_out=gT.csr.max_degree, graph=g)
        for v in avg_logs:
            ref[("scalers", v)] = g.degree_scalers(v)
        return ref
    finally:
        G.BATCH_PLAN_ROWS = keep


def same(a, b):
    """Equality of two tensors down to the bits (floats compared as their int32 images, so that NaN payloads and -0 count)."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.is_floating_point():
        return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
    return torch.equal(a, b)
