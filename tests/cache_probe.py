"""Scaffolding of the cache-coherence tests (test_cache_coherence_host.py, test_gpu_cache_coherence.py).

Every fast path keeps operands derived from parameters, buffers or caller tensors -- packed weight images, collapsed weights, folded
BatchNorm constants, argument blocks -- under a `_pna_amd_*` tag on a module, a tensor or a graph; the weight-derived ones all behind
one helper and one key (pna_amd/_cache.py: memo, tensor_key), the topology and caller-tensor ones behind keys of their own.
The invariant the tests hold every such cache to:

    a WARM layer (served at least twice) whose state was changed in any way torch changes state gives, on its next call, bit for
    bit the output of a FRESH layer of the same constructor arguments loaded with the same state_dict.

This module holds what both test files share: the census of the tags, builders of small graphs / layers with non-trivial values,
the enumeration of a module's state tensors, the mutations, and the float64 anchors (the bars of the paths' existing accuracy tests).
"""
import copy
import io
import pathlib
import re

import numpy as np
import torch

AGG, SCA = "mean max min std", "identity amplification attenuation"
BF = torch.bfloat16
TAG_RE = re.compile(r"_pna_amd_\w+")
ROOT = pathlib.Path(__file__).resolve().parent.parent

HOST, GPU = "test_cache_coherence_host.py", "test_gpu_cache_coherence.py"

# ---- the census ---------------------------------------------------------------------------------------------------------------
# tag -> (kind, where, note).  kind "host": a case of test_cache_coherence_host.py compares the cached operands element for element;
# "gpu": a path of test_gpu_cache_coherence.py fills the tag (asserted or printed after its warm-up) and compares outputs bit for bit;
# "exempt": the builder reads NO parameter, buffer or caller tensor VALUE (asserted by review; the reason stands next to the entry).
# test_cache_coherence_host.py::test_census_names_every_cache_tag fails for a tag in the sources that is missing here.
CENSUS = {
    # dgl/pna_layer.py
    "_pna_amd_graph": ("host", f"{HOST}::test_graph_of_follows_edge_index_edits; {GPU}::test_pyg_conv", "CSR of a PyG edge_index / a DGL graph"),
    "_pna_amd_float": ("host", f"{HOST}::test_avg_log_value_follows_the_tensor; {GPU} avg_d mutation of every path", "avg_d['log'] as a float"),
    "_pna_amd_proj": ("host", f"{HOST}::test_projection_caches; {GPU} paths tower_grouped, tower_ordinary", "[W_a ; W_b] of all towers"),
    "_pna_amd_proj_pad": ("host", f"{HOST}::test_projection_caches; {GPU} path tower_fused_t1", "padded projection of one tower"),
    "_pna_amd_proj_pad_div": ("host", f"{HOST}::test_projection_caches; {GPU} path tower_fused_div", "block-diagonal padded projection"),
    "_pna_amd_proj_pad_multi": ("host", f"{HOST}::test_projection_caches; {GPU} path tower_fused_multi", "source half, T towers over the whole input"),
    "_pna_amd_small": ("gpu", f"{GPU} paths tower_small, tower_small_etab, simple_small; {HOST}::test_warm_layer_copies_without_its_plan",
                       "the fp32 one-call plans (_SmallTowerPlan / _SmallSimplePlan)"),
    "_pna_amd_small_ok": ("exempt", "", "booleans of the layer's STRUCTURE (layer counts, aggregator names, widths): reads no tensor value"),
    # functional.py, ops.py
    "_pna_amd_answer": ("exempt", "", "the library's tile bytes for one tuple of shape integers (functional.small_tower_fits, "
                        "ops.tower_layer_bf16_lds_bytes; tests/test_lds_queries_host.py sweeps shapes through it): reads no tensor value"),
    # functional.py
    "_pna_amd_fold": ("host", f"{HOST}::test_fold_batchnorm_follows_its_tensors; {GPU} every fp32 path with BatchNorm", "eval BatchNorm as scale / shift"),
    "_pna_amd_fold_f32": ("host", f"{HOST}::test_fold_batchnorm_follows_its_tensors; {GPU} bf16 paths", "the same, folded in fp32 from bf16 tensors"),
    "_pna_amd_bias_stack": ("host", f"{HOST}::test_stack_cached_follows_its_tensors; {GPU} path tower_ordinary", "stacked posttrans biases"),
    "_pna_amd_cs_stack": ("host", f"{HOST}::test_stack_cached_follows_its_tensors; {GPU} path tower_ordinary", "stacked BatchNorm scales"),
    "_pna_amd_ct_stack": ("host", f"{HOST}::test_stack_cached_follows_its_tensors; {GPU} path tower_ordinary", "stacked BatchNorm shifts"),
    "_pna_amd_collapsed": ("host", f"{HOST}::test_tower_collapsed_flat_and_pass_weights; {GPU} tower_fused_* / tower_grouped* paths", "posttrans . BatchNorm . mixing"),
    "_pna_amd_flat": ("host", f"{HOST}::test_tower_collapsed_flat_and_pass_weights; {GPU} path tower_fused_div", "column permutation of the collapsed weight"),
    "_pna_amd_pass_w": ("host", f"{HOST}::test_tower_pass_weights_follow_the_pretrans_tensors (ADVICE r6 item 1); {GPU} path tower_fused_multi",
                        "per-tower cuts + the dense term of FusedMultiTowerCall"),
    "_pna_amd_beta_pad": ("gpu", f"{GPU} path tower_fused_multi", "beta of _pna_amd_pass_w padded to the output pitch: keyed on the beta object"),
    "_pna_amd_bf16_images": ("gpu", f"{GPU} path bf16_tower_multi", "bf16 contraction images of the multi-launch tower layer"),
    "_pna_amd_bf16_small": ("gpu", f"{GPU} paths bf16_tower_small, bf16_simple", "images of pna_tower_layer_bf16"),
    "_pna_amd_bf16_mix": ("gpu", f"{GPU} path bf16_tower_multi", "bf16 image of the mixing weight"),
    # ops.py
    "_pna_amd_pack": ("gpu", f"{GPU} paths simple_ordinary, tower_ordinary", "packed posttrans weight (exact f32 kernel)"),
    "_pna_amd_pack_x3": ("gpu", f"{GPU} paths simple_ordinary_x3, tower_ordinary_x3", "bf16x3 image of a posttrans weight (what large graphs use)"),
    "_pna_amd_fpack": ("gpu", f"{GPU}::test_fused_simple_follows_its_weight", "packed weight of ops.fused_simple (no layer calls it: the op is public)"),
    "_pna_amd_tower_pack": ("gpu", f"{GPU} paths tower_ordinary, tower_ordinary_x3", "all towers' posttrans weights in one image"),
    "_pna_amd_pack_bf16": ("gpu", f"{GPU} path bf16_simple_multi", "bf16 image of the simple layer's posttrans weight"),
    # degree_groups.py
    "_pna_amd_group_img": ("gpu", f"{GPU} paths simple_grouped, tower_grouped*", "combined images W_D of the two-kernel grouped path"),
    "_pna_amd_fused_img": ("gpu", f"{GPU} paths simple_fused_*, tower_fused_*", "W_D images of the one-kernel layers"),
    "_pna_amd_virtual": ("gpu", f"{GPU} path simple_fused_aggs", "posttrans weight re-expressed over the four standard statistics"),
    "_pna_amd_degree_plan": ("exempt", "", "topology only: rows ordered by in-degree (reads the CSR's rowptr, no feature or weight)"),
    # autograd.py
    "_pna_amd_edge_rows": ("exempt", "", "an uninitialised scratch buffer sized from (E, V, F): every use writes it before reading it"),
    "_pna_amd_transposed": ("exempt", "", "topology only: the graph with its edges reversed"),
    "_pna_amd_rank_t": ("exempt", "", "topology only: rank of each edge inside its transposed row"),
    "_pna_amd_pos_t": ("exempt", "", "topology only: position of every transposed edge in the forward CSR"),
    # pytorch/pna/sparsify.py
    "_pna_amd_sparse": ("host", f"{HOST}::test_sparsify_follows_adjacency_edits; {GPU}::test_dense_layer", "CSR pair of a dense adjacency"),
}


# tag -> the paths of test_gpu_cache_coherence.PATHS whose asserted tag list holds it, or the name of the GPU case that asserts it.  Every
# census row that names the GPU file has an entry here, and test_census_names_every_cache_tag checks each entry against PATHS / the file.
CENSUS_GPU = {
    "_pna_amd_graph": "test_pyg_conv",
    "_pna_amd_float": ["tower_ordinary", "simple_ordinary"],
    "_pna_amd_proj": ["tower_grouped", "tower_ordinary"],
    "_pna_amd_proj_pad": ["tower_fused_t1"],
    "_pna_amd_proj_pad_div": ["tower_fused_div"],
    "_pna_amd_proj_pad_multi": ["tower_fused_multi"],
    "_pna_amd_small": ["tower_small", "tower_small_etab", "simple_small"],
    "_pna_amd_fold": ["tower_small", "tower_ordinary", "simple_ordinary", "simple_grouped"],
    "_pna_amd_fold_f32": ["bf16_tower_multi", "bf16_tower_small", "bf16_simple", "bf16_simple_multi"],
    "_pna_amd_bias_stack": ["tower_ordinary"],
    "_pna_amd_cs_stack": ["tower_ordinary"],
    "_pna_amd_ct_stack": ["tower_ordinary"],
    "_pna_amd_collapsed": ["tower_fused_t1", "tower_fused_div", "tower_fused_multi", "tower_grouped", "tower_grouped_div"],
    "_pna_amd_flat": ["tower_fused_div"],
    "_pna_amd_pass_w": ["tower_fused_multi"],
    "_pna_amd_beta_pad": ["tower_fused_multi"],
    "_pna_amd_bf16_images": ["bf16_tower_multi"],
    "_pna_amd_bf16_small": ["bf16_tower_small", "bf16_simple"],
    "_pna_amd_bf16_mix": ["bf16_tower_multi"],
    "_pna_amd_pack": ["simple_ordinary", "tower_ordinary"],
    "_pna_amd_pack_x3": ["simple_ordinary_x3", "tower_ordinary_x3"],
    "_pna_amd_fpack": "test_fused_simple_follows_its_weight",
    "_pna_amd_tower_pack": ["tower_ordinary", "tower_ordinary_x3"],
    "_pna_amd_pack_bf16": ["bf16_simple_multi"],
    "_pna_amd_group_img": ["simple_grouped", "tower_grouped", "tower_grouped_div"],
    "_pna_amd_fused_img": ["simple_fused_f64", "simple_fused_f120", "simple_fused_aggs", "tower_fused_t1", "tower_fused_div"],
    "_pna_amd_virtual": ["simple_fused_aggs"],
    "_pna_amd_sparse": "test_dense_layer",
}


def source_tags():
    """Every `_pna_amd_*` tag in the Python sources of the package -> {tag: [files]}."""
    out = {}
    for p in sorted((ROOT / "pna_amd").rglob("*.py")):
        for tag in set(TAG_RE.findall(p.read_text())):
            out.setdefault(tag, []).append(str(p.relative_to(ROOT)))
    return out


# ---- graphs, layers, state ----------------------------------------------------------------------------------------------------
def make_graph(V=1400, E=4200, seed=0, hub=(700, 300), isolated=(0, 17, 1399)):
    """A small graph with what the paths branch on: degree values that fill 128-row tiles (groups), rare degrees and -- with `hub` =
    (row, in-edges) -- a hub row beyond the heavy threshold (rest rows), rows without in-edges (`isolated`), two member graphs."""
    from pna_amd import Graph
    rng = np.random.default_rng(seed)
    src, dst = rng.integers(0, V, E), rng.integers(0, V, E)
    if hub is not None:
        src = np.concatenate([src, rng.integers(0, V, hub[1])])
        dst = np.concatenate([dst, np.full(hub[1], hub[0])])
    keep = ~np.isin(dst, np.asarray(isolated, dtype=np.int64))
    return Graph(torch.from_numpy(src[keep]), torch.from_numpy(dst[keep]), V, [V // 2, V - V // 2])


def avg_of(graph):
    return {"log": torch.log(graph.in_degrees().double().cpu() + 1).mean().float()}


def randomise(module, seed):
    """Non-trivial values for every parameter and BatchNorm statistic (defaults leave biases near 0 and the statistics at 0 / 1)."""
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in module.named_parameters():
            if p.dim() == 2 and "embedding" not in n:
                p.copy_(torch.randn(p.shape, generator=gen) / p.shape[-1] ** 0.5)
            elif p.dim() == 1:
                p.copy_(torch.randn(p.shape, generator=gen) / 3.0 + (1.0 if "batchnorm" in n and n.endswith("weight") else 0.0))
        for n, b in module.named_buffers():
            if n.endswith("running_mean"):
                b.copy_(torch.randn(b.shape, generator=gen) * 0.2)
            elif n.endswith("running_var"):
                b.copy_(torch.rand(b.shape, generator=gen) + 0.5)
    return module


def state_tensors(module):
    """[(name, tensor)]: every parameter and every floating-point buffer -- what a cache can be stale against."""
    return list(module.named_parameters()) + [(n, b) for n, b in module.named_buffers() if b.is_floating_point()]


def perturb_(name, t, k=0):
    """An optimizer-style in-place write (bumps the version counter, keeps the address): alternately a scaling and a shift."""
    with torch.no_grad():
        if name.endswith("running_var") or k % 2 == 0:
            t.mul_(1.5)
        else:
            t.add_(0.25)


def perturbed_state(module, only=None, factor=1.25):
    sd = {k: v.clone() for k, v in module.state_dict().items()}
    out = {}
    for k, v in sd.items():
        if v.is_floating_point() and (only is None or only in k):
            out[k] = v * factor + (0.0 if k.endswith("running_var") else 0.0625)
        elif only is None:
            out[k] = v
    return out


def fresh_like(build, module, device=None, dtype=None):
    """A layer of the same constructor arguments that never ran, holding `module`'s state."""
    fresh = build()
    if device is not None:
        fresh = fresh.to(device)
    if dtype is not None:
        fresh = fresh.to(dtype)
    fresh.load_state_dict(module.state_dict())
    return fresh.train(module.training)


def warm_tags(*owners):
    """The `_pna_amd_*` tags present on the given modules (their submodules, parameters and buffers included), graphs or tensors."""
    found = set()

    def scan(obj):
        d = getattr(obj, "__dict__", None)
        if d:
            found.update(k for k in d if isinstance(k, str) and k.startswith("_pna_amd_"))

    def walk(entry):                                                 # (key, value, tensors): values are tensors or nests of them
        for x in entry:
            if torch.is_tensor(x):
                scan(x)
            elif isinstance(x, (list, tuple)):
                walk(x)
    for o in owners:
        if isinstance(o, torch.nn.Module):
            for m in o.modules():
                scan(m)
                for t in list(m._parameters.values()) + list(m._buffers.values()):
                    if t is not None:
                        scan(t)
                for v in list(m.__dict__.values()):                  # tensors held by a cache entry carry caches of their own (Wv)
                    if isinstance(v, tuple):
                        walk(v)
        elif o is not None:
            scan(o)
    return found


def roundtrip_save(module):
    buf = io.BytesIO()
    torch.save(module, buf)
    buf.seek(0)
    return torch.load(buf, weights_only=False)


def deep(module):
    return copy.deepcopy(module)


# ---- float64 anchors (the bars are those of each path's existing accuracy test) -----------------------------------------------
def _sd64(module):
    return {k: (v.detach().double().cpu() if v.is_floating_point() else v.cpu()) for k, v in module.state_dict().items()}


def tower_layer_f64(layer, graph, h, e, snorm, cfg, avg_log):
    """oracle.torch_oracle.dgl_layer_forward in float64 on the host for a pna_amd PNALayer and its inputs."""
    from oracle import torch_oracle as O
    src, dst = graph.csr.col.long().cpu(), graph.csr.row.long().cpu()
    E = src.numel()
    e64 = torch.zeros(E, 0, dtype=torch.float64) if e is None else e.detach().double().cpu()[graph.csr.eid.long().cpu()]
    return O.dgl_layer_forward(_sd64(layer), src, dst, h.shape[0], h.detach().double().cpu(), e64, snorm.detach().double().cpu(), AGG.split(),
                               cfg["scalers"].split(), torch.tensor(float(avg_log), dtype=torch.float64), cfg["towers"], cfg["divide_input"],
                               cfg["graph_norm"], cfg["batch_norm"], cfg["residual"], e is not None)


def anchor_tower_small(y, y64):
    """test_gpu_tower_fused.py::test_tower_layer_small_vs_float64_and_large_graph_path: max error / max(1, max |y64|) <= 2e-5."""
    err = (y.double().cpu() - y64).abs().max().item() / max(1.0, y64.abs().max().item())
    assert err <= 2e-5, err
    return err


def anchor_tower_large(y, y64):
    """test_gpu_degree_groups.py::test_grouped_tower_layer_vs_reference_golden (one-kernel, degree-grouped and ordinary paths): at least
    99.9 % of the elements within 1e-5 relative + 1e-5 absolute.  (That test's per-element floor for cancelling rows needs the
    reference's own fp32 output, which synthetic inputs do not have: the share criterion is the part that carries over.)  A share
    cannot see ONE wrong row -- the hub row is 0.07 % of the elements -- so EVERY element is also held to the bar of
    test_gpu_tower_fused.py::test_tower_layer_small_vs_float64_and_large_graph_path: error <= 2e-5 max(1, max |y64|)."""
    err = (y.double().cpu() - y64).abs()
    worst = err.max().item() / max(1.0, y64.abs().max().item())
    row = (err.max(dim=1).values / y64.abs().max(dim=1).values.clamp(min=1.0)).max().item()
    share = (err <= 1e-5 * y64.abs() + 1e-5).double().mean().item()
    print(f"  anchor: max error / max(1, max |y64|) {worst:.2e}, worst row by its own scale {row:.2e}, share {share:.5f}")
    assert worst <= 2e-5, (worst, share)
    assert share >= 0.999, (share, err.max().item())
    return share


def anchor_simple(layer, graph, h, y, avg_log):
    """test_gpu_degree_groups.py::test_grouped_layer_rows_vs_float64: per row, max error / max(1, max |ref|) <= 2e-5 against float64."""
    from oracle import torch_oracle as O
    src, dst = graph.csr.col.long().cpu(), graph.csr.row.long().cpu()
    y64 = O.simple_layer_forward(_sd64(layer), src, dst, h.shape[0], h.detach().double().cpu(), list(layer.aggregators), list(layer.scalers),
                                 torch.tensor(float(avg_log), dtype=torch.float64), batch_norm=layer.batch_norm, residual=layer.residual)
    err = (y.double().cpu() - y64).abs().max(dim=1).values / y64.abs().max(dim=1).values.clamp(min=1.0)
    assert err.max().item() <= 2e-5, err.max().item()
    return err.max().item()
