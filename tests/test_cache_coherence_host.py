"""Cache coherence of the weight-derived operands that are pure torch, on CPU tensors: after a change of ANY tensor a
builder reads, the operands it returns for a warm layer equal, element for element, those of a fresh layer holding the same state.
Plus the census of the `_pna_amd_*` tags (cache_probe.CENSUS) and the copy / pickle behaviour of a warm layer's one-call plan."""
import copy
import ctypes
import io
import pathlib
import pickle

import pytest
import torch

import cache_probe as CP
from pna_amd import _cache
from pna_amd import functional as PF
from pna_amd.dgl import pna_layer as PL
from pna_amd.dgl.pna_layer import PNALayer, PNASimpleLayer


def _layer(in_dim=20, out_dim=20, towers=4, divide_input=False, seed=1):
    layer = PNALayer(in_dim, out_dim, CP.AGG, CP.SCA, {"log": torch.tensor(1.3)}, 0.0, True, True, towers=towers, divide_input=divide_input,
                     residual=True).eval()
    return CP.randomise(layer, seed)


def _flat(x):
    """The tensors of a builder's result, nested lists / tuples flattened, non-tensors dropped."""
    if torch.is_tensor(x):
        return [x]
    if isinstance(x, (list, tuple)):
        return [t for y in x for t in _flat(y)]
    return []


def _same(a, b):
    fa, fb = _flat(a), _flat(b)
    return len(fa) == len(fb) and all(x.shape == y.shape and torch.equal(x, y) for x, y in zip(fa, fb))


def _max_diff(a, b):
    return max(float((x.double() - y.double()).abs().max()) for x, y in zip(_flat(a), _flat(b)) if x.numel())


def _check_builder(make, builder, must_see):
    """For every state tensor of a warm layer: mutate it in place; the builder's operands equal a fresh layer's.  `must_see`: name parts
    of tensors the builder certainly reads -- their mutation must change the operands (so that the equality is not vacuous)."""
    layer = make()
    builder(layer), builder(layer)                                       # warm
    seen = set()
    for k, (name, t) in enumerate(CP.state_tensors(layer)):
        before = [x.clone() for x in _flat(builder(layer))]
        CP.perturb_(name, t, k)
        after = builder(layer)
        fresh = CP.fresh_like(make, layer)
        want = builder(fresh)
        assert _same(after, want), f"{name}: stale operands after an in-place update (max difference {_max_diff(after, want):.3e})"
        if not _same(before, after):
            seen.add(name)
    for part in must_see:
        names = [n for n, _ in CP.state_tensors(layer) if part in n]
        assert names and all(n in seen for n in names), (part, sorted(set(names) - seen))


def test_tower_pass_weights_follow_the_pretrans_tensors():
    """ADVICE r6, first item: _tower_pass_weights' dense term Wd and beta are built from every tower's PRETRANS weight[:, Fi:2Fi] and
    bias; its cache was accepted on the identity of the collapsed weight alone, whose key covers posttrans, mixing and BatchNorm only.
    On the parent commit this test fails: after towers[2].pretrans weight *= 1.5 and towers[1].pretrans bias += 0.3 the second call
    returned the FIRST call's Wd object (max |Wd - fresh| 1.3e-1, max |beta - fresh| 2.0e-1 at this seed)."""
    layer = _layer()
    towers, mix = list(layer.towers), layer.mixing_network
    first = PF._tower_pass_weights(layer, towers, mix)
    assert PF._tower_pass_weights(layer, towers, mix)[1] is first[1]      # warm: served from the cache
    with torch.no_grad():
        layer.towers[2].pretrans.fully_connected[0].linear.weight.mul_(1.5)
        layer.towers[1].pretrans.fully_connected[0].linear.bias.add_(0.3)
    second = PF._tower_pass_weights(layer, towers, mix)
    fresh = CP.fresh_like(_layer, layer)
    want = PF._tower_pass_weights(fresh, list(fresh.towers), fresh.mixing_network)
    print("max |Wd - fresh|", float((second[1] - want[1]).abs().max()), "max |beta - fresh|", float((second[2] - want[2]).abs().max()))
    assert second[1] is not first[1]
    assert torch.equal(second[1], want[1]) and torch.equal(second[2], want[2])
    assert not torch.equal(second[1], first[1]) and not torch.equal(second[2], first[2])
    assert _same(second, want)


def test_tower_collapsed_flat_and_pass_weights():
    _check_builder(lambda: _layer(divide_input=False), lambda l: PF._tower_collapsed_weights(l, list(l.towers), l.mixing_network, False),
                   ["posttrans", "batchnorm_h", "mixing_network"])
    _check_builder(lambda: _layer(divide_input=True), lambda l: PF._tower_flat_weights(l, list(l.towers), l.mixing_network),
                   ["posttrans", "batchnorm_h", "mixing_network"])
    _check_builder(lambda: _layer(divide_input=False), lambda l: PF._tower_pass_weights(l, list(l.towers), l.mixing_network),
                   ["pretrans", "posttrans", "batchnorm_h", "mixing_network"])


def test_flat_weights_are_the_permuted_collapsed_weight():
    """_tower_flat_weights is accepted on the identity of the collapsed weight: sound, because it reads nothing else -- pinned here."""
    layer = _layer(divide_input=True)
    towers, mix = list(layer.towers), layer.mixing_network
    Wp = PF._tower_flat_weights(layer, towers, mix)[0]
    assert PF._tower_flat_weights(layer, towers, mix)[0] is Wp
    Wv, K = PF._tower_collapsed_weights(layer, towers, mix, True)[0], PF._tower_collapsed_weights(layer, towers, mix, True)[4]
    assert Wp.shape == Wv.shape and torch.equal(torch.sort(Wp, dim=1).values, torch.sort(Wv, dim=1).values) and Wv.shape[1] % K == 0
    with torch.no_grad():
        layer.mixing_network.linear.weight.mul_(2.0)
    Wp2 = PF._tower_flat_weights(layer, towers, mix)[0]
    assert Wp2 is not Wp and torch.equal(Wp2, Wp * 2.0)


def test_projection_caches():
    see = ["pretrans"]
    _check_builder(_layer, lambda l: PL._projection_cache(list(l.towers), l.towers[0].in_dim), see)
    _check_builder(lambda: _layer(20, 20, 1), lambda l: PL._projection_cache_padded(l.towers[0], 20, 24), see)
    _check_builder(lambda: _layer(20, 20, 4, True), lambda l: PL._projection_cache_padded_div(list(l.towers), 5, 24), see)
    _check_builder(_layer, lambda l: PL._projection_cache_padded_multi(list(l.towers), 20, 24), ["pretrans.fully_connected.0.linear.weight"])


@pytest.mark.parametrize("fold,dtype", [(PF._fold_batchnorm, torch.float32), (PF._fold_batchnorm_f32, torch.bfloat16)])
def test_fold_batchnorm_follows_its_tensors(fold, dtype):
    make = lambda: CP.randomise(_Bn(dtype), 3)    # noqa: E731
    _check_builder(make, lambda m: fold(m.batchnorm_h), ["weight", "bias", "running_mean", "running_var"])
    m = make()
    a = fold(m.batchnorm_h)
    m.batchnorm_h.weight.data = m.batchnorm_h.weight.data.clone() * 2                       # same version counter, new address
    b = fold(m.batchnorm_h)
    assert not _same(a, b) and _same(b, fold(CP.fresh_like(make, m).batchnorm_h))


class _Bn(torch.nn.Module):
    def __init__(self, dtype):
        super().__init__()
        self.batchnorm_h = torch.nn.BatchNorm1d(12).to(dtype)
        self.eval()


def test_stack_cached_follows_its_tensors():
    owner = torch.nn.Linear(2, 2)
    ts = [torch.randn(5) for _ in range(3)]
    first = PF._stack_cached(owner, "_pna_amd_bias_stack", ts)
    assert PF._stack_cached(owner, "_pna_amd_bias_stack", ts) is first
    for i in range(3):
        ts[i].add_(1.0)
        got = PF._stack_cached(owner, "_pna_amd_bias_stack", ts)
        assert torch.equal(got, torch.stack(ts)), i
    ts[2] = ts[2].clone() * 3                                            # another tensor in the same slot
    assert torch.equal(PF._stack_cached(owner, "_pna_amd_bias_stack", ts), torch.stack(ts))
    for tag in ("_pna_amd_cs_stack", "_pna_amd_ct_stack"):               # (the same function under the other two tags)
        assert torch.equal(PF._stack_cached(owner, tag, ts), torch.stack(ts))
        ts[0].mul_(2.0)
        assert torch.equal(PF._stack_cached(owner, tag, ts), torch.stack(ts))


class _Owner:
    """Any object with a __dict__ can own an entry."""


def _counting(value_of):
    calls = []

    def build():
        calls.append(torch.is_grad_enabled())
        return value_of()
    return build, calls


def test_memo_serves_the_same_object_and_rebuilds_on_every_visible_change():
    """_cache.memo, the one helper behind every weight-derived cache: a warm call returns the first call's object; each way torch shows a
    change of a keyed tensor -- and a changed `extra` -- rebuilds."""
    owner = _Owner()
    a, b = torch.nn.Parameter(torch.randn(3, 4)), torch.randn(4)
    build, calls = _counting(lambda: a.detach().sum() + b.sum())
    get = lambda ts=None, extra=7: _cache.memo(owner, "_pna_amd_test", [a, b] if ts is None else ts, extra, build)      # noqa: E731
    first = get()
    assert get() is first and get() is first and len(calls) == 1
    with torch.no_grad():
        a.mul_(2.0)                                                      # an in-place write to a keyed tensor
    second = get()
    assert len(calls) == 2 and second is not first and torch.equal(second, a.detach().sum() + b.sum())
    b.add_(1.0)                                                          # ... to any of them
    assert torch.equal(get(), a.detach().sum() + b.sum()) and len(calls) == 3
    a.data = a.data.clone() * 3                                          # `t.data = other`: same object, same version counter, new address
    assert torch.equal(get(), a.detach().sum() + b.sum()) and len(calls) == 4
    assert get() is get() and len(calls) == 4
    none = get([a, None])                                                # a slot that holds no tensor ...
    assert len(calls) == 5 and get([a, None]) is none and len(calls) == 5
    get([a, b])                                                          # ... becoming a tensor
    assert len(calls) == 6
    get([a, None])                                                       # ... and back
    assert len(calls) == 7
    get([a, None], extra=8)                                              # a changed `extra`
    assert len(calls) == 8
    get([a, None], extra=8)
    assert len(calls) == 8
    entry = owner.__dict__["_pna_amd_test"]
    assert type(entry) is tuple and len(entry) == 3 and entry[0] == (_cache.tensor_key([a, None]), 8)


def test_memo_tells_two_tensors_at_one_version_and_address_apart():
    """Two views of one buffer share the version counter and the address: only the object differs.  The (version, address, device) keys
    this helper replaced served the first view's entry for the second."""
    owner, buf = _Owner(), torch.randn(12)
    v1, v2 = buf.view(-1), buf.view(-1)
    assert v1 is not v2 and v1._version == v2._version and v1.data_ptr() == v2.data_ptr() and v1.shape == v2.shape
    build, calls = _counting(lambda: torch.zeros(1))
    first = _cache.memo(owner, "_pna_amd_test", [v1], None, build)
    assert _cache.memo(owner, "_pna_amd_test", [v1], None, build) is first and len(calls) == 1
    assert _cache.memo(owner, "_pna_amd_test", [v2], None, build) is not first and len(calls) == 2


def test_memo_entry_holds_its_keyed_tensors():
    """While an entry is live the ids and addresses in its key cannot be handed to another tensor: the entry keeps the tensors."""
    owner = _Owner()
    t = torch.randn(5)
    ident = id(t)
    _cache.memo(owner, "_pna_amd_test", [t, None], None, lambda: t.sum())
    del t
    held = owner.__dict__["_pna_amd_test"][2]
    assert [id(x) for x in held if x is not None] == [ident]
    assert owner.__dict__["_pna_amd_test"][0][0][0][0] == ident          # ... the object the key names
    # a tensor that owns its entry is not held by it (it outlives the entry anyway; holding it would be a reference cycle)
    w, other = torch.randn(3), torch.randn(3)
    _cache.memo(w, "_pna_amd_test", [w, other], None, lambda: w + other)
    assert [x is other for x in w.__dict__["_pna_amd_test"][2]] == [True]


def test_memo_builds_without_gradients():
    owner = _Owner()
    w = torch.nn.Parameter(torch.randn(3))
    build, calls = _counting(lambda: w * 2.0)
    with torch.enable_grad():
        assert torch.is_grad_enabled()
        value = _cache.memo(owner, "_pna_amd_test", [w], None, build)
        assert torch.is_grad_enabled()                                   # (the caller's mode is back)
    assert calls == [False] and not value.requires_grad


def test_bf16_edge_table_is_built_once_per_state_of_the_rows(monkeypatch):
    """PNANet registers its embedding weight on the graph in every forward, and the graph keeps `weight.detach()`: a NEW tensor object
    per forward over the same storage and version counter.  The bf16 edge table must be built once per state of the weight, not per
    alias -- its key leaves the object out (a rebuild is a kernel launch and allocations per layer and forward, and a captured graph
    would replay it)."""
    built = []
    monkeypatch.setattr(PF.ops, "contract_bf16", lambda rows, ed, img, width: (built.append(rows), rows.float() @ img[0, :width, :ed].float().t())[1])
    w = torch.nn.Parameter(torch.randn(4, 6))
    im = {"edge": torch.randn(1, 16, 32), "etab": None}
    a, b = w.detach(), w.detach()
    assert a is not b and a.data_ptr() == b.data_ptr() and a._version == b._version
    first = PF._small_edge_table_bf16(im, a, 6, 8)
    assert PF._small_edge_table_bf16(im, b, 6, 8) is first and PF._small_edge_table_bf16(im, w.detach(), 6, 8) is first and len(built) == 1
    with torch.no_grad():
        w.mul_(2.0)                                                      # a new state of the weight: seen through any alias
    second = PF._small_edge_table_bf16(im, w.detach(), 6, 8)
    assert len(built) == 2 and torch.equal(second, first * 2.0)
    assert PF._small_edge_table_bf16(im, b, 6, 8) is second and len(built) == 2
    w.data = w.data.clone() + 1.0                                        # same version counter, new address
    assert not torch.equal(PF._small_edge_table_bf16(im, w.detach(), 6, 8), second) and len(built) == 3


def test_avg_log_value_follows_the_tensor():
    avg = {"log": torch.tensor(1.25)}
    assert PL._avg_log_value(avg) == 1.25 and PL._avg_log_value(avg) == 1.25
    avg["log"].mul_(2.0)                                                 # edited in place
    assert PL._avg_log_value(avg) == 2.5
    avg["log"].data = torch.tensor(3.0)                                  # same version counter, new address
    assert PL._avg_log_value(avg) == 3.0
    avg["log"] = torch.tensor(0.5)                                       # another tensor
    assert PL._avg_log_value(avg) == 0.5
    assert PL._avg_log_value({"log": 0.75}) == 0.75


def test_graph_of_follows_edge_index_edits():
    from pna_amd.pytorch_geometric.pna import _graph_of
    ei = torch.tensor([[0, 1, 2, 3, 0], [1, 2, 3, 0, 2]])
    g0 = _graph_of(ei, 4)
    assert _graph_of(ei, 4) is g0
    col0 = g0.csr.col.clone()                                            # (the CSR is built on first use: before the edit)
    ei[0, 4] = 1                                                         # an edge rewired in place
    g1 = _graph_of(ei, 4)
    want = _graph_of(ei.clone(), 4)
    assert g1 is not g0
    for a, b in zip(g1.csr[:4], want.csr[:4]):
        assert torch.equal(a, b)
    assert not torch.equal(g1.csr.col, col0)
    assert _graph_of(ei, 5) is not g1                                    # another node count: another graph


def test_sparsify_follows_adjacency_edits():
    from pna_amd.pytorch.pna.sparsify import sparsify
    gen = torch.Generator().manual_seed(0)
    adj = (torch.rand(2, 6, 6, generator=gen) < 0.4).float()
    s0 = sparsify(adj, False)
    assert sparsify(adj, False) is s0
    adj[0, 1, 2] = 1.0 - adj[0, 1, 2]                                    # one entry flipped in place
    s1 = sparsify(adj, False)
    want = sparsify(adj.clone(), False)
    assert s1 is not s0
    assert torch.equal(s1.by_row.csr.col, want.by_row.csr.col) and torch.equal(s1.by_row.csr.rowptr, want.by_row.csr.rowptr)
    assert torch.equal(s1.by_col.csr.col, want.by_col.csr.col) and torch.equal(s1.w_row, want.w_row) and torch.equal(s1.w_col, want.w_col)
    assert s1.by_row.csr.col.numel() != s0.by_row.csr.col.numel()


def test_data_edits_are_a_documented_blind_spot():
    """DESIGN.md 4.13, INTEGRATION.md: an in-place edit THROUGH `.data` changes neither the version counter nor the address -- no key can
    see it (torch's optimizers, nn.init and load_state_dict do not write that way).  Pinned, so that the documents stay true."""
    layer = _layer()
    towers = list(layer.towers)
    w = towers[0].pretrans.fully_connected[0].linear.weight
    first = PL._projection_cache(towers, 20)[0]
    v = w._version
    w.data.mul_(2.0)
    assert w._version == v
    assert PL._projection_cache(towers, 20)[0] is first                  # stale, by design
    with torch.no_grad():
        w.mul_(1.0)                                                      # any visible write makes the cache follow
    assert not torch.equal(PL._projection_cache(towers, 20)[0], first)


def test_census_names_every_cache_tag():
    """Every `_pna_amd_*` tag in the sources has a row in cache_probe.CENSUS naming the case that exercises it, or an exemption with
    its reason: the next cache cannot arrive without a coherence case."""
    found = CP.source_tags()
    assert len(found) >= 30, sorted(found)
    missing = sorted(set(found) - set(CP.CENSUS))
    assert not missing, f"cache tags without a coherence case in tests/cache_probe.py CENSUS: {missing} ({[found[m] for m in missing]})"
    gone = sorted(set(CP.CENSUS) - set(found))
    assert not gone, f"CENSUS rows for tags that no longer exist: {gone}"
    for tag, (kind, where, note) in CP.CENSUS.items():
        assert kind in ("host", "gpu", "exempt") and note, tag
        if kind == "exempt":
            assert "topology only" in note or "reads no tensor value" in note or "writes it before reading it" in note, (tag, note)
        else:
            assert "test_" in where, tag
    # the host cases the table names exist
    import re
    import sys
    me = sys.modules[__name__]
    for tag, (kind, where, _) in CP.CENSUS.items():
        for name in re.findall(CP.HOST.replace(".", r"\.") + r"::(test_\w+)", where):
            assert callable(getattr(me, name, None)), (tag, name)
        if kind == "host":
            assert CP.HOST + "::test_" in where, tag
    # the GPU cases the table names exist and ASSERT the tag: a path holds it in its asserted tag list, a named case is in the file
    import test_gpu_cache_coherence as G
    for tag, (kind, where, _) in CP.CENSUS.items():
        if CP.GPU in where:
            assert tag in CP.CENSUS_GPU, f"{tag}: the census names the GPU file but CENSUS_GPU has no entry"
        assert kind != "gpu" or tag in CP.CENSUS_GPU, tag
    for tag, how in CP.CENSUS_GPU.items():
        assert tag in CP.CENSUS and CP.CENSUS[tag][0] != "exempt", tag
        if isinstance(how, str):
            assert callable(getattr(G, how, None)), (tag, how)
            assert f'"{tag}"' in pathlib.Path(G.__file__).read_text(), f"{how} does not name {tag}"
        else:
            assert how, tag
            for path in how:
                assert path in G.PATHS, (tag, path)
                assert tag in G.PATHS[path][7], f"path {path} does not assert {tag}"
            for path, star in re.findall(r"\b((?:tower|simple|bf16)_\w+)(\*?)", CP.CENSUS[tag][1].split(CP.GPU, 1)[1]):
                assert path in how or (star and any(h.startswith(path) for h in how)), f"{tag}: the census row names path {path}, CENSUS_GPU does not"


def _stand_in_plan(cls):
    """An object shaped like a warm one-call plan: the ctypes argument block and its byref (a real plan needs the GPU to be built)."""
    from pna_amd import _lib
    plan = cls.__new__(cls)
    plan.args = _lib.PnaTowerLayerArgs()
    plan.ref = ctypes.byref(plan.args)
    plan.keep = {"proj_img": torch.zeros(4)}
    plan.ts, plan.versions, plan.divide_input = [], [], False
    return plan


@pytest.mark.parametrize("cls", [PF._SmallTowerPlan, PF._SmallSimplePlan])
def test_warm_layer_copies_without_its_plan(cls):
    """copy.deepcopy / pickle / torch.save of a layer that has served a molecule batch: the plan (ctypes block: not copyable, pointing into
    the ORIGINAL's device buffers) is dropped, the copy builds its own on first use."""
    from pna_amd import _lib
    with pytest.raises((ValueError, TypeError)):
        copy.deepcopy(_lib.PnaTowerLayerArgs())                          # why the plan cannot simply be copied
    layer = _layer() if cls is PF._SmallTowerPlan else PNASimpleLayer(8, 8, CP.AGG, CP.SCA, {"log": torch.tensor(1.0)}, 0.0, True, True).eval()
    layer.__dict__["_pna_amd_small"] = plan = _stand_in_plan(cls)
    clone = copy.deepcopy(layer)
    assert clone.__dict__.get("_pna_amd_small") is None and layer.__dict__["_pna_amd_small"] is plan
    via_pickle = pickle.loads(pickle.dumps(layer))
    assert via_pickle.__dict__.get("_pna_amd_small") is None
    buf = io.BytesIO()
    torch.save(layer, buf)
    buf.seek(0)
    loaded = torch.load(buf, weights_only=False)
    assert loaded.__dict__.get("_pna_amd_small") is None
    for other in (clone, via_pickle, loaded):
        for (n, a), (_, b) in zip(CP.state_tensors(layer), CP.state_tensors(other)):
            assert torch.equal(a, b) and a.data_ptr() != b.data_ptr(), n


def test_a_conversion_drops_every_cached_operand():
    """.to() / .float() / .cuda() give every parameter NEW storage under an UNCHANGED version counter, and the allocator may hand the
    converted tensor the address its predecessor freed: .to(bfloat16).float() rounds every weight and can leave every (version, address,
    device) key as it was.  So a conversion drops the caches (functional.drop_weight_caches, from `_apply`) instead of trusting the keys:
    after it the operands are a fresh layer's, whatever addresses the allocator chose, and no tag is left on the layer, a submodule, a
    parameter or a buffer."""
    layer = _layer()
    towers, mix = list(layer.towers), layer.mixing_network
    build = lambda l: (PF._tower_pass_weights(l, list(l.towers), l.mixing_network), PL._projection_cache(list(l.towers), 20),
                       [PF._fold_batchnorm(t.batchnorm_h) for t in l.towers])      # noqa: E731
    first = [x.clone() for x in _flat(build(layer))]
    build(layer)
    w = towers[-1].posttrans.fully_connected[0].linear.weight
    w._pna_amd_pack = ("a stand-in for the packed image ops.py keeps on the weight",)
    w._pna_amd_group_img = ("a stand-in for the combined images degree_groups.py keeps on the weight",)
    PL._projection_cache_padded_multi(towers, 20, 24)                    # (one tag of every file that caches through _cache.memo)
    PF._mix_image_bf16(mix)
    PL._avg_log_value({"log": towers[0].batchnorm_h.num_batches_tracked})                   # (a buffer in the place of avg_d['log'])
    assert {"_pna_amd_pass_w", "_pna_amd_collapsed", "_pna_amd_proj", "_pna_amd_fold", "_pna_amd_pack", "_pna_amd_group_img",
            "_pna_amd_proj_pad_multi", "_pna_amd_bf16_mix", "_pna_amd_float"} <= CP.warm_tags(layer)
    layer.to(torch.bfloat16).float()
    assert not CP.warm_tags(layer), sorted(CP.warm_tags(layer))
    after = build(layer)
    assert _same(after, build(CP.fresh_like(_layer, layer)))
    assert not _same(first, after)                                       # the rounding to bf16 is visible in the operands
    # a layer inside a module of the caller's: the conversion of the parent reaches the hook
    parent = torch.nn.Sequential(layer)
    build(layer)
    assert CP.warm_tags(layer)
    parent.double().float()
    assert not CP.warm_tags(layer)
