"""The one memo behind every weight-derived operand cache: packed weight images, collapsed weights, folded BatchNorm
constants, padded projections -- whatever a fast path builds from parameters and buffers and keeps under a `_pna_amd_*` tag on a module
or a tensor.  A call site reads  memo(owner, "_pna_amd_<tag>", [tensors the builder reads], extra, build).
"""
import torch


def tensor_key(ts):
    """The state of a list of tensors as far as torch shows it: per tensor the object, its version counter (in-place writes, in-place
    transposes), its address (`t.data = other`: EMA / SWA swaps, offloading), device, dtype and shape; None stays None, so a bias that
    appears or disappears changes the key.  The device and shape OBJECTS compare like their string / tuple forms at a third of the cost.
    No stride: every in-place change of a tensor's strides bumps its version counter, and `w.data = w.data.t()` on a square weight
    belongs to the documented blind spot of `.data` edits."""
    return tuple([t if t is None else (id(t), t._version, t.data_ptr(), t.device, t.dtype, t.shape) for t in ts])


def memo(owner, tag, tensors, extra, build):
    """build() -- run without gradients -- cached in owner.__dict__[tag] (a module, a tensor, any object with a __dict__) as the entry
    (key, value, tensors), key = (tensor_key(tensors), extra).  The entry HOLDS the keyed tensors: while a key is live, none of the
    ids and addresses in it can be handed to another tensor.  The one exception is `owner` itself where it is among the keyed tensors
    (a weight that carries its own image): it outlives its own entry anyway, and a tensor holding itself would keep its images until
    the cycle collector runs.
    `tensors` must be objects that are the SAME from call to call (parameters, buffers, cached operands): a fresh `w.detach()` per call
    is a new state to this key.  A cache over such aliases keeps a key of its own (functional._small_edge_table_bf16)."""
    key = (tensor_key(tensors), extra)
    d = owner.__dict__
    hit = d.get(tag)
    if hit is not None and hit[0] == key:
        return hit[1]
    with torch.no_grad():
        value = build()
    d[tag] = (key, value, [t for t in tensors if t is not owner])
    return value


def drop_weight_caches(module):
    """Remove every `_pna_amd_*` entry from `module`, its submodules and their parameters and buffers.  Called from `_apply` (.to(),
    .float(), .cuda(), ...): there every parameter gets NEW storage under an UNCHANGED version counter, and the allocator may hand the
    converted tensor the address its predecessor just freed (.to(bfloat16).float() does exactly that) -- no key over (object, version,
    address) can tell that state from the one the caches were built for.  Nothing on the per-call path: the next call rebuilds."""
    for m in module.modules():
        for owner in [m, *m._parameters.values(), *m._buffers.values()]:
            d = getattr(owner, "__dict__", None)
            if d:
                for tag in [k for k in d if isinstance(k, str) and k.startswith("_pna_amd_")]:
                    del d[tag]


class DropsCachesOnConversion:
    """Mixin of every layer and net (before nn.Module in the bases): a conversion -- `_apply`, the one route of .to(), .float(), .cuda(),
    .cpu() -- drops every cached operand below the module.  A submodule of another class converted ON ITS OWN
    (`layer.mixing_network.to(...)`) does not pass here: convert the layer."""

    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        drop_weight_caches(self)
        return out
