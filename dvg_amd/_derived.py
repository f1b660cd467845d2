"""Tensors derived from parameters, remembered until the parameter changes - and the list of every module-level cache.

`derived(owner, tag, sources, build)` is the one place that implements "look up by owner, compare (data_ptr, _version),
rebuild on mismatch, store": packed / transposed / Winograd-domain weights, BatchNorm folds, GEMM-operand forms.

Correctness under hipGraph capture needs two operations over ALL module-level caches of the package (see
graphs.drop_version_keyed_caches / graphs.snapshot_eager_caches): forget everything, and hold everything alive.  A cache
that lives at module level calls `register` next to its definition, or it is neither dropped nor kept alive.  The caches keyed
on a rollout's skip tensors name their dicts there as well: graph holders forget what ONE capture added to them
(`skip_mark` / `skip_drop_since`).

Imports torch and weakref only, so that every module of the package can import it."""
from __future__ import annotations

import weakref

import torch

_registry = {}     # name -> (clear, tensors)
_skip_keyed = []   # the dicts whose entries depend on a rollout's skip tensors


def register(name: str, clear, tensors, skip_keyed=()) -> None:
    """clear(): forget every entry.  tensors(): an iterable of what the cache holds now (nested containers allowed).
    skip_keyed: the cache's dicts, if its entries are keyed on skip activations."""
    if name in _registry:
        raise RuntimeError(f"cache {name!r} is registered twice")
    _registry[name] = (clear, tensors)
    _skip_keyed.extend(skip_keyed)


def skip_mark() -> list:
    """The keys the skip-keyed caches hold now."""
    return [set(d) for d in _skip_keyed]


def skip_drop_since(mark) -> None:
    """Forget every entry of the skip-keyed caches whose key was not there at `mark`."""
    for d, had in zip(_skip_keyed, mark):
        for k in [k for k in d if k not in had]:
            del d[k]


def registered() -> tuple:
    return tuple(_registry)


def drop_all() -> None:
    for clear, _ in _registry.values():
        clear()


def snapshot() -> list:
    """Strong references to every tensor the registered caches hold right now."""
    keep = []

    def walk(o):
        if torch.is_tensor(o):
            keep.append(o)
        elif isinstance(o, (tuple, list)):
            for v in o:
                walk(v)
        elif isinstance(o, dict):
            for v in o.values():
                walk(v)
        elif hasattr(o, "__dict__") and type(o).__module__.startswith("dvg_amd"):
            walk(vars(o))          # ops.WinoV and similar small holders

    for _, tensors in _registry.values():
        walk(list(tensors()))
    return keep


def version_key(*ts) -> tuple:
    """What `derived` compares: a tensor updated in place, re-allocated or replaced has another key (None stays None)."""
    return tuple([(t.data_ptr(), t._version) if t is not None else None for t in ts])


_store = {}        # id(owner) -> (weakref(owner), {tag: (version_key(*sources), value)}); gone with its owner
register("derived", _store.clear, lambda: [slot for _, slot in _store.values()])


def drop_derived() -> None:
    """Forget what `derived` holds and nothing else (the other registered caches stay)."""
    _store.clear()


def derived_mark() -> dict:
    """What `derived` holds now, entry by entry (the tensors are referenced, not copied): for derived_restore."""
    return {k: (ref, dict(slot)) for k, (ref, slot) in _store.items()}


def derived_restore(mark: dict) -> None:
    """Make `derived` hold what it held at `mark` again: entries built since are forgotten, entries replaced since come back.
    For a pass that must leave no trace while the parameters stay what they are (validate.Validator.run): every entry that
    comes back is as valid for its key as it was at the mark."""
    _store.clear()
    _store.update({k: (ref, dict(slot)) for k, (ref, slot) in mark.items() if ref() is not None})


def _forget(ref, key):
    if key in _store and _store[key][0] is ref:        # (the id may already belong to a new owner)
        del _store[key]


def derived(owner, tag, sources, build):
    """The value build() returned last time for (owner, tag) while every tensor of `sources` is what it was then; else
    build(), stored.  owner: an nn.Module or a parameter (not kept alive); tag: hashable; None is a legal value."""
    ent = _store.get(id(owner))
    if ent is None or ent[0]() is not owner:
        ent = _store[id(owner)] = (weakref.ref(owner, lambda ref, key=id(owner): _forget(ref, key)), {})
    key = version_key(*sources)
    hit = ent[1].get(tag)
    if hit is not None and hit[0] == key:
        return hit[1]
    value = build()
    ent[1][tag] = (key, value)
    return value


_zero_states = {}  # (device, rows, columns) -> all-zero tensor, read only
register("zero_state", _zero_states.clear, _zero_states.values)


def zero_state(b: int, h: int, dev):
    """One shared all-zero (b, h) tensor per device and shape: the initial (h, c) of every LSTM sequence, read only (no
    kernel of the recurrent path writes its state in place).  None when it would have to be created while the current
    stream is capturing: a tensor that lives in a graph's private pool is never cached, the caller makes its own."""
    key = (str(dev), b, h)
    z = _zero_states.get(key)
    if z is None and not torch.cuda.is_current_stream_capturing():
        z = _zero_states[key] = torch.zeros((b, h), device=dev)
    return z
